"""paq8's DMC forest as a device building block, without a GPU: the step functions of cmx_p8s_dmc_kernel (cmix_amd/csrc/p8dmc_dev.h:
one lane per state graph, cooperative reset) run on the host by tests/host/p8dmc_emul.cpp against the oracle's restatement
(oracle/paq8_dmc.c, pinned against the reference's own classes): the 6 mixer inputs of every bit, at level 0 (the graphs
fill within a few KB and the eight fast models are reset again and again) and at level 5. The same comparison runs on the
device in tests/test_zgpu_p8dmc.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_p8cm2_host import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "host", "libp8dmcemul.so")
SRC = os.path.join(ROOT, "tests", "host", "p8dmc_emul.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "cmix_amd", "csrc", f) for f in ("p8dmc_dev.h", "p8dmc_build.h", "p8cm2_dev.h")]


def emul():
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", SO, SRC])
    L = C.CDLL(SO)
    L.p8x_create.restype = C.c_void_p
    L.p8x_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.p8x_destroy.argtypes = [C.c_void_p]
    L.p8x_resets.restype = C.c_uint64
    L.p8x_resets.argtypes = [C.c_void_p]
    L.p8x_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return L


def oracle_rows(level, data):
    lib = O.lib()
    lib.orc_p8_dmc_new.restype = C.c_void_p
    lib.orc_p8_dmc_new.argtypes = [C.c_int]
    lib.orc_p8_dmc_mix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.orc_p8_dmc_free.argtypes = [C.c_void_p]
    f = lib.orc_p8_dmc_new(level)
    rows = np.zeros((8 * len(data), 6), np.int16)
    o, y = np.zeros(8, np.int16), 0
    for n in range(len(data)):
        for bpos in range(8):
            assert lib.orc_p8_dmc_mix(f, y, bpos, o.ctypes.data) == 6
            rows[8 * n + bpos] = o[:6]
            y = (int(data[n]) >> (7 - bpos)) & 1
    lib.orc_p8_dmc_free(f)
    return rows


CASES = [(0, 40000), (5, 12000)]


@pytest.mark.parametrize("level,nbytes", CASES)
def test_vs_oracle(level, nbytes):
    from cmix_amd import synth
    L = emul()
    data = np.frombuffer(synth.enwik_like(nbytes, 29), np.uint8)
    want = oracle_rows(level, data)
    nex, stretch, _ = tables()
    h = L.p8x_create(level, nex.ctypes.data, stretch.ctypes.data)
    bits = np.unpackbits(np.ascontiguousarray(data))
    got = np.zeros((len(bits), 6), np.int16)
    pos = 0
    for n in [3, 13, 8000, 1 << 30]:        # chunks need not be whole bytes here
        n = min(n, len(bits) - pos)
        if n <= 0:
            break
        b, o = np.ascontiguousarray(bits[pos:pos + n]), got[pos:pos + n]
        L.p8x_run(h, b.ctypes.data, n, o.ctypes.data)
        pos += n
    resets = L.p8x_resets(h)
    L.p8x_destroy(h)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first mismatch (bit, input):", bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (resets > 0) == (level == 0), resets


POISON = [0xFF, 0xA5, 0x00]   # what the LDS model holds when a run ("launch") begins: all bits set, a non-trivial byte, a fresh device's zeros
_poison_ref = {}


@pytest.mark.parametrize("poison", POISON)
def test_poisoned_lds_vs_oracle(poison):
    """Nothing the body reads from P8DmcShared (the ten stretched predictions, the reset flags) may be what the previous launch left there:
    refilled with a byte at the start of every run, ragged chunks -- ends inside a byte included -- still give the oracle's rows, resets and all."""
    level = 0
    if not _poison_ref:
        from cmix_amd import synth
        data = np.frombuffer(synth.enwik_like(40000, 29), np.uint8)
        _poison_ref["case"] = (data, oracle_rows(level, data))
    data, want = _poison_ref["case"]
    L = emul()
    L.p8x_set_poison.argtypes = [C.c_void_p, C.c_int]
    nex, stretch, _ = tables()
    h = L.p8x_create(level, nex.ctypes.data, stretch.ctypes.data)
    L.p8x_set_poison(h, poison)
    bits = np.unpackbits(np.ascontiguousarray(data))
    got = np.zeros((len(bits), 6), np.int16)
    pos = 0
    for n in [1, 3, 13, 8000, 150000, 1 << 30]:
        n = min(n, len(bits) - pos)
        if n <= 0:
            break
        b, o = np.ascontiguousarray(bits[pos:pos + n]), got[pos:pos + n]
        L.p8x_run(h, b.ctypes.data, n, o.ctypes.data)
        pos += n
    resets = L.p8x_resets(h)
    L.p8x_destroy(h)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("poison 0x%02X" % poison, "first mismatch (bit, input):", bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert resets > 0, resets


def test_vs_golden_columns():
    """cmix sees paq8's mixer inputs as squash(x) / 4095 (paq8.cpp:542-545). The forest's six inputs at cmix's level 11,
    started the way paq8's Predictor starts (first call after one coded bit), must appear as six consecutive layer-0
    columns of the golden trace recorded from the unmodified reference predictor, from the second byte on (during the
    first byte the context maps ahead of it emit nothing and the columns sit elsewhere). Fixtures only; the test finds
    the columns rather than assuming them and requires the match to be unique."""
    import make_golden as mg
    from conftest import load_golden
    lib = O.lib()
    lib.orc_p8_squash.argtypes = [C.c_int]
    g = load_golden("text_96")
    probs, data = mg.unpack_probs(g), np.ascontiguousarray(g["stream"], np.uint8)
    bits = np.unpackbits(data)
    L = emul()
    L.p8x_seed.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    nex, stretch, _ = tables()
    h = L.p8x_create(11, nex.ctypes.data, stretch.ctypes.data)
    L.p8x_seed(h, int(bits[0]), 1)
    rest = np.ascontiguousarray(bits[1:])
    out = np.zeros((len(rest), 6), np.int16)          # row j = the inputs before bit j + 1
    L.p8x_run(h, rest.ctypes.data, len(rest), out.ctypes.data)
    L.p8x_destroy(h)
    sq = np.array([lib.orc_p8_squash(int(v)) for v in range(-2048, 2048)], np.int32)
    got = sq[np.clip(out[7:].astype(np.int32), -2047, 2047) + 2048].astype(np.float32) * np.float32(1.0 / 4095)
    rows = probs[8:8 + len(got)]
    hits = [k for k in range(434, 2025 - 5) if np.array_equal(rows[:, k:k + 6].view(np.uint32), got.view(np.uint32))]
    assert len(hits) == 1, hits
