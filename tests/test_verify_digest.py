"""CPU: the digest of the mixing network's verify mode (cmix_amd/csrc/cmx_verify.h, include/cmix_amd.h cmx_mixnet_set_verify), built for the host
(tests/host/verify_digest.cpp) and checked against a numpy restatement: the mix of (class, bit, index, word), block sums mod 2^64 that do not depend on
the order in which waves fold their words, and the property the mode rests on -- any single changed word changes its block's sum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "verify_digest.cpp")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def vd(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("verify") / "libverifydigest.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.vd_mix.restype = C.c_uint64
    L.vd_mix.argtypes = [C.c_uint32] * 4
    L.vd_key.restype = C.c_uint64
    L.vd_key.argtypes = [C.c_uint32] * 5
    L.vd_mix_class.restype = C.c_uint32
    L.vd_mix_class.argtypes = [C.c_uint32]
    L.vd_block_sums.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


def np_mix(c, t, i, w):
    """cmx_vmix restated: key = ((c << 60) ^ (t << 24) ^ i) * golden, then splitmix64's finaliser over key ^ w (uint64 arithmetic wraps mod 2^64)."""
    u = np.uint64
    c, t, i, w = (np.asarray(x).astype(np.uint64) for x in (c, t, i, w))
    with np.errstate(over="ignore"):
        x = ((c << u(60)) ^ (t << u(24)) ^ i) * u(0x9E3779B97F4A7C15)
        x = x ^ w
        x = x ^ (x >> u(30))
        x = x * u(0xBF58476D1CE4E5B9)
        x = x ^ (x >> u(27))
        x = x * u(0x94D049BB133111EB)
        x = x ^ (x >> u(31))
    return x


def np_block_sums(c, t0, words):
    T, n = words.shape
    t = np.repeat(np.arange(T, dtype=np.uint64) + np.uint64(t0), n).reshape(T, n)
    i = np.tile(np.arange(n, dtype=np.uint64), T).reshape(T, n)
    m = np_mix(c, t, i, words)
    nb = (T + 63) // 64
    out = np.zeros(nb, np.uint64)
    with np.errstate(over="ignore"):
        for b in range(nb):
            out[b] = m[64 * b:64 * b + 64].sum(dtype=np.uint64)
    return out


def host_block_sums(vd, c, t0, words):
    words = np.ascontiguousarray(words, np.uint32)
    T, n = words.shape
    out = np.zeros((T + 63) // 64, np.uint64)
    vd.vd_block_sums(c, t0, words.ctypes.data, T, n, out.ctypes.data)
    return out


def test_mix_matches_numpy_restatement(vd):
    rng = np.random.default_rng(1)
    for _ in range(2000):
        c, t, i, w = int(rng.integers(1, 10)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 2112)), int(rng.integers(0, 1 << 32))
        assert vd.vd_mix(c, t, i, w) == int(np_mix(c, t, i, w))
    assert vd.vd_mix(9, 260025, 2077, 0xFFFFFFFF) == int(np_mix(9, 260025, 2077, 0xFFFFFFFF))
    # the words the tail waves and the helpers fold are the same words as the gather's and the stretch waves': one mix class each
    assert [vd.vd_mix_class(k) for k in range(1, 10)] == [1, 2, 3, 4, 4, 4, 7, 7, 9]


def test_mix_is_a_bijection_in_the_word():
    """For a fixed (class, bit, index) no two words share a mixed value (a sample of 2^20 words; the map is XOR then a bijective finaliser)."""
    w = np.arange(1 << 20, dtype=np.uint64) * np.uint64(4093)
    for c, t, i in ((1, 0, 0), (7, 12345, 2077), (9, 260025, 511)):
        assert len(np.unique(np_mix(c, t, i, w))) == len(w)


def test_block_sums_host_equal_numpy_and_ignore_fold_order(vd):
    rng = np.random.default_rng(2)
    T, n = 300, 2078   # a ragged last block
    words = rng.integers(0, 1 << 32, (T, n), dtype=np.uint64).astype(np.uint32)
    want = np_block_sums(1, 4096, words)
    assert np.array_equal(host_block_sums(vd, 1, 4096, words), want)
    # the kernel's split: stretch wave sw folds bits t = sw mod 4 and the sums of the four waves are added; any other order gives the same sums
    t = np.repeat(np.arange(T, dtype=np.uint64) + np.uint64(4096), n).reshape(T, n)
    i = np.tile(np.arange(n, dtype=np.uint64), T).reshape(T, n)
    m = np_mix(1, t, i, words.astype(np.uint64))
    per_wave = np.zeros((4, len(want)), np.uint64)
    order = rng.permutation(T * n)
    with np.errstate(over="ignore"):
        for k in order[: T * n // 3]:          # a third of the words in a random order ...
            tt, ii = divmod(int(k), n)
            per_wave[tt % 4, tt // 64] += m[tt, ii]
        rest = np.ones(T * n, bool)
        rest[order[: T * n // 3]] = False
        for tt in range(T):                     # ... the rest row by row
            per_wave[tt % 4, tt // 64] += m[tt][rest[tt * n:(tt + 1) * n]].sum(dtype=np.uint64)
        assert np.array_equal(per_wave.sum(axis=0, dtype=np.uint64), want)


def test_any_single_changed_word_changes_its_block_sum(vd):
    rng = np.random.default_rng(3)
    T, n = 192, 47
    words = rng.integers(0, 1 << 32, (T, n), dtype=np.uint64).astype(np.uint32)
    base = host_block_sums(vd, 3, 0, words)
    for _ in range(300):
        t, i = int(rng.integers(0, T)), int(rng.integers(0, n))
        bad = words.copy()
        bad[t, i] ^= np.uint32(1 << int(rng.integers(0, 32))) if rng.random() < 0.5 else np.uint32(rng.integers(1, 1 << 32))
        got = host_block_sums(vd, 3, 0, bad)
        assert got[t // 64] != base[t // 64]
        assert np.array_equal(np.delete(got, t // 64), np.delete(base, t // 64))
    # two words swapped between positions of a block change it too (the key enters every word's mix)
    bad = words.copy()
    bad[5, 1], bad[5, 2] = words[5, 2], words[5, 1]
    if words[5, 1] != words[5, 2]:
        assert host_block_sums(vd, 3, 0, bad)[0] != base[0]


def test_first_mismatch_order_is_block_then_class_then_mixer(vd):
    k = vd.vd_key
    assert k(3, 9, 25, 10000, 3) < k(4, 1, 0, 0, 0)
    assert k(4, 1, 0, 0, 0) < k(4, 8, 0, 0, 0) < k(4, 8, 1, 0, 0) < k(4, 9, 0, 0, 0)
    key = k(12345, 9, 17, 9999, 2)
    assert (key >> 40, (key >> 36) & 15, (key >> 31) & 31, (key >> 17) & 0x3FFF, (key >> 15) & 3) == (12345, 9, 17, 9999, 2)
