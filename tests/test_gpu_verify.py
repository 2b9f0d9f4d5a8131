"""GPU: verify mode of the mixing network (include/cmix_amd.h, cmx_mixnet_set_verify). With it on, every word the compressor's
network consumes -- raw inputs, coded bits, selectors, decay words, the stretched inputs of the in-launch ring as written and as each helper read them,
and every layer-0 row segment a helper loads back -- is checked against its source. The results stay bit-identical; a perturbation of any class is
reported as an error naming it, with its block's stream bit and, for the ring and the row segments, the mixer."""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal, load_golden, synth_mixnet_inputs
import make_golden as mg

pytestmark = pytest.mark.gpu


def _dev(probs, sel, bits):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(probs)).cuda(),
            torch.from_numpy((sel & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(bits)).cuda())


def _run(net, d_probs, d_sel, d_bits, edges):
    import torch
    T = int(d_bits.numel())
    p = torch.empty(T, dtype=torch.float32, device="cuda")
    mix = torch.empty((T, 47), dtype=torch.float32, device="cuda")
    for a, b in zip(edges[:-1], edges[1:]):
        net.run(d_probs[a:b], d_sel[a:b], d_bits[a:b], p[a:b], mix[a:b])
    torch.cuda.synchronize()
    return p.cpu().numpy(), mix.cpu().numpy()


def _stage(probs, sel, bits, edges, verify):
    from cmix_amd import engine as E
    net = E.MixNet(0)
    try:
        if verify:
            net.set_verify(True)
        out = _run(net, *_dev(probs, sel, bits), edges)
        net.sync()
        return out, net.verify_report()
    finally:
        net.close()


@pytest.mark.parametrize("name", ["text_96", "binary_64"])
def test_verify_on_is_bit_identical_to_the_goldens(name):
    g = load_golden(name)
    probs = mg.unpack_probs(g)
    T = len(g["bits"])
    edges = [0, T // 3, T]
    (p, mix), rep = _stage(probs, g["sel"], g["bits"], edges, True)
    assert bits_equal(p, g["p_final"]).all() and bits_equal(mix, g["mix_out"]).all()
    assert rep["chunks"] == 2 and rep["bits"] == T and rep["mismatches"] == 0


def test_verify_on_equals_verify_off_over_several_chunks():
    """Few contexts, so layer-0 rows are written back and loaded again within a chunk and across chunks: the row-segment digests are exercised."""
    T = 3000
    probs, sel, bits = synth_mixnet_inputs(T, seed=11, n_ctx_bits=1)
    edges = [0, 700, 1500, 1501, 2300, T]
    (p0, m0), rep0 = _stage(probs, sel, bits, edges, False)
    (p1, m1), rep1 = _stage(probs, sel, bits, edges, True)
    assert bits_equal(p0, p1).all() and bits_equal(m0, m1).all()
    assert rep0["chunks"] == 0 and rep1 == {"chunks": 5, "bits": T, "mismatches": 0, "cls": None, "first_bit": None, "mixer": None, "row": None, "segment": None}


def test_verify_refuses_tolerance_and_late_use():
    from cmix_amd import engine as E
    net = E.MixNet(0)
    try:
        net.set_verify(True)
        with pytest.raises(E.CmxError, match="verify"):
            net.set_tolerance(True)
        with pytest.raises(E.CmxError, match="verify"):
            net.predict(np.full(2078, 0.5, np.float32), np.zeros(47, np.uint32))
    finally:
        net.close()
    net = E.MixNet(0)
    try:
        net.set_tolerance(True)
        with pytest.raises(E.CmxError, match="tolerance"):
            net.set_verify(True)
    finally:
        net.close()


T1, T2, BIT = 1000, 1000, 130   # a clean chunk, then the perturbed one; BIT lies in the chunk's block 2
SEG_MIXER, SEG_INDEX = 8, 700   # mixer 8 has one selector value (synth_mixnet_inputs): row 0, loaded at the start of every chunk


@pytest.mark.parametrize("cls,index,mask,want_cls,want_bit,want_mixer", [
    ("row", 1234, 0x00000001, 1, T1 + 128, None),
    ("bit", 0, 0x01, 2, T1 + 128, None),
    ("sel", 30, 0x00010000, 3, T1 + 128, None),
    ("decay", 0, 0x00000400, 4, T1 + 128, None),
    ("ring_written", 777, 0x00000001, 8, T1 + 128, 0),   # the stretch wave stores the changed value: every helper reads it, mixer 0 first
    ("segment", SEG_INDEX, 0x00400000, 9, T1, SEG_MIXER),
])
def test_each_class_of_perturbation_is_reported(cls, index, mask, want_cls, want_bit, want_mixer):
    from cmix_amd import engine as E
    probs, sel, bits = synth_mixnet_inputs(T1 + T2, seed=5, n_ctx_bits=2)
    d = _dev(probs, sel, bits)
    net = E.MixNet(0)
    try:
        net.set_verify(True)
        _run(net, *[x[:T1] for x in d], [0, T1])
        net.sync()
        assert net.verify_report()["mismatches"] == 0
        net.debug_verify_perturb(cls, SEG_MIXER * 10001 if cls == "segment" else BIT, index, mask)
        _run(net, *[x[T1:] for x in d], [0, T2])
        with pytest.raises(E.CmxError) as e:
            net.sync()
        rep = net.verify_report()
    finally:
        net.close()
    assert E.VERIFY_CLASSES[want_cls] in str(e.value) and "stream bit %d" % want_bit in str(e.value)
    assert rep["chunks"] == 2 and rep["bits"] == T1 + T2 and rep["mismatches"] >= 1
    assert rep["cls"] == want_cls and rep["first_bit"] == want_bit and rep["mixer"] == want_mixer
    if cls == "segment":
        assert rep["row"] == 0 and rep["segment"] == SEG_INDEX // 512
    # a fresh handle on the same inputs runs clean
    (_, _), rep = _stage(probs, sel, bits, [0, T1, T1 + T2], True)
    assert rep["mismatches"] == 0 and rep["bits"] == T1 + T2


def test_input_perturbation_leaves_the_results_and_the_input_unchanged():
    """An input class is perturbed between the network kernel and the verify kernel and restored behind it: the network computed on the clean word."""
    from cmix_amd import engine as E
    T = 700
    probs, sel, bits = synth_mixnet_inputs(T, seed=7)
    (p0, m0), _ = _stage(probs, sel, bits, [0, T], True)
    d = _dev(probs, sel, bits)
    net = E.MixNet(0)
    try:
        net.set_verify(True)
        net.debug_verify_perturb("row", 300, 5, 0x80000000)
        p1, m1 = _run(net, *d, [0, T])
        with pytest.raises(E.CmxError, match="layer-0 row"):
            net.sync()
    finally:
        net.close()
    assert bits_equal(p0, p1).all() and bits_equal(m0, m1).all()
    assert bits_equal(d[0].cpu().numpy(), probs).all()


def test_engine_stream_256k_shard_prefix_with_verify():
    """The first 256 KB of the bench shard through the whole engine in verify mode: the reference binary's file (size and SHA-256 of
    tests/golden/dropin_256k.npz), every chunk of the 262 150-byte TEXT-block stream verified, no mismatch."""
    from cmix_amd import synth
    from cmix_amd.pipeline import EngineStream, text_file_stream
    with np.load(os.path.join(GOLDEN, "dropin_256k.npz")) as z:
        want_sha, want_size, (n, seed) = z["sha256"].tobytes(), int(z["size"][0]), z["seed"]
    stream = text_file_stream(synth.enwik_like(int(n), int(seed)))
    assert len(stream) == 262150
    eng = EngineStream(0, stream, 4096, verify=True)
    try:
        eng.feed(len(stream))
        got = eng.finish()
        rep = eng.pipe.verify_report()
    finally:
        eng.close()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["chunks"] == (len(stream) + 4095) // 4096 and rep["bits"] == 8 * len(stream) and rep["mismatches"] == 0


def test_dropin_program_with_cmix_verify_writes_the_reference_file():
    from cmix_amd import synth
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        want_sha, want_size, (n, seed) = z["sha256"].tobytes(), int(z["size"][0]), z["seed"]
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(synth.enwik_like(int(n), int(seed)))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, CMIX_VERIFY="1"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
