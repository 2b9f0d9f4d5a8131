"""GPU: shadow mixing networks and their vote (include/cmix_amd.h: cmx_vote_*, cmx_mixnet_state_diff, cmx_pipeline_set_shadow).
The unchanged network kernel runs on two or three handles over the same inputs; the vote kernel compares every bit's 47 mixer outputs and final p
word for word and names the first differing element and the odd instance; the state diff kernel compares every state word of two handles in HBM.
A perturbation is a data change made by a test hook between chunks: no kernel stops, no wait times out."""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal, synth_mixnet_inputs

pytestmark = pytest.mark.gpu

MASK = 0x00400000


# ---- the vote kernel against its host twin ----------------------------------------------------------------------------------

def _random_instances(n, T, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)
    m = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
    return [p.copy() for _ in range(n)], [m.copy() for _ in range(n)]


def _plant(ps, ms, place, inst, T):
    if place == "first":
        ms[inst][0, 0] ^= 1
    elif place == "last":
        ps[inst][T - 1] ^= 0x80000000
    else:   # column 47 only, in the middle of the chunk
        ps[inst][T // 2] ^= 0x100


def _to_dev(ps, ms, lead):
    """device copies; lead = 1: every array starts one row into its allocation (the mixer outputs are then not 16-byte aligned)"""
    import torch
    dp, dm = [], []
    for p, m in zip(ps, ms):
        bp = torch.zeros(len(p) + lead, dtype=torch.int32, device="cuda")
        bm = torch.zeros((len(p) + lead, 47), dtype=torch.int32, device="cuda")
        bp[lead:] = torch.from_numpy(p.view(np.int32)).cuda()
        bm[lead:] = torch.from_numpy(m.view(np.int32)).cuda()
        dp.append(bp[lead:])
        dm.append(bm[lead:])
    return dp, dm


@pytest.mark.parametrize("place", ["first", "last", "col47"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T", [1, 63, 1000, 32768])
def test_vote_kernel_equals_the_host_twin(T, n, place):
    import torch
    from cmix_amd import engine as E
    from cmix_amd.vote import vote_reference
    ps, ms = _random_instances(n, T, 17 + T + n)
    inst = {"first": 1, "last": n - 1, "col47": 0}[place]
    _plant(ps, ms, place, inst, T)
    want, want_words = vote_reference(ps, ms, 5000)
    assert want[3] == 1 and want[6] == (inst if n == 3 else (1 << 64) - 1)
    lead = 1 if T == 63 else 0
    dp, dm = _to_dev(ps, ms, lead)
    sel = torch.arange(T * 47, dtype=torch.int32, device="cuda")
    bits = (torch.arange(T, device="cuda") % 2).to(torch.uint8)
    v = E.Vote(n)
    try:
        v.run(dp, dm, 5000, sel, bits)
        rep, val = v.report(), v.values()
        assert rep["raw"] == want
        assert np.array_equal(val["words"], want_words)
        t = want[4] - 5000
        assert np.array_equal(val["sel"], np.arange(t * 47, t * 47 + 47, dtype=np.uint32)) and val["bit"] == t % 2
        # a second chunk on the same handle, with another difference: the first event's fields stick, the counters advance
        ps2, ms2 = _random_instances(n, T, 99)
        ms2[0][T - 1, 46] ^= 2
        dp2, dm2 = _to_dev(ps2, ms2, lead)
        v.run(dp2, dm2, 5000 + T)
        rep2 = v.report()
        assert rep2["raw"] == [2, 2 * T, n, 2] + want[4:]
        assert np.array_equal(v.values()["words"], want_words)
        # and a clean one
        ps3, ms3 = _random_instances(n, T, 100)
        v.run(*_to_dev(ps3, ms3, lead), 5000 + 2 * T)
        assert v.report()["raw"] == [3, 3 * T, n, 2] + want[4:]
    finally:
        v.close()


def test_vote_kernel_all_agree_and_word_semantics():
    import torch
    from cmix_amd import engine as E
    T = 1000
    p = torch.zeros(T, dtype=torch.float32, device="cuda")
    m = torch.full((T, 47), float("nan"), dtype=torch.float32, device="cuda")   # one NaN pattern everywhere: equal words
    q = p.clone()
    v = E.Vote(3)
    try:
        v.run([p, p.clone(), q], [m, m.clone(), m.clone()], 0)
        assert v.report()["raw"] == [1, T, 3, 0, 0, 0, 0, 0]
        q[7] = -0.0   # == 0.0 as a float
        v.run([p, p.clone(), q], [m, m.clone(), m.clone()], T)
        assert v.report()["raw"] == [2, 2 * T, 3, 1, T + 7, 47, 2, 1]
    finally:
        v.close()


# ---- three MixNet handles on the same inputs ----------------------------------------------------------------------------------

T1 = 1000


@pytest.fixture(scope="module")
def synth():
    probs, sel, bits = synth_mixnet_inputs(2 * T1, seed=5, n_ctx_bits=2)
    return probs, sel, bits


def _dev(probs, sel, bits):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(probs)).cuda(),
            torch.from_numpy((sel & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(bits)).cuda())


class _Three:
    def __init__(self, synth):
        import torch
        from cmix_amd import engine as E
        self.torch = torch
        self.d = _dev(*synth)
        self.nets = [E.MixNet(0) for _ in range(3)]
        self.vote = E.Vote(3)
        T = 2 * T1
        self.p = [torch.empty(T, dtype=torch.float32, device="cuda") for _ in range(3)]
        self.mix = [torch.empty((T, 47), dtype=torch.float32, device="cuda") for _ in range(3)]

    def chunk(self, a, b):
        d = self.d
        for net, p, mix in zip(self.nets, self.p, self.mix):
            net.run(d[0][a:b], d[1][a:b], d[2][a:b], p[a:b], mix[a:b])
        self.vote.run([p[a:b] for p in self.p], [m[a:b] for m in self.mix], a, d[1][a:b], d[2][a:b])
        self.torch.cuda.synchronize()
        for net in self.nets:
            net.sync()

    def close(self):
        self.vote.close()
        for net in self.nets:
            net.close()


def _first_use_of_row0(sel, mixer, start):
    """the first bit >= start at which `mixer` selects its row 0 (the row of the first key it ever saw)"""
    key = sel[:, mixer] & np.uint64(0xFFFFFFFF)
    return start + int(np.flatnonzero(key[start:] == key[0])[0])


@pytest.mark.parametrize("region,mixer,layer", [("rows0", 8, 0), ("rows1", 26, 1), ("rows2", 46, 2)])
def test_three_handles_vote_names_the_perturbed_instance_and_mixer(synth, region, mixer, layer):
    probs, sel, bits = synth
    t_exp = _first_use_of_row0(sel, mixer, T1)
    if layer == 0:   # a layer-0 weight whose input at the expected bit is well away from 0.5 (its stretched value from 0)
        x = probs[t_exp]
        index = int(np.flatnonzero((np.abs(x - 0.5) > 0.2) & (x > 0) & (x < 1))[0])
    else:            # the last auxiliary input of layers 1 / 2: the stretched column 2077 (a random float in this generator)
        index = 28 if layer == 1 else 48
        assert abs(probs[t_exp, 2077] - 0.5) > 1e-3
    h = _Three(synth)
    try:
        h.chunk(0, T1)
        rep = h.vote.report()
        assert rep["raw"] == [1, T1, 3, 0, 0, 0, 0, 0]
        sd = h.nets[0].state_diff(h.nets[1])
        assert sd["words"] == 0 and sd["first"] is None and sd["layer0_mask"] == 0 and sd["layer12_mask"] == 0 and not any(sd["per_region"].values())
        h.nets[1].debug_state_xor(region, mixer, 0, index, MASK)
        sd = h.nets[0].state_diff(h.nets[1])
        assert sd["words"] == 1 and sd["per_region"][region] == 1 and sum(sd["per_region"].values()) == 1
        f = sd["first"]
        assert (f["region"], f["mixer"], f["row"], f["index"]) == (layer, mixer, 0, index) and f["b"] == f["a"] ^ MASK
        assert sd["layer0_mask"] == ((1 << 8) if layer == 0 else 0)            # the other 25 layer-0 mixers are untouched
        assert sd["layer12_mask"] == (0 if layer == 0 else 1 << (mixer - 26))
        assert h.nets[0].state_diff(h.nets[2])["words"] == 0
        h.chunk(T1, 2 * T1)
        rep, val = h.vote.report(), h.vote.values()
        assert rep["chunks"] == 2 and rep["bits"] == 2 * T1 and rep["events"] == 1
        assert (rep["first_bit"], rep["column"], rep["odd"]) == (t_exp, mixer, 1)
        w = val["words"]
        assert w[0, mixer] == w[2, mixer] != w[1, mixer] and np.array_equal(w[0, :mixer], w[1, :mixer])
        assert np.array_equal(val["sel"], (sel[t_exp] & np.uint64(0xFFFFFFFF)).astype(np.uint32)) and val["bit"] == bits[t_exp]
        assert bits_equal(h.p[0].cpu().numpy(), h.p[2].cpu().numpy()).all()
        # a chunk later the masks still name the origin: a mixer's inputs are the layer's inputs and the outputs of the mixers BEFORE it in
        # its layer, and its update depends on its own output alone, so everything before the origin is still identical
        sd = h.nets[0].state_diff(h.nets[1])
        assert sd["words"] >= 1
        if layer == 0:
            assert sd["layer0_mask"] & ((1 << 9) - 1) == 1 << 8
        else:
            assert sd["layer0_mask"] == 0 and sd["layer12_mask"] & ((1 << (mixer - 25)) - 1) == 1 << (mixer - 26)
    finally:
        h.close()


def test_state_diff_sees_one_sse_word(synth):
    h = _Three(synth)
    try:
        h.chunk(0, T1)
        h.nets[1].debug_state_xor("s6", None, None, 123457, 0x00010000)
        sd = h.nets[0].state_diff(h.nets[1])
        assert sd["words"] == 1 and sd["per_region"]["s6"] == 1 and sum(sd["per_region"].values()) == 1
        f = sd["first"]
        assert (f["region"], f["mixer"], f["row"], f["index"]) == (6, None, None, 123457) and f["b"] == f["a"] ^ 0x00010000
        assert sd["layer0_mask"] == 0 and sd["layer12_mask"] == 0
    finally:
        h.close()


# ---- the bare pipeline: no fxcm / paq8 stage, the caller's columns ---------------------------------------------------------------

N_CHUNK = 256


def _bare(shadow, nchunks, before=None):
    """a Pipeline over nchunks chunks of 256 synthetic text bytes; columns 3..2024 are the caller's (a seeded grid)"""
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    data = np.frombuffer(S.enwik_like(4 * N_CHUNK, 21), np.uint8)
    rng = np.random.default_rng(8)
    cols = (rng.integers(1, 4095, (8 * 4 * N_CHUNK, 2078)).astype(np.float32) * np.float32(1.0 / 4095)).astype(np.float32)
    layer0 = torch.from_numpy(cols).cuda()
    p = torch.full((8 * 4 * N_CHUNK,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)
    if before:
        before(pipe)
    if shadow:
        pipe.set_shadow(shadow)

    def submit(i):
        a, b = i * N_CHUNK, (i + 1) * N_CHUNK
        pipe.submit(data[a:b].tobytes(), layer0[8 * a:8 * b], p[8 * a:8 * b])
    for i in range(nchunks):
        submit(i)
        pipe.wait(i)
    return pipe, p, submit


def test_pipeline_shadow_clean_run_then_the_primary_is_perturbed():
    from cmix_amd import engine as E
    q0 = E.hw_queues()
    pipe, p_off, _ = _bare(0, 3)
    try:
        pipe.sync()
        q1 = E.hw_queues()
        assert pipe.shadow_report()["raw"] == [0] * 8
        want = p_off.cpu().numpy()[:8 * 3 * N_CHUNK]
    finally:
        pipe.close()
    assert E.hw_queues() == q0
    pipe, p_on, submit = _bare(2, 3)
    try:
        assert E.hw_queues() == q1 + 2
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], want).all()
        rep = pipe.shadow_report()
        assert rep["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.shadow_state_diff(0, 1)["words"] == 0 and pipe.shadow_state_diff(1, 2)["words"] == 0
        with pytest.raises(E.CmxError, match="before the first chunk"):
            pipe.set_shadow(1)
        # mixer 26 is keyed by the constant zero context: its row 0 is used by every bit; weight 28 meets the LSTM's stretched prediction
        pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, MASK)
        assert pipe.shadow_state_diff(0, 1)["words"] == 1
        submit(3)
        with pytest.raises(E.CmxError) as e:
            pipe.wait(3)
        msg = str(e.value)
        assert "chunk 3" in msg and "stream bit %d" % (8 * 3 * N_CHUNK) in msg and "mixer 26" in msg and "instance 0" in msg
        rep = pipe.shadow_report()
        assert rep["events"] == 1 and (rep["first_bit"], rep["column"], rep["odd"]) == (8 * 3 * N_CHUNK, 26, 0)
        with pytest.raises(E.CmxError, match="void"):   # the handle is voided ...
            submit(0)
        sd = pipe.shadow_state_diff(0, 1)               # ... and can still be diagnosed: the origin lies in layer 1 of instance 0
        assert sd["words"] >= 1 and sd["layer0_mask"] == 0 and sd["layer12_mask"] & 1
        assert pipe.shadow_state_diff(1, 2)["words"] == 0
    finally:
        pipe.close()
    assert E.hw_queues() == q0


def test_pipeline_one_shadow_has_no_majority_and_refusals():
    from cmix_amd import engine as E
    q0 = E.hw_queues()

    def refusals(pipe):
        with pytest.raises(E.CmxError, match="0, 1 or 2"):
            pipe.set_shadow(3)
        pipe.set_tolerance(True)
        with pytest.raises(E.CmxError, match="tolerance"):
            pipe.set_shadow(1)
        pipe.set_tolerance(False)
        pipe.set_shadow(1)
        with pytest.raises(E.CmxError, match="shadow"):
            pipe.set_tolerance(True)
        q = E.hw_queues()
        pipe.set_shadow(0)          # dropped again: its queue goes back
        assert E.hw_queues() == q - 1
    pipe, _, submit = _bare(1, 1, before=refusals)
    try:
        assert pipe.shadow_report()["raw"] == [1, 8 * N_CHUNK, 2, 0, 0, 0, 0, 0]
        pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, MASK)
        submit(1)
        with pytest.raises(E.CmxError, match="no majority between 2 instances") as e:
            pipe.wait(1)
        assert "mixer 26" in str(e.value) and "chunk 1" in str(e.value)
        rep = pipe.shadow_report()
        assert rep["events"] == 1 and rep["odd"] is None and rep["column"] == 26 and rep["first_bit"] == 8 * N_CHUNK
        with pytest.raises(E.CmxError, match="no such instance"):
            pipe.shadow_state_diff(0, 2)
    finally:
        pipe.close()
    assert E.hw_queues() == q0


# ---- the whole engine --------------------------------------------------------------------------------------------------------

def _golden_64k():
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        return z["sha256"].tobytes(), int(z["size"][0]), int(z["seed"][0]), int(z["seed"][1])


def test_engine_stream_64k_with_two_shadows_writes_the_reference_file():
    from cmix_amd import synth as S
    from cmix_amd.pipeline import EngineStream, text_file_stream
    want_sha, want_size, n, seed = _golden_64k()
    stream = text_file_stream(S.enwik_like(n, seed))
    eng = EngineStream(0, stream, 4096, shadow=2)
    try:
        eng.feed(len(stream))
        got = eng.finish()
        rep = eng.pipe.shadow_report()
    finally:
        eng.close()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["raw"] == [(len(stream) + 4095) // 4096, 8 * len(stream), 3, 0, 0, 0, 0, 0]


def test_dropin_program_with_cmix_shadow_writes_the_reference_file():
    from cmix_amd import synth as S
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    want_sha, want_size, n, seed = _golden_64k()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(S.enwik_like(n, seed))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, CMIX_SHADOW="2"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
