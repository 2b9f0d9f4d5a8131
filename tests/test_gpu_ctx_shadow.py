"""GPU: shadow context stages and their vote (include/cmix_amd.h: cmx_ctxvote_*, cmx_ctxmodels_create_compact, cmx_ctxmodels_state_diff,
cmx_pipeline_set_ctx_shadow). The unchanged context-stage kernel runs on two or three handles over the same bytes; the vote kernel
compares every bit's 54 model outputs and 47 selectors word for word and names the first differing element and the odd instance; the state diff
kernel compares every state word of two handles in HBM. A perturbation is a data change made by a test hook between chunks: no kernel stops, no
wait times out."""
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1


# ---- the vote kernel against its host twin ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base(T, seed):
    """random words: the full-stride matrix of instance 0 [T, 2078], the selectors [T, 47], and what a compact instance holds beside its 54 columns"""
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 1 << 32, (T, 2078), dtype=np.uint64).astype(np.uint32)
    sel = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
    pad = rng.integers(0, 1 << 32, (T, 10), dtype=np.uint64).astype(np.uint32)
    return full, sel, pad


def _instances(n, T, seed):
    """n instances that agree: instance 0 full-stride, the others compact (their columns 54..63 hold other words, which the vote must not read)"""
    from cmix_amd.ctxvote import LAYER0_COLS
    full, sel, pad = _base(T, seed)
    mats = [full.copy()]
    for i in range(1, n):
        m = np.empty((T, 64), np.uint32)
        m[:, :54] = full[:, LAYER0_COLS]
        m[:, 54:] = pad + np.uint32(i)
        mats.append(m)
    return mats, [sel.copy() for _ in range(n)]


def _plant(mats, sels, inst, t, c, mask):
    from cmix_amd.ctxvote import LAYER0_COLS
    if c >= 54:
        sels[inst][t, c - 54] ^= np.uint32(mask)
    else:
        mats[inst][t, c if inst else LAYER0_COLS[c]] ^= np.uint32(mask)


def _outs(mats):
    from cmix_amd.ctxvote import model_outputs
    return [model_outputs(m, i > 0) for i, m in enumerate(mats)]


def _to_dev(mats, sels, lead):
    """device copies; lead = 1: every array starts one row into its allocation (a selector row is 188 bytes, a full row 8312: neither array is then 16-byte aligned)"""
    import torch
    dm, ds = [], []
    for m, s in zip(mats, sels):
        bm = torch.zeros((m.shape[0] + lead, m.shape[1]), dtype=torch.int32, device="cuda")
        bs = torch.zeros((s.shape[0] + lead, 47), dtype=torch.int32, device="cuda")
        bm[lead:] = torch.from_numpy(m.view(np.int32)).cuda()
        bs[lead:] = torch.from_numpy(s.view(np.int32)).cuda()
        dm.append(bm[lead:])
        ds.append(bs[lead:])
    return dm, ds


# T: a single row, one below and one above a wave's worth of rows, no grid-stride step yet, a grid-stride tail (2500 rows on 2048 waves), more rows than the grid
@pytest.mark.parametrize("place", ["first", "last", "c53", "c54"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T", [1, 63, 65, 1000, 2500, 4096])
def test_vote_kernel_equals_the_host_twin(T, n, place):
    import torch
    from cmix_amd import engine as E
    from cmix_amd.ctxvote import chunk_result, ctx_vote_reference
    mats, sels = _instances(n, T, 17 + T)
    inst, t, c = {"first": (1, 0, 0), "last": (n - 1, T - 1, 100), "c53": (0, T // 2, 53), "c54": (0, T // 2, 54)}[place]
    _plant(mats, sels, inst, t, c, 0x80000000 if place == "last" else 1)
    want, want_words = ctx_vote_reference(_outs(mats), sels, 5000)
    assert want == [1, T, n, 1, 5000 + t, c, inst if n == 3 else NONE, 1]
    lead = 1 if T == 63 else 0
    compact = [False] + [True] * (n - 1)
    bits = (torch.arange(T, device="cuda") % 2).to(torch.uint8)
    v = E.CtxVote(n)
    try:
        dm, ds = _to_dev(mats, sels, lead)
        v.run(dm, compact, ds, 5000, bits)
        rep, val = v.report(), v.values()
        assert rep["raw"] == want
        assert np.array_equal(val["words"], want_words) and val["bit"] == t % 2
        assert v.last()["raw"] == chunk_result(_outs(mats), sels, 5000)
        # a second chunk on the same handle, with another difference: the first event's fields stick, the counters advance
        mats2, sels2 = _instances(n, T, 99 + T)
        _plant(mats2, sels2, 0, T - 1, 20, 2)
        dm2, ds2 = _to_dev(mats2, sels2, lead)
        v.run(dm2, compact, ds2, 5000 + T)
        assert v.report()["raw"] == [2, 2 * T, n, 2] + want[4:]
        assert np.array_equal(v.values()["words"], want_words)
        assert v.last()["raw"] == chunk_result(_outs(mats2), sels2, 5000 + T) == [1, 5000 + 2 * T - 1, 20, 0 if n == 3 else NONE]
        # and a clean one
        mats3, sels3 = _instances(n, T, 100 + T)
        dm3, ds3 = _to_dev(mats3, sels3, lead)
        v.run(dm3, compact, ds3, 5000 + 2 * T)
        assert v.report()["raw"] == [3, 3 * T, n, 2] + want[4:]
        assert v.last()["raw"] == [0, 0, 0, 0]
    finally:
        v.close()


def test_vote_kernel_all_agree_and_word_semantics():
    import torch
    from cmix_amd import engine as E
    T = 1000
    nan = torch.full((T, 2078), float("nan"), dtype=torch.float32, device="cuda")   # one NaN pattern everywhere: equal words
    cn = torch.full((T, 64), float("nan"), dtype=torch.float32, device="cuda")
    sel = torch.zeros((T, 47), dtype=torch.float32, device="cuda")
    q = sel.clone()
    v = E.CtxVote(3)
    try:
        v.run([nan, cn, cn.clone()], [False, True, True], [sel, sel.clone(), q], 0)
        assert v.report()["raw"] == [1, T, 3, 0, 0, 0, 0, 0]
        q[7, 3] = -0.0   # == 0.0 as a float
        v.run([nan, cn, cn.clone()], [False, True, True], [sel, sel.clone(), q], T)
        assert v.report()["raw"] == [2, 2 * T, 3, 1, T + 7, 54 + 3, 2, 1]
        with pytest.raises(E.CmxError, match="pstride"):   # a full-form instance needs a full row
            v.run([cn, cn, cn], [False, True, True], [sel, sel, sel], 0)
    finally:
        v.close()


# ---- three CtxModels handles on the same bytes ----------------------------------------------------------------------------------

N_CHUNK = 256
IPRED_SLOT = 18     # the Indirect model of the order-1..6 word context (lane 20, layer-0 column 2042): in 512 bytes of text nearly every byte's
IPRED_STATE = 0     # context is new, its state byte is 0 ("never seen"), so entry [18][0] is read -- and learnt -- at bit 0 of nearly every byte
IPRED_MASK = 0x00400000   # the top mantissa bit: another probability, never a NaN


def test_three_handles_agree_then_one_ipred_word_is_perturbed():
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    from cmix_amd.ctxvote import ctx_vote_reference, model_outputs
    data = torch.from_numpy(np.frombuffer(S.enwik_like(2 * N_CHUNK, 21), np.uint8).copy()).cuda()
    vocab = np.ones(256, np.uint8)
    hs = [E.CtxModels(vocab, 0), E.CtxModels(vocab, 0, compact=True), E.CtxModels(vocab, 0, compact=True)]
    compact = [False, True, True]
    vote = E.CtxVote(3)
    try:
        def chunk(i):
            outs = [h.run(data[i * N_CHUNK:(i + 1) * N_CHUNK]) for h in hs]
            vote.run([o[0] for o in outs], compact, [o[1] for o in outs], 8 * i * N_CHUNK)
            torch.cuda.synchronize()
            for h in hs:
                h.sync()
            return [model_outputs(o[0].cpu().numpy(), c) for o, c in zip(outs, compact)], [o[1].cpu().numpy().view(np.uint32) for o in outs]
        outs, sels = chunk(0)
        assert outs[1].shape == (8 * N_CHUNK, 54)
        for i in (1, 2):   # the compact form holds the full handle's 54 columns and 47 selectors word for word
            assert np.array_equal(outs[i], outs[0]) and np.array_equal(sels[i], sels[0])
        assert vote.report()["raw"] == [1, 8 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        for a, b in ((0, 1), (1, 2), (2, 0)):   # a compact and a full handle differ in configuration, never in state
            sd = hs[a].state_diff(hs[b])
            assert sd["words"] == 0 and sd["first"] is None and sd["lane_mask"] == 0 and not any(sd["per_region"].values())
        with pytest.raises(E.CmxError, match="same handle"):
            hs[0].state_diff(hs[0])
        lay = E.ctx_layout()
        word = lay["ipred"] + IPRED_SLOT * 256 + IPRED_STATE
        assert lay["regs"] == 0 and lay["br_probs"] < lay["ipred"] < lay["mpred"] < lay["words"] and lay["mpred"] - lay["ipred"] == 31 * 256
        hs[2].debug_state_xor("persist", None, word, IPRED_MASK)
        sd = hs[2].state_diff(hs[0])
        assert sd["words"] == 1 and sd["per_region"]["persist"] == 1 and sum(sd["per_region"].values()) == 1 and sd["lane_mask"] == 0
        f = sd["first"]
        assert (f["region"], f["lane"], f["index"]) == (0, None, word) and f["a"] == f["b"] ^ IPRED_MASK
        assert hs[0].state_diff(hs[1])["words"] == 0
        outs, sels = chunk(1)
        want, want_words = ctx_vote_reference(outs, sels, 8 * N_CHUNK)
        assert want[3] == 1, "the perturbed ipred entry was not read in chunk 2: the outputs are still equal"
        assert want[6] == 2 and np.array_equal(outs[0], outs[1])
        rep = vote.report()
        assert rep["raw"] == [2, 2 * 8 * N_CHUNK, 3, 1] + want[4:]
        assert np.array_equal(vote.values()["words"], want_words)
        assert hs[0].state_diff(hs[1])["words"] == 0 and hs[2].state_diff(hs[0])["per_region"]["persist"] >= 1
    finally:
        vote.close()
        for h in hs:
            h.close()


# ---- the bare pipeline: no fxcm / paq8 stage, the caller's columns ---------------------------------------------------------------

def _bare(ctx_shadow, nchunks, before=None, shadow=0, verify=False, pretrain=None):
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
    try:
        if before:
            before(pipe)
        if verify:
            pipe.set_verify(True)
        if shadow:
            pipe.set_shadow(shadow)
        if ctx_shadow:
            pipe.set_ctx_shadow(ctx_shadow)
        if pretrain:
            pipe.pretrain(pretrain)

        def submit(i):
            a, b = i * N_CHUNK, (i + 1) * N_CHUNK
            pipe.submit(data[a:b].tobytes(), layer0[8 * a:8 * b], p[8 * a:8 * b])
        for i in range(nchunks):
            submit(i)
            pipe.wait(i)
    except Exception:
        pipe.close()
        raise
    return pipe, p, submit, layer0


@pytest.fixture(scope="module")
def clean():
    """the run without shadows, once: p of four chunks, the Bracket model's column 0 at the fourth chunk's first bit, the queue counts"""
    from cmix_amd import engine as E
    q0 = E.hw_queues()
    pipe, p, _, layer0 = _bare(0, 4)
    try:
        pipe.sync()
        q1 = E.hw_queues()
        assert pipe.ctx_shadow_report()["raw"] == [0] * 8
        out = {"p": p.cpu().numpy().copy(), "col0": float(layer0[8 * 3 * N_CHUNK, 0].item()), "q0": q0, "q1": q1}
    finally:
        pipe.close()
    assert E.hw_queues() == q0
    return out


def _inject_br_probs(pipe):
    from cmix_amd import engine as E
    # br_probs[0] of the stream's own stage: any value in [0, 1) becomes one >= 2, which changes the denominator of bit 0 of the next chunk's first byte
    pipe.debug_ctx_shadow_xor(0, "persist", None, E.ctx_layout()["br_probs"], 0x40000000)


def test_pipeline_ctx_shadow_clean_run_then_the_primary_is_perturbed(clean):
    from cmix_amd import engine as E
    assert clean["col0"] != 0.0   # (a zero numerator would hide the changed denominator)
    pipe, p_on, submit, _ = _bare(2, 3)
    try:
        assert E.hw_queues() == clean["q1"] + 2
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.ctx_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.ctx_shadow_state_diff(0, 1)["words"] == 0 and pipe.ctx_shadow_state_diff(1, 2)["words"] == 0
        with pytest.raises(E.CmxError, match="before the first chunk"):
            pipe.set_ctx_shadow(1)
        _inject_br_probs(pipe)
        sd = pipe.ctx_shadow_state_diff(0, 1)
        assert sd["words"] == 1 and sd["first"]["region"] == 0 and sd["first"]["index"] == E.ctx_layout()["br_probs"]
        submit(3)
        with pytest.raises(E.CmxError) as e:
            pipe.wait(3)
        msg = str(e.value)
        assert "chunk 3" in msg and "stream bit %d" % (8 * 3 * N_CHUNK) in msg and "layer-0 column 0" in msg and "instance 0" in msg
        rep = pipe.ctx_shadow_report()
        assert rep["events"] == 1 and (rep["first_bit"], rep["column"], rep["odd"]) == (8 * 3 * N_CHUNK, 0, 0)
        w = pipe.ctx_shadow_values()["words"]
        assert w.shape == (3, 101) and w[1, 0] == w[2, 0] != w[0, 0] and np.array_equal(w[1], w[2])
        with pytest.raises(E.CmxError, match="void"):   # the handle is voided ...
            submit(0)
        assert pipe.ctx_shadow_state_diff(1, 2)["words"] == 0   # ... and can still be diagnosed
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]


def test_pipeline_one_ctx_shadow_has_no_majority_and_refusals(clean):
    from cmix_amd import engine as E

    def refusals(pipe):
        with pytest.raises(E.CmxError, match="0, 1 or 2"):
            pipe.set_ctx_shadow(3)
        pipe.set_ctx_shadow(2)
        q = E.hw_queues()
        pipe.set_ctx_shadow(0)          # dropped again: the queues go back
        assert E.hw_queues() == q - 2
    pipe, _, submit, _ = _bare(1, 1, before=refusals)
    try:
        assert E.hw_queues() == clean["q1"] + 1
        assert pipe.ctx_shadow_report()["raw"] == [1, 8 * N_CHUNK, 2, 0, 0, 0, 0, 0]
        _inject_br_probs(pipe)
        submit(1)
        with pytest.raises(E.CmxError, match="no majority between 2 instances") as e:
            pipe.wait(1)
        assert "layer-0 column 0" in str(e.value) and "chunk 1" in str(e.value)
        rep = pipe.ctx_shadow_report()
        assert rep["events"] == 1 and rep["odd"] is None and rep["column"] == 0 and rep["first_bit"] == 8 * N_CHUNK
        with pytest.raises(E.CmxError, match="no such instance"):
            pipe.ctx_shadow_state_diff(0, 2)
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]


def test_pipeline_pretrain_trains_every_instance():
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    pipe, _, _, _ = _bare(2, 2, pretrain=S.enwik_like(300, 4))
    try:
        pipe.sync()
        assert pipe.ctx_shadow_report()["raw"] == [2, 8 * 2 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.ctx_shadow_state_diff(0, 2)["words"] == 0
    finally:
        pipe.close()
    # a shadow set after the dictionary would start untrained: refused
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)
    try:
        pipe.pretrain(S.enwik_like(300, 4))
        with pytest.raises(E.CmxError, match="pretrain"):
            pipe.set_ctx_shadow(1)
    finally:
        pipe.close()


def test_pipeline_ctx_shadow_beside_the_network_vote_and_verify_mode(clean):
    pipe, p_on, _, _ = _bare(2, 3, shadow=2, verify=True)
    try:
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.ctx_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        ver = pipe.verify_report()
        assert ver["chunks"] == 3 and ver["mismatches"] == 0
    finally:
        pipe.close()


# ---- the whole engine --------------------------------------------------------------------------------------------------------

def _golden_64k():
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        return z["sha256"].tobytes(), int(z["size"][0]), int(z["seed"][0]), int(z["seed"][1])


def test_engine_stream_64k_with_two_ctx_shadows_writes_the_reference_file():
    from cmix_amd import synth as S
    from cmix_amd.pipeline import EngineStream, text_file_stream
    want_sha, want_size, n, seed = _golden_64k()
    stream = text_file_stream(S.enwik_like(n, seed))
    eng = EngineStream(0, stream, 4096, ctx_shadow=2)
    try:
        eng.feed(len(stream))
        got = eng.finish()
        rep = eng.pipe.ctx_shadow_report()
    finally:
        eng.close()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["raw"] == [(len(stream) + 4095) // 4096, 8 * len(stream), 3, 0, 0, 0, 0, 0]


def test_dropin_program_with_cmix_ctx_shadow_writes_the_reference_file():
    from cmix_amd import synth as S
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    want_sha, want_size, n, seed = _golden_64k()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(S.enwik_like(n, seed))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, CMIX_CTX_SHADOW="2"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
