"""GPU: shadow LSTM stages and their vote (include/cmix_amd.h: cmx_lstmvote_*, cmx_lstm_state_diff, cmx_pipeline_set_lstm_shadow).
The unchanged LSTM kernels run on two or three handles over the same bytes and PPMd distributions; the vote kernel compares every byte's 256-way
distribution, eight bit predictions and eight ex words word for word and names the first differing element and the odd instance; the state diff kernel
compares every state word of two handles in HBM. A perturbation is a data change made by a test hook between chunks: no kernel is altered, no wait
times out, no fault is provoked."""
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal, load_golden
import make_golden as mg
import make_lstm_vocab as mk

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
CHUNKS = [1, 2, 99, 100, 101, 199, 205]   # two BPTT rounds; a chunk that ends on, before and after an epoch boundary
GAMMA_MASK = 0x00400000                   # on gb[0][0] word 0 = gamma of layer 0's forget gate, cell 0 (1.0 at the start -> 1.5): the top mantissa bit, so finite; read at the next forward step


# ---- the vote kernel against its host twin ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base(N, seed):
    """random words: a distribution [N, 256], bit predictions [N, 8], ex [N, 8]"""
    rng = np.random.default_rng(seed)
    mk_ = lambda w: rng.integers(0, 1 << 32, (N, w), dtype=np.uint64).astype(np.uint32)
    return mk_(256), mk_(8), mk_(8)


def _instances(n, N, seed):
    d, p, x = _base(N, seed)
    return [d.copy() for _ in range(n)], [p.copy() for _ in range(n)], [x.copy() for _ in range(n)]


def _plant(ds, ps, xs, inst, b, c, mask):
    a, k = (ds[inst], c) if c < 256 else (ps[inst], c - 256) if c < 264 else (xs[inst], c - 264)
    a[b, k] ^= np.uint32(mask)


def _to_dev(ds, ps, xs, lead):
    """device copies; instance 0's bit predictions lie in column 2077 of a [8 N, 2078] matrix of other words; lead = 1: every array starts one row
    into its allocation (a layer-0 row is 8312 bytes: that matrix is then not 16-byte aligned)"""
    import torch
    N = ds[0].shape[0]

    def up(a, rows, width):
        buf = torch.zeros((rows + lead, width), dtype=torch.int32, device="cuda")
        buf[lead:] = torch.from_numpy(a.view(np.int32).reshape(rows, width)).cuda()
        return buf[lead:]
    dd = [up(d, N, 256) for d in ds]
    dx = [up(x, N, 8) for x in xs]
    l0 = torch.randint(-(1 << 31), (1 << 31) - 1, (8 * N + lead, 2078), dtype=torch.int32, device="cuda")[lead:]
    l0[:, 2077] = torch.from_numpy(ps[0].view(np.int32).reshape(-1)).cuda()
    dp = [l0] + [up(p, N, 8) for p in ps[1:]]
    return dd, dp, dx


# N: a single row, one below and one above a wave's worth of rows, no grid-stride step yet, a grid-stride tail (2500 rows on 2048 waves), a full chunk
@pytest.mark.parametrize("place", ["first", "last", "c255", "c256", "c263", "c264"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("N", [1, 63, 65, 1000, 2500, 4096])
def test_vote_kernel_equals_the_host_twin(N, n, place):
    import torch
    from cmix_amd import engine as E
    from cmix_amd.lstmvote import chunk_result, lstm_vote_reference
    ds, ps, xs = _instances(n, N, 17 + N)
    inst, b, c = {"first": (1, 0, 0), "last": (n - 1, N - 1, 271), "c255": (0, N // 2, 255), "c256": (0, N // 2, 256), "c263": (n - 1, N // 2, 263),
                  "c264": (0, N // 2, 264)}[place]
    _plant(ds, ps, xs, inst, b, c, 0x80000000 if place == "last" else 1)
    want, want_words = lstm_vote_reference(ds, ps, xs, 5000)
    assert want == [1, N, n, 1, 5000 + b, c, inst if n == 3 else NONE, 1]
    lead = 1 if N == 63 else 0
    data = (torch.arange(N, device="cuda") % 251).to(torch.uint8)
    v = E.LstmVote(n)
    try:
        dd, dp, dx = _to_dev(ds, ps, xs, lead)
        assert dp[0].shape == (8 * N, 2078)
        v.run(dd, dp, dx, 5000, data)
        rep, val = v.report(), v.values()
        assert rep["raw"] == want
        assert np.array_equal(val["words"], want_words) and val["byte"] == b % 251
        assert v.last()["raw"] == chunk_result(ds, ps, xs, 5000)
        # a second chunk on the same handle, with another difference: the first event's fields stick, the counters advance
        ds2, ps2, xs2 = _instances(n, N, 99 + N)
        _plant(ds2, ps2, xs2, 0, N - 1, 20, 2)
        v.run(*_to_dev(ds2, ps2, xs2, lead), 5000 + N)
        assert v.report()["raw"] == [2, 2 * N, n, 2] + want[4:]
        assert np.array_equal(v.values()["words"], want_words)
        assert v.last()["raw"] == chunk_result(ds2, ps2, xs2, 5000 + N) == [1, 5000 + 2 * N - 1, 20, 0 if n == 3 else NONE]
        # and a clean one
        v.run(*_to_dev(*_instances(n, N, 100 + N), lead), 5000 + 2 * N)
        assert v.report()["raw"] == [3, 3 * N, n, 2] + want[4:]
        assert v.last()["raw"] == [0, 0, 0, 0]
    finally:
        v.close()


def test_vote_kernel_all_agree_and_word_semantics():
    import torch
    from cmix_amd import engine as E
    N = 1000
    nan = torch.full((N, 256), float("nan"), dtype=torch.float32, device="cuda")   # one NaN pattern everywhere: equal words
    p = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    x = torch.zeros((N, 8), dtype=torch.int32, device="cuda")
    q = p.clone()
    v = E.LstmVote(3)
    try:
        v.run([nan, nan.clone(), nan.clone()], [p, p.clone(), q], [x, x, x], 0)
        assert v.report()["raw"] == [1, N, 3, 0, 0, 0, 0, 0]
        q[7, 3] = -0.0   # == 0.0 as a float
        v.run([nan, nan.clone(), nan.clone()], [p, p.clone(), q], [x, x, x], N)
        assert v.report()["raw"] == [2, 2 * N, 3, 1, N + 7, 256 + 3, 2, 1]
    finally:
        v.close()


# ---- three Lstm handles on one stream ----------------------------------------------------------------------------------------

def _three_handles(vocab, ppmd, stream, nbytes, check):
    """three Lstm handles over stream[:nbytes] in chunks cut at CHUNKS, instance 0 writing its bit predictions in place into layer-0 rows; the vote
    after every chunk. check(i, dist, bitp, ex, a, b) for every instance's chunk. -> (handles, vote, device inputs); the caller closes them."""
    import torch
    from cmix_amd import engine as E
    hs = [E.Lstm(vocab, 0) for _ in range(3)]
    vote = E.LstmVote(3)
    try:
        d_in = torch.from_numpy(np.ascontiguousarray(ppmd, np.float32)).cuda()
        d_b = torch.from_numpy(np.ascontiguousarray(stream, np.uint8)).cuda()
        edges = sorted(set([0, nbytes] + CHUNKS))
        for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            outs = _run_chunk(hs, vote, d_in, d_b, a, b)
            for i, (dist, bitp, ex) in enumerate(outs):
                check(i, dist, bitp, ex, a, b)
            assert vote.last()["raw"] == [0, 0, 0, 0], "the instances disagree in chunk %d (bytes %d..%d)" % (k, a, b)
            assert vote.report()["raw"] == [k + 1, b, 3, 0, 0, 0, 0, 0]
        for h in hs:
            assert E.lib().cmx_lstm_failed(h.h) == 0
        for a, b in ((0, 1), (1, 2), (2, 0)):
            sd = hs[a].state_diff(hs[b])
            assert sd["words"] == 0 and sd["first"] is None and not any(sd["per_region"].values()), (a, b, sd)
        with pytest.raises(E.CmxError, match="same handle"):
            hs[0].state_diff(hs[0])
    except Exception:
        vote.close()
        for h in hs:
            h.close()
        raise
    return hs, vote, d_in, d_b


def _run_chunk(hs, vote, d_in, d_b, a, b):
    """bytes a..b on every handle, then the vote; -> per instance (dist [n, 256], bitp [n, 8], ex [n, 8]) read back"""
    import torch
    layer0 = torch.zeros((8 * (b - a), 2078), dtype=torch.float32, device="cuda")
    res = [hs[0].run(d_in[a:b], d_b[a:b], layer0=layer0)] + [h.run(d_in[a:b], d_b[a:b]) for h in hs[1:]]
    vote.run([r[0] for r in res], [layer0] + [r[1] for r in res[1:]], [r[2] for r in res], a, d_b[a:b])
    torch.cuda.synchronize()
    return [(r[0].cpu().numpy(), (layer0[:, 2077].reshape(-1, 8) if i == 0 else r[1]).cpu().numpy(), r[2].cpu().numpy()) for i, r in enumerate(res)]


def test_three_handles_agree_then_one_gamma_word_is_perturbed():
    from cmix_amd import engine as E
    from cmix_amd.lstmvote import lstm_vote_reference
    g = load_golden("text_2k_nofull")
    N, M = 230, 30
    want_bp = mg.unpack_probs(g)[:8 * (N + M), 2077].reshape(N + M, 8) if "probs_q" in g else None

    def check(i, dist, bitp, ex, a, b):
        bad = np.nonzero(~bits_equal(dist, g["lstm_probs"][1 + a:1 + b]).all(axis=1))[0]
        assert len(bad) == 0, f"instance {i}: LSTM distribution differs from the golden trace first after byte {a + bad[0]}"
        if want_bp is not None:
            assert bits_equal(bitp, want_bp[a:b]).all(), f"instance {i}: bit predictions of bytes {a}..{b}"
    hs, vote, d_in, d_b = _three_handles(g["vocab"], g["ppmd_probs"][1:N + M + 1], g["stream"][:N + M], N, check)
    try:
        nchunks = vote.report()["chunks"]
        lay = E.lstm_layout(hs[0])
        gb00 = [a for a in lay if a["name"] == "gb[0][0]"][0]
        assert gb00 == {"name": "gb[0][0]", "region": "gb", "offset": 0, "words": 8 * 200}
        with pytest.raises(E.CmxError, match="refused"):   # input_history: a word the kernels address memory with
            hs[2].debug_state_xor("indices", 0, 1)
        hs[2].debug_state_xor("gb", 0, GAMMA_MASK)
        sd = hs[2].state_diff(hs[0])
        assert sd["words"] == 1 and sd["per_region"]["gb"] == 1 and sum(sd["per_region"].values()) == 1
        f = sd["first"]
        assert (f["region"], f["index"]) == (4, 0) and f["a"] == f["b"] ^ GAMMA_MASK
        assert hs[0].state_diff(hs[1])["words"] == 0
        outs = _run_chunk(hs, vote, d_in, d_b, N, N + M)
        want, want_words = lstm_vote_reference([o[0] for o in outs], [o[1] for o in outs], [o[2] for o in outs], N)
        assert want[3] == 1, "the perturbed gamma was not read in the 30 bytes: the outputs are still equal"
        assert want[6] == 2 and want[4] == N   # the odd instance; the chunk's first byte (the word is read at the next forward step)
        assert vote.report()["raw"] == [nchunks + 1, N + M, 3, 1] + want[4:]
        assert np.array_equal(vote.values()["words"], want_words)
        for i in (0, 1):   # the majority still follows the reference
            check(i, outs[i][0], outs[i][1], outs[i][2], N, N + M)
        assert hs[0].state_diff(hs[1])["words"] == 0 and hs[2].state_diff(hs[0])["words"] >= 1
    finally:
        vote.close()
        for h in hs:
            h.close()


@pytest.fixture(scope="module")
def sweep():
    return mk.load_sweep()


# the smallest vocabulary; one whose layer inputs (201 + V and 401 + V columns) are no multiple of four: the tail of the transposed weights' layout
@pytest.mark.parametrize("V", [1, 62])
def test_three_handles_agree_at_other_vocabulary_sizes(sweep, V):
    from cmix_amd import engine as E
    c = sweep[V]
    assert V == min(sweep) or ((201 + V) % 4 != 0 and (401 + V) % 4 != 0)
    N = 230

    def check(i, dist, bitp, ex, a, b):
        assert bits_equal(dist, c["lstm"][a:b]).all(), f"V = {V}, instance {i}: distributions of bytes {a}..{b}"
        assert bits_equal(bitp, c["bitp"][a:b]).all(), f"V = {V}, instance {i}: bit predictions of bytes {a}..{b}"
        assert (ex.astype(np.int64) == c["ex"][a:b]).all(), f"V = {V}, instance {i}: ex of bytes {a}..{b}"
    hs, vote, _, _ = _three_handles(c["vocab"], c["ppmd"][:N], c["stream"][:N], N, check)
    try:
        lay = {a["name"]: a for a in E.lstm_layout(hs[0])}
        assert len(lay) == 80
        assert lay["W[0][0]"]["words"] == lay["WT[0][0]"]["words"] == 200 * (201 + 2 * V) and lay["W[1][2]"]["words"] == 200 * (401 + 2 * V)
        assert lay["W[1][0]"]["offset"] == 3 * 200 * (201 + 2 * V) and lay["layer_input[1]"]["words"] == 100 * (401 + V)
        assert lay["OL"]["words"] == 100 * V * 401 and lay["output"]["offset"] == lay["OL"]["words"]
        assert lay["bp_symbol"] == {"name": "bp_symbol", "region": "indices", "offset": 100, "words": 100}
    finally:
        vote.close()
        for h in hs:
            h.close()


# ---- the bare pipeline: no fxcm / paq8 stage, the caller's columns ---------------------------------------------------------------

N_CHUNK = 256
JOURNAL_LOG2 = 10


def _bare(lstm_shadow, nchunks, before=None, shadow=0, ctx_shadow=0, verify=False, journal=0, fill=None):
    """a Pipeline over nchunks chunks of 256 synthetic text bytes; columns 3..2024 are the caller's (a seeded grid); fill(): before the handle and
    before every submit"""
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    data = np.frombuffer(S.enwik_like(4 * N_CHUNK, 21), np.uint8)
    rng = np.random.default_rng(8)
    cols = (rng.integers(1, 4095, (8 * 4 * N_CHUNK, 2078)).astype(np.float32) * np.float32(1.0 / 4095)).astype(np.float32)
    layer0 = torch.from_numpy(cols).cuda()
    p = torch.full((8 * 4 * N_CHUNK,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if fill:
        fill()
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
        if lstm_shadow:
            pipe.set_lstm_shadow(lstm_shadow)
        if journal:
            pipe.set_journal(journal)

        def submit(i):
            a, b = i * N_CHUNK, (i + 1) * N_CHUNK
            if fill:
                pipe.sync()
                fill()
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
    """the run without shadows, once: p of four chunks, its journal, the queue counts"""
    from cmix_amd import engine as E
    q0 = E.hw_queues()
    pipe, p, _, _ = _bare(0, 4, journal=JOURNAL_LOG2)
    try:
        pipe.sync()
        q1 = E.hw_queues()
        assert pipe.lstm_shadow_report()["raw"] == [0] * 8
        out = {"p": p.cpu().numpy().copy(), "journal": pipe.journal(), "q0": q0, "q1": q1}
    finally:
        pipe.close()
    assert E.hw_queues() == q0
    return out


def _inject_gamma(pipe, instance=0):
    pipe.debug_lstm_shadow_xor(instance, "gb", 0, GAMMA_MASK)


def test_pipeline_lstm_shadow_clean_run_then_the_primary_is_perturbed(clean):
    from cmix_amd import engine as E
    pipe, p_on, submit, _ = _bare(2, 3)
    try:
        assert E.hw_queues() == clean["q1"] + 2
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.lstm_shadow_report()["raw"] == [3, 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.lstm_shadow_state_diff(0, 1)["words"] == 0 and pipe.lstm_shadow_state_diff(1, 2)["words"] == 0
        with pytest.raises(E.CmxError, match="before the first chunk"):
            pipe.set_lstm_shadow(1)
        with pytest.raises(E.CmxError, match="refused"):
            pipe.debug_lstm_shadow_xor(0, "indices", 0, 1)
        _inject_gamma(pipe)
        sd = pipe.lstm_shadow_state_diff(0, 1)
        assert sd["words"] == 1 and sd["first"]["region"] == 4 and sd["first"]["index"] == 0
        submit(3)
        with pytest.raises(E.CmxError) as e:
            pipe.wait(3)
        msg = str(e.value)
        assert "chunk 3" in msg and "stream byte %d" % (3 * N_CHUNK) in msg and "instance 0" in msg and "the stream's own stage" in msg
        assert "distribution entry" in msg or "prediction (layer-0 column 2077)" in msg or "'s ex" in msg
        rep = pipe.lstm_shadow_report()
        assert rep["events"] == 1 and (rep["first_bit"], rep["odd"]) == (3 * N_CHUNK, 0)
        w = pipe.lstm_shadow_values()["words"]
        assert w.shape == (3, 272) and np.array_equal(w[1], w[2]) and w[0, rep["column"]] != w[1, rep["column"]]
        with pytest.raises(E.CmxError, match="void"):   # the handle is voided ...
            submit(0)
        assert pipe.lstm_shadow_state_diff(1, 2)["words"] == 0   # ... and can still be diagnosed
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]


def test_pipeline_one_lstm_shadow_has_no_majority_and_refusals(clean):
    from cmix_amd import engine as E

    def refusals(pipe):
        with pytest.raises(E.CmxError, match="0, 1 or 2"):
            pipe.set_lstm_shadow(3)
        pipe.set_lstm_shadow(2)
        q = E.hw_queues()
        with pytest.raises(E.CmxError, match="shadow LSTM stages are set"):
            pipe.set_tolerance(True)
        pipe.set_lstm_shadow(0)          # dropped again: the queues go back
        assert E.hw_queues() == q - 2
    pipe, _, submit, _ = _bare(1, 1, before=refusals)
    try:
        assert E.hw_queues() == clean["q1"] + 1
        assert pipe.lstm_shadow_report()["raw"] == [1, N_CHUNK, 2, 0, 0, 0, 0, 0]
        _inject_gamma(pipe)
        submit(1)
        with pytest.raises(E.CmxError, match="no majority between 2 instances") as e:
            pipe.wait(1)
        assert "chunk 1" in str(e.value) and "stream byte %d" % N_CHUNK in str(e.value)
        rep = pipe.lstm_shadow_report()
        assert rep["events"] == 1 and rep["odd"] is None and rep["first_bit"] == N_CHUNK
        with pytest.raises(E.CmxError, match="no such instance"):
            pipe.lstm_shadow_state_diff(0, 2)
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)   # with the tolerance switch: refused
    try:
        pipe.set_tolerance(True)
        with pytest.raises(E.CmxError, match="tolerance switch"):
            pipe.set_lstm_shadow(1)
    finally:
        pipe.close()


def test_pipeline_lstm_shadow_after_pretrain(clean):
    """the LSTM is not pretrained: shadows may be set behind the dictionary, and agree"""
    from cmix_amd import synth as S
    pipe, _, _, _ = _bare(2, 2, before=lambda pipe: pipe.pretrain(S.enwik_like(300, 4)))
    try:
        pipe.sync()
        assert pipe.lstm_shadow_report()["raw"] == [2, 2 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.lstm_shadow_state_diff(0, 2)["words"] == 0
    finally:
        pipe.close()


def test_pipeline_lstm_shadow_beside_every_other_guard(clean):
    pipe, p_on, _, _ = _bare(2, 3, shadow=2, ctx_shadow=2, verify=True, journal=JOURNAL_LOG2)
    try:
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.lstm_shadow_report()["raw"] == [3, 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.ctx_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        ver = pipe.verify_report()
        assert ver["chunks"] == 3 and ver["mismatches"] == 0
        ends, words = pipe.journal()
        nb = (8 * 3 * N_CHUNK) >> JOURNAL_LOG2
        assert len(ends) == nb and np.array_equal(ends, clean["journal"][0][:nb]) and np.array_equal(words, clean["journal"][1][:nb])
    finally:
        pipe.close()


def test_pipeline_lstm_shadow_with_poisoned_lds(clean):
    """three LSTM instances' block kernels (LDS-resident weights, ~130 KB per workgroup) with every compute unit's LDS overwritten before the handle
    and before every submit: p and the record are those of the clean run"""
    from cmix_amd import engine as E
    calls = []

    def fill():
        r = E.lds_fill(0xFFFFFFFF)
        assert r["full"] and r["workgroups"] >= r["compute_units"] > 0, "LDS fill did not cover the device: %r" % (r,)
        calls.append(r)
    pipe, p_on, _, _ = _bare(2, 3, fill=fill)
    try:
        pipe.sync()
        assert len(calls) == 4
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.lstm_shadow_report()["raw"] == [3, 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.lstm_shadow_state_diff(0, 1)["words"] == 0 and pipe.lstm_shadow_state_diff(0, 2)["words"] == 0
    finally:
        pipe.close()


# ---- the whole engine --------------------------------------------------------------------------------------------------------

def _golden_64k():
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        return z["sha256"].tobytes(), int(z["size"][0]), int(z["seed"][0]), int(z["seed"][1])


def test_engine_stream_64k_with_two_lstm_shadows_writes_the_reference_file():
    from cmix_amd import synth as S
    from cmix_amd.pipeline import EngineStream, text_file_stream
    want_sha, want_size, n, seed = _golden_64k()
    stream = text_file_stream(S.enwik_like(n, seed))
    eng = EngineStream(0, stream, 4096, lstm_shadow=2)
    try:
        eng.feed(len(stream))
        got = eng.finish()
        rep = eng.pipe.lstm_shadow_report()
    finally:
        eng.close()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["raw"] == [(len(stream) + 4095) // 4096, len(stream), 3, 0, 0, 0, 0, 0]


def test_dropin_program_with_cmix_lstm_shadow_writes_the_reference_file():
    from cmix_amd import synth as S
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    want_sha, want_size, n, seed = _golden_64k()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(S.enwik_like(n, seed))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, CMIX_LSTM_SHADOW="2"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
