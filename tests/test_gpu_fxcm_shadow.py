"""GPU: shadow fxcm stages and their vote (include/cmix_amd.h: cmx_fxcm_create_shadow / _run_shared, cmx_fxcmvote_*, cmx_fxcm_state_diff,
cmx_pipeline_set_fxcm_shadow). The unchanged roles kernel runs on two or three FxDev over ONE parser's records, the same bytes and the
same LSTM hints; the vote kernel compares every bit's 431 values word for word and names the first differing bit, column and the odd instance; the
state diff compares every table word of two handles in HBM. A perturbation is a data change made by a test hook between launches, in a region whose
words the kernels never address memory with: no kernel is altered, no wait times out, no fault is provoked. Every test asserts that the instances'
sticky hand-off flags stay clear."""
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal
from test_fxcm_stage_host import compare, hints, oracle_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

NONE = (1 << 64) - 1
WX_M = [2048, 1536, 6144, 2048, 1536, 7168, 0x4000, 0x4000, 0x20000, 0x20000, 224, 1]   # rows per mixer (fxcm_build.h)
WX11 = sum(256 * m for m in WX_M[:10]) + 8 * WX_M[10]   # word offset of wx[11] in region "wx": ten tables of rows of 512 weights, one of rows of 16
WX_MASK = 0x40004000   # weights 0 and 1 of final mixer 11's only row (selected at every bit): +-16384 of 65536, a value like any other
REFUSED = ("const_tables", "map_buckets", "mhash", "sp_table", "buffer", "fxdev")


# ---- the vote kernel against its host twin ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _base(T, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (T, 431), dtype=np.uint64).astype(np.uint32)


def _instances(n, T, seed):
    return [_base(T, seed).copy() for _ in range(n)]


def _to_dev(rows, lead):
    """device copies: instance 0 inside a [T, 2078] matrix of other words (columns 3..433: its row base is 4-byte aligned only, differently from row to
    row), the others inside [T, 434] ones; lead = 1: every matrix starts one row into its allocation"""
    import torch
    T = rows[0].shape[0]
    out = []
    for i, r in enumerate(rows):
        width = 2078 if i == 0 else 434
        buf = torch.randint(-(1 << 31), (1 << 31) - 1, (T + lead, width), dtype=torch.int32, device="cuda")[lead:]
        buf[:, 3:434] = torch.from_numpy(r.view(np.int32)).cuda()
        out.append(buf)
    return out


# T: one byte, one below and one above a wave's worth of rows (a partial last workgroup), 520 rows without a grid-stride step, 4096 rows on the grid's
# 2048 waves (two rows per wave: the grid stride)
@pytest.mark.parametrize("c", [0, 63, 64, 430])
@pytest.mark.parametrize("row", ["first", "last"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T", [8, 63, 65, 520, 4096])
def test_vote_kernel_equals_the_host_twin(T, n, row, c):
    import torch
    from cmix_amd import engine as E
    from cmix_amd.fxcmvote import chunk_result, fxcm_vote_reference
    rows = _instances(n, T, 17 + T)
    inst = (c + (row == "last")) % n
    t = 0 if row == "first" else T - 1
    rows[inst][t, c] ^= np.uint32(0x80000000 if row == "last" else 1)
    want, want_words = fxcm_vote_reference(rows, 5000)
    assert want == [1, T, n, 1, 5000 + t, c, inst if n == 3 else NONE, 1]
    lead = 1 if T == 63 else 0
    data = (torch.arange((T + 7) // 8, device="cuda") * 37 % 251).to(torch.uint8)
    v = E.FxcmVote(n)
    try:
        dev = _to_dev(rows, lead)
        assert dev[0].shape == (T, 2078) and dev[1].shape == (T, 434)
        v.run(dev, 5000, data)
        rep, val = v.report(), v.values()
        assert rep["raw"] == want
        byte = (t >> 3) * 37 % 251
        assert np.array_equal(val["words"], want_words) and val["byte"] == byte and val["bit"] == (byte >> (7 - (t & 7))) & 1
        assert v.last()["raw"] == chunk_result(rows, 5000)
        # a second chunk on the same handle, with another difference: the record keeps the first event, `last` has the second
        rows2 = _instances(n, T, 99 + T)
        rows2[0][T - 1, 20] ^= np.uint32(2)
        v.run(_to_dev(rows2, lead), 5000 + T)
        assert v.report()["raw"] == [2, 2 * T, n, 2] + want[4:]
        assert np.array_equal(v.values()["words"], want_words)
        assert v.last()["raw"] == chunk_result(rows2, 5000 + T) == [1, 5000 + 2 * T - 1, 20, 0 if n == 3 else NONE]
        # and a clean one
        v.run(_to_dev(_instances(n, T, 100 + T), lead), 5000 + 2 * T)
        assert v.report()["raw"] == [3, 3 * T, n, 2] + want[4:]
        assert v.last()["raw"] == [0, 0, 0, 0]
    finally:
        v.close()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T", [8, 63, 65, 520, 4096])
def test_vote_kernel_all_agree(T, n):
    """all agree: the record is [1, T, n, 0, 0, 0, 0, 0]; then -0.0 against 0.0: different words"""
    import torch
    from cmix_amd import engine as E
    v = E.FxcmVote(n)
    try:
        dev = _to_dev(_instances(n, T, 5 + T), 0)
        v.run(dev, 0)
        assert v.report()["raw"] == [1, T, n, 0, 0, 0, 0, 0] and v.last()["raw"] == [0, 0, 0, 0]
        f = [d.view(torch.float32) for d in dev]
        for d in f:
            d[T - 1, 3 + 430] = 0.0
        f[n - 1][T - 1, 3 + 430] = -0.0   # == 0.0 as a float
        v.run(dev, T)
        assert v.report()["raw"] == [2, 2 * T, n, 1, 2 * T - 1, 430, n - 1 if n == 3 else NONE, 1]
    finally:
        v.close()


# ---- three bare handles on one parser's records ------------------------------------------------------------------------------------

RAGGED = [1, 7, 100, 1000, 892]
N_ORACLE = 2200


@functools.lru_cache(maxsize=None)
def _text_case():
    from cmix_amd import synth
    data = np.frombuffer(synth.enwik_like(4000, 31), np.uint8)
    pr, ex = hints(8 * len(data), 7)
    return data, pr, ex, oracle_rows(data[:N_ORACLE], pr, ex)


class _Three:
    """an owner and two shadows over one stream; launch(a, b) runs bytes a..b on all three (the owner in place into layer-0 rows of 2078, the shadows
    into rows of 434) and votes"""

    def __init__(self, n_inst=3):
        from cmix_amd import engine as E
        self.E = E
        self.hs = [E.Fxcm(None, 0)]
        try:
            self.hs += [E.Fxcm(device=0, shadow=True) for _ in range(n_inst - 1)]
            self.vote = E.FxcmVote(n_inst)
        except Exception:
            self.close()
            raise
        self.data, self.pr, self.ex, self.want = _text_case()
        self.held = []

    def tensors(self, a, b):
        import torch
        return (torch.from_numpy(np.ascontiguousarray(self.pr[8 * a:8 * b], np.int16)).cuda(), torch.from_numpy(np.ascontiguousarray(self.ex[8 * a:8 * b], np.uint8)).cuda(),
                [torch.full((8 * (b - a), 2078 if i == 0 else 434), -1.0, dtype=torch.float32, device="cuda") for i in range(len(self.hs))])

    def launch(self, a, b, tensors=None, streams=None, vote=True):
        import torch
        pr, ex, probs = tensors or self.tensors(a, b)
        st = streams or [None] * len(self.hs)
        self.hs[0].run(self.data[a:b], pr, ex, probs[0], stream=st[0])
        for i, h in enumerate(self.hs[1:], 1):
            h.run_shared(self.hs[0], probs[i], stream=st[i])
        self.held.append((pr, ex, probs))
        if vote:
            torch.cuda.synchronize()
            self.vote.run(probs, 8 * a, self.hs[0]._last[0])
        return probs

    def rows(self, probs):
        import torch
        torch.cuda.synchronize()
        out = []
        for p in probs:
            got = p.cpu().numpy()
            assert (got[:, :3] == -1.0).all() and (got.shape[1] == 434 or (got[:, 434:] == -1.0).all())   # columns outside 3..433 are not the stage's
            out.append(np.ascontiguousarray(got[:, 3:434]))
        return out

    def clear(self):
        for i, h in enumerate(self.hs):
            assert not h.failed(), "a bounded wait of the roles kernel of instance %d ran out" % i

    def close(self):
        if getattr(self, "vote", None):
            self.vote.close()
        for h in self.hs:
            h.close()


def _ragged_run(three):
    """the 2000 bytes in ragged launches, every instance's rows against the oracle, a clean vote"""
    pos = 0
    for k, n in enumerate(RAGGED):
        got = three.rows(three.launch(pos, pos + n))
        for i, g in enumerate(got):
            compare(g, three.want[8 * pos:8 * (pos + n)], "instance %d, launch %d" % (i, k))
        assert three.vote.last()["raw"] == [0, 0, 0, 0]
        pos += n
    assert pos == 2000 and three.vote.report()["raw"] == [len(RAGGED), 8 * 2000, len(three.hs), 0, 0, 0, 0, 0]
    three.clear()
    return pos


def test_three_handles_on_shared_records_agree_and_pair_up():
    three = _Three()
    E = three.E
    try:
        _ragged_run(three)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            sd = three.hs[a].state_diff(three.hs[b])
            assert sd["words"] == 0 and sd["first"] is None and not any(sd["per_region"].values()), (a, b, sd)
        with pytest.raises(E.CmxError, match="same handle"):
            three.hs[0].state_diff(three.hs[0])
        lay = {a["name"]: a for a in E.fxcm_layout(three.hs[1])}
        assert len(lay) == 141 and lay["wx[11]"] == {"name": "wx[11]", "region": "wx", "offset": WX11, "words": 8}
        assert lay["apm_t[0]"]["offset"] == 0 and lay["apm_t[0]"]["words"] == (256 * 33 * 2 + 4 + 3) // 4 and lay["maps[0].sm"]["words"] == 3 * 256
        assert lay["squash"]["words"] == 4095 * 2 // 4 + 1 and lay["buffer"]["words"] == (1 << 24) // 4 and lay["FxDev"]["region"] == "fxdev"
        for region in REFUSED:   # words the kernels address memory or bound loops with
            with pytest.raises(E.CmxError, match="refused"):
                three.hs[2].debug_state_xor(region, 0, 1)
        with pytest.raises(E.CmxError, match="no parser"):   # a shadow cannot parse
            three.hs[1].run(three.data[:4], *three.tensors(0, 4)[:2])
        with pytest.raises(E.CmxError, match="every chunk of its owner, once"):   # nor run a chunk twice
            three.hs[1].run_shared(three.hs[0])
        three.clear()
    finally:
        three.close()


def _trained_word(h, region, offset, words, run):
    """a word of the window [offset, offset + words) of `region` that run() changes -- read out before and after it: a word the launch trained, and so
    one of the few the stage is working with -- preferring one that the launch before it had changed too"""
    s0 = h.debug_state_read(region, offset, words)
    run(0)
    s1 = h.debug_state_read(region, offset, words)
    run(1)
    s2 = h.debug_state_read(region, offset, words)
    both = np.flatnonzero((s0 != s1) & (s1 != s2))
    cand = both if len(both) else np.flatnonzero(s1 != s2)
    assert len(cand), "no word of %s changed in two launches: the window is not a table the stage trains" % region
    return offset + int(cand[0])


@pytest.mark.parametrize("region, inst, mask", [("wx", 2, WX_MASK), ("apm", 1, 0x40004000), ("map_statemaps", 2, 0x40000000)])
def test_one_perturbed_word_is_found_by_state_diff_and_named_by_the_next_vote(region, inst, mask):
    """wx: weights 0, 1 of final mixer 11's one row; apm: two cells of APM 0 (contexts c0: 256 rows); map_statemaps: a StateMap cell of map 0 -- each a
    word the last two launches trained. The perturbed instance is the odd one of the next launch; the other two still pair up word for word."""
    three = _Three()
    try:
        pos = 0
        for n in RAGGED[:3]:
            three.launch(pos, pos + n)
            pos += n
        cuts = [(pos, pos + 1000), (pos + 1000, pos + 1892)]
        lay = {a["name"]: a for a in three.E.fxcm_layout(three.hs[0])}
        name = {"wx": "wx[11]", "apm": "apm_t[0]", "map_statemaps": "maps[0].sm"}[region]
        index = _trained_word(three.hs[inst], region, lay[name]["offset"], lay[name]["words"], lambda k: three.launch(*cuts[k]))
        if region == "wx":
            index = WX11   # word 0 of the one row: selected at every bit, whatever was trained
        assert three.vote.report()["raw"] == [5, 8 * 2000, 3, 0, 0, 0, 0, 0]
        others = [i for i in range(3) if i != inst]
        three.hs[inst].debug_state_xor(region, index, mask)
        sd = three.hs[inst].state_diff(three.hs[others[0]])
        assert sd["words"] == 1 and sd["per_region"][region] == 1 and sum(sd["per_region"].values()) == 1
        f = sd["first"]
        assert (f["region"], f["index"]) == (three.E.FXCM_STATE_REGIONS.index(region), index) and f["a"] == f["b"] ^ mask
        assert three.hs[others[0]].state_diff(three.hs[others[1]])["words"] == 0
        got = three.rows(three.launch(2000, 2600))
        last, rep = three.vote.last(), three.vote.report()
        assert last["elements"] > 0 and last["odd"] == inst, (region, index, last)
        assert rep["events"] == 1 and rep["odd"] == inst and 8 * 2000 <= rep["first_bit"] < 8 * 2600
        t, c = rep["first_bit"] - 8 * 2000, rep["column"]
        w = three.vote.values()["words"]
        assert np.array_equal(w[others[0]], w[others[1]]) and w[inst, c] != w[others[0], c]
        assert all(np.array_equal(w[i], got[i][t].view(np.uint32)) for i in range(3))
        for i in others:   # the majority still follows the oracle
            compare(got[i][:8 * (2200 - 2000)], three.want[8 * 2000:], "instance %d behind the perturbation of instance %d" % (i, inst))
        assert three.hs[others[0]].state_diff(three.hs[others[1]])["words"] == 0 and three.hs[inst].state_diff(three.hs[others[0]])["words"] >= 1
        three.clear()
    finally:
        three.close()


def test_staging_ring_with_readers_seventeen_launches_without_a_host_sync():
    """17 launches of 128 bytes on the ring's 8 slots, owner and two shadows on streams of their own, nothing waited for by the host in between (after
    the first launch has sized the row buffers): a staging slot is refilled only when the owner's launch AND both readers' launches on it are done"""
    import torch
    three = _Three()
    try:
        n, k = 128, 17
        tens = [three.tensors(i * n, (i + 1) * n) for i in range(k)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in three.hs]
        sids = [s.cuda_stream for s in streams]
        probs = [three.launch(i * n, (i + 1) * n, tens[i], sids, vote=False) for i in range(k)]
        for h in three.hs:
            h.sync()
        three.clear()
        waits = three.hs[0].debug_ring_waits()
        print("ring waits that met a launch (the owner's or a reader's) in flight: %d of %d reuses" % (waits, k - 8))
        assert 0 < waits <= k - 8
        for i, p in enumerate(probs):
            for j, g in enumerate(three.rows(p)):
                compare(g, three.want[8 * i * n:8 * (i + 1) * n], "launch %d, instance %d" % (i, j))
    finally:
        three.close()


def test_three_instances_agree_under_jitter(monkeypatch):
    """CMX_FXCM_JITTER with one seed: the owner stalls with that seed, every shadow with one derived from it, so the three instances' roles lead and
    lag each other at different bits; the rows are the oracle's and the vote is clean"""
    monkeypatch.setenv("CMX_FXCM_JITTER", "5")
    three = _Three()
    try:
        pos = 0
        for n in (100, 400):
            for i, g in enumerate(three.rows(three.launch(pos, pos + n))):
                compare(g, three.want[8 * pos:8 * (pos + n)], "instance %d under jitter" % i)
            pos += n
        assert three.vote.report()["raw"] == [2, 8 * 500, 3, 0, 0, 0, 0, 0]
        counts = [h.debug_jitter_counts() for h in three.hs]
        print("stall counts per instance:", counts)
        assert all(sum(c) > 0 for c in counts) and not (counts[0] == counts[1] == counts[2])
        three.clear()
    finally:
        three.close()


# ---- the pipeline: fxcm on the device, the caller's columns 434..2024 --------------------------------------------------------------

N_CHUNK = 256
JOURNAL_LOG2 = 10


def _bare(fxcm_shadow, nchunks, before=None, pretrain=None, shadow=0, ctx_shadow=0, lstm_shadow=0, verify=False, journal=0, fill=None, enable=True):
    """a Pipeline over nchunks chunks of 256 synthetic text bytes with the fxcm stage on the device; columns 434..2024 are the caller's (a seeded grid);
    fill(): before the handle and before every submit"""
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
        if enable:
            pipe.enable_fxcm(None)
        if before:
            before(pipe)
        if fxcm_shadow:
            pipe.set_fxcm_shadow(fxcm_shadow)
        if pretrain is not None:
            pipe.pretrain(pretrain)
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
    """the run without shadows, once: p of four chunks, its fxcm columns, its journal, the queue counts"""
    from cmix_amd import engine as E
    q0 = E.hw_queues()
    pipe, p, _, layer0 = _bare(0, 4, journal=JOURNAL_LOG2)
    try:
        pipe.sync()
        q1 = E.hw_queues()
        assert pipe.fxcm_shadow_report()["raw"] == [0] * 8
        out = {"p": p.cpu().numpy().copy(), "rows": layer0[:, 3:434].cpu().numpy().copy(), "journal": pipe.journal(), "q0": q0, "q1": q1}
    finally:
        pipe.close()
    assert E.hw_queues() == q0
    return out


def test_pipeline_fxcm_shadow_clean_run_then_the_primary_is_perturbed(clean):
    from cmix_amd import engine as E
    pipe, p_on, submit, layer0 = _bare(2, 3)
    try:
        assert E.hw_queues() == clean["q1"] + 2
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.fxcm_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.fxcm_shadow_state_diff(0, 1)["words"] == 0 and pipe.fxcm_shadow_state_diff(1, 2)["words"] == 0
        with pytest.raises(E.CmxError, match="before the first chunk"):
            pipe.set_fxcm_shadow(1)
        with pytest.raises(E.CmxError, match="refused"):
            pipe.debug_fxcm_shadow_xor(0, "fxdev", 0, 1)
        pipe.debug_fxcm_shadow_xor(0, "wx", WX11, WX_MASK)
        sd = pipe.fxcm_shadow_state_diff(0, 1)
        assert sd["words"] == 1 and sd["first"]["region"] == 9 and sd["first"]["index"] == WX11
        submit(3)
        with pytest.raises(E.CmxError) as e:
            pipe.wait(3)
        msg = str(e.value)
        rep = pipe.fxcm_shadow_report()
        assert rep["events"] == 1 and rep["odd"] == 0 and 8 * 3 * N_CHUNK <= rep["first_bit"] < 8 * 4 * N_CHUNK
        assert "chunk 3" in msg and "stream bit %d (byte %d, bit %d)" % (rep["first_bit"], rep["first_bit"] >> 3, rep["first_bit"] & 7) in msg
        assert "instance 0" in msg and "the stream's own stage" in msg and "fxcm column %d (layer-0 column %d)" % (rep["column"], 3 + rep["column"]) in msg
        val = pipe.fxcm_shadow_values()
        w = val["words"]
        assert w.shape == (3, 431) and np.array_equal(w[1], w[2]) and w[0, rep["column"]] != w[1, rep["column"]]
        row0 = layer0[rep["first_bit"], 3:434].cpu().numpy().view(np.uint32)   # instance 0 was read in place
        assert np.array_equal(w[0], row0)
        with pytest.raises(E.CmxError, match="void"):   # the handle is voided ...
            submit(0)
        assert pipe.fxcm_shadow_state_diff(1, 2)["words"] == 0   # ... and can still be diagnosed
        assert "hand-off" not in msg   # no instance's sticky time-out flag was set
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]


def test_pipeline_one_fxcm_shadow_has_no_majority_and_refusals(clean):
    from cmix_amd import engine as E
    from cmix_amd import synth as S

    def refusals(pipe):
        with pytest.raises(E.CmxError, match="0, 1 or 2"):
            pipe.set_fxcm_shadow(3)
        pipe.set_fxcm_shadow(2)
        q = E.hw_queues()
        pipe.set_tolerance(True)         # fxcm has no tolerance form: the switch and the shadows coexist
        pipe.set_tolerance(False)
        pipe.set_fxcm_shadow(0)          # dropped again: the queues go back
        assert E.hw_queues() == q - 2
    pipe, _, submit, _ = _bare(1, 1, before=refusals)
    try:
        assert E.hw_queues() == clean["q1"] + 1
        assert pipe.fxcm_shadow_report()["raw"] == [1, 8 * N_CHUNK, 2, 0, 0, 0, 0, 0]
        pipe.debug_fxcm_shadow_xor(1, "wx", WX11, WX_MASK)
        submit(1)
        with pytest.raises(E.CmxError, match="no majority between 2 instances") as e:
            pipe.wait(1)
        assert "chunk 1" in str(e.value) and "fxcm column" in str(e.value)
        rep = pipe.fxcm_shadow_report()
        assert rep["events"] == 1 and rep["odd"] is None and 8 * N_CHUNK <= rep["first_bit"] < 16 * N_CHUNK
        with pytest.raises(E.CmxError, match="no such instance"):
            pipe.fxcm_shadow_state_diff(0, 2)
    finally:
        pipe.close()
    assert E.hw_queues() == clean["q0"]
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)
    try:
        with pytest.raises(E.CmxError, match="cmx_pipeline_enable_fxcm first"):   # without the stage on the device
            pipe.set_fxcm_shadow(1)
        pipe.enable_fxcm(None)
        pipe.pretrain(S.enwik_like(300, 4))
        with pytest.raises(E.CmxError, match="before cmx_pipeline_pretrain"):     # behind the dictionary: a shadow would have missed it
            pipe.set_fxcm_shadow(1)
        assert E.hw_queues() == clean["q1"]
    finally:
        pipe.close()


def test_pipeline_fxcm_shadows_learn_the_dictionary(clean):
    from cmix_amd import synth as S
    pipe, _, _, layer0 = _bare(2, 2, pretrain=S.enwik_like(300, 4))
    try:
        pipe.sync()
        assert pipe.fxcm_shadow_report()["raw"] == [2, 8 * 2 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert pipe.fxcm_shadow_state_diff(a, b)["words"] == 0, (a, b)
        rows = layer0[:8 * 2 * N_CHUNK, 3:434].cpu().numpy()
        assert not bits_equal(rows, clean["rows"][:8 * 2 * N_CHUNK]).all(), "the rows equal a run without pretraining: the dictionary was not learned"
    finally:
        pipe.close()


def test_pipeline_fxcm_shadow_beside_every_other_guard(clean):
    pipe, p_on, _, _ = _bare(2, 3, shadow=2, ctx_shadow=2, lstm_shadow=2, verify=True, journal=JOURNAL_LOG2)
    try:
        pipe.sync()
        assert bits_equal(p_on.cpu().numpy()[:8 * 3 * N_CHUNK], clean["p"][:8 * 3 * N_CHUNK]).all()
        assert pipe.fxcm_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
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


def test_pipeline_fxcm_shadow_with_poisoned_lds(clean):
    """three instances' roles kernels (~150 KB of LDS per workgroup) with every compute unit's LDS overwritten before the handle and before every
    submit: p and the record are those of the clean run"""
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
        assert pipe.fxcm_shadow_report()["raw"] == [3, 8 * 3 * N_CHUNK, 3, 0, 0, 0, 0, 0]
        assert pipe.fxcm_shadow_state_diff(0, 1)["words"] == 0 and pipe.fxcm_shadow_state_diff(0, 2)["words"] == 0
    finally:
        pipe.close()


# ---- the whole engine --------------------------------------------------------------------------------------------------------

def _golden_64k():
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        return z["sha256"].tobytes(), int(z["size"][0]), int(z["seed"][0]), int(z["seed"][1])


def test_engine_stream_64k_with_two_fxcm_shadows_writes_the_reference_file():
    from cmix_amd import synth as S
    from cmix_amd.pipeline import EngineStream, text_file_stream
    want_sha, want_size, n, seed = _golden_64k()
    stream = text_file_stream(S.enwik_like(n, seed))
    eng = EngineStream(0, stream, 4096, fxcm_shadow=2)
    try:
        eng.feed(len(stream))
        got = eng.finish()
        rep = eng.pipe.fxcm_shadow_report()
    finally:
        eng.close()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["raw"] == [(len(stream) + 4095) // 4096, 8 * len(stream), 3, 0, 0, 0, 0, 0]


def test_dropin_program_with_cmix_fxcm_shadow_writes_the_reference_file():
    from cmix_amd import synth as S
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    want_sha, want_size, n, seed = _golden_64k()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(S.enwik_like(n, seed))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, CMIX_FXCM_SHADOW="2"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
