"""GPU: an outvoted mixing network is repaired from the majority and the stream carries on (include/cmix_amd.h: cmx_mixnet_state_repair, cmx_vote_last,
cmx_pipeline_set_shadow_repair). The shapes are those of test_gpu_shadow.py: three handles on the synthetic stream, the bare pipeline
with 256-byte chunks, the whole engine on the 64 KB golden. An event is a data change made by a test hook between chunks: no kernel stops, no wait
times out."""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits_equal, synth_mixnet_inputs

pytestmark = pytest.mark.gpu

MASK = 0x00400000
MASK2 = 0x00200000
T1 = 400   # bits per step of the bare handles


# ---- the chunk's own result against its host twin ---------------------------------------------------------------------------------

def test_vote_last_is_the_chunks_own_result():
    import torch
    from cmix_amd import engine as E
    from cmix_amd.vote import NONE, chunk_result
    T = 1000
    rng = np.random.default_rng(4)

    def instances():
        p = rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)
        m = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
        return [p.copy() for _ in range(3)], [m.copy() for _ in range(3)]

    def dev(ps, ms):
        return ([torch.from_numpy(p.view(np.int32)).cuda() for p in ps], [torch.from_numpy(m.view(np.int32)).cuda() for m in ms])
    v = E.Vote(3)
    try:
        ps, ms = instances()
        ms[2][500, 7] ^= 1
        ps[2][999] ^= 1
        v.run(*dev(ps, ms), 3000)
        assert v.last()["raw"] == chunk_result(ps, ms, 3000) == [2, 3500, 7, 2]
        ps, ms = instances()                      # a clean chunk: its own result is clean, the sticky record still holds the first event
        v.run(*dev(ps, ms), 4000)
        assert v.last()["raw"] == [0, 0, 0, 0] and v.last()["odd"] is None
        assert v.report()["raw"] == [2, 2 * T, 3, 1, 3500, 7, 2, 2]
        ms[0][10, 0] ^= 1
        ms[1][900, 46] ^= 1                       # two odd instances in one chunk: no single one to repair
        v.run(*dev(ps, ms), 5000)
        assert v.last()["raw"] == chunk_result(ps, ms, 5000) == [2, 5010, 0, NONE]
        ms[1][900, 46] ^= 1
        ms[1][10, 0] ^= 2                         # all three differ at one element
        v.run(*dev(ps, ms), 6000)
        assert v.last()["raw"] == chunk_result(ps, ms, 6000) == [1, 6010, 0, NONE]
        assert v.report()["raw"] == [4, 4 * T, 3, 3, 3500, 7, 2, 2]
    finally:
        v.close()


# ---- state_repair on three bare handles -------------------------------------------------------------------------------------------

class _Three:
    def __init__(self):
        import torch
        from cmix_amd import engine as E
        self.torch = torch
        probs, sel, bits = synth_mixnet_inputs(2 * T1, seed=5, n_ctx_bits=2)
        self.d = (torch.from_numpy(np.ascontiguousarray(probs)).cuda(),
                  torch.from_numpy((sel & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
                  torch.from_numpy(np.ascontiguousarray(bits)).cuda())
        self.nets = [E.MixNet(0) for _ in range(3)]
        self.vote = E.Vote(3)
        self.p = [torch.empty(2 * T1, dtype=torch.float32, device="cuda") for _ in range(3)]
        self.mix = [torch.empty((2 * T1, 47), dtype=torch.float32, device="cuda") for _ in range(3)]

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


# one word in each of rows0, rows1, rows2, row_steps, an SSE table, x1 and the scalars (sse_pc: word 48 + 96 + 2 + 1 of region 10); row_steps has
# 47 * 10001 * 2 = 940094 words, two more than a multiple of four: (46, 9999, 1) is the last word of the last quad, (46, 10000, 0 / 1) are the tail
WORDS = [("rows0", 8, 0, 5), ("rows0", 25, 10000, 2111), ("rows1", 26, 0, 28), ("rows2", 46, 0, 48), ("row_steps", 3, 0, 0), ("row_steps", 46, 9999, 1),
         ("row_steps", 46, 10000, 0), ("row_steps", 46, 10000, 1), ("s6", None, None, 123457), ("x1", None, None, 1000), ("scalars", None, None, 147)]


def test_state_repair_makes_the_odd_handle_equal_and_leaves_the_source_alone():
    from cmix_amd import engine as E
    h = _Three()
    try:
        a, b, c = h.nets
        h.chunk(0, T1)
        assert a.state_diff(b)["words"] == 0
        rp = a.state_repair(b)                       # nothing differs: nothing is reported (and nothing stored)
        assert rp["words"] == 0 and rp["first"] is None and not any(rp["per_region"].values())
        for region, mixer, row, index in WORDS:
            a.debug_state_xor(region, mixer, row, index, 1 if region == "scalars" else MASK)
        sd = a.state_diff(b)
        assert sd["words"] == len(WORDS) and sd["per_region"]["row_steps"] == 4 and sd["per_region"]["scalars"] == 1
        assert sd["layer0_mask"] == (1 << 8) | (1 << 25) and sd["layer12_mask"] == 1 | (1 << 20)
        rp = a.state_repair(b)                       # one pass diagnoses and repairs: the state BEFORE it, word for word as the diff saw it
        assert rp["raw"] == sd["raw"]
        f = rp["first"]
        assert (f["region"], f["mixer"], f["row"], f["index"]) == (0, 8, 0, 5) and f["a"] == f["b"] ^ MASK
        assert a.state_diff(b)["words"] == 0
        assert b.state_diff(c)["words"] == 0         # the source was only read
        assert a.state_repair(b)["words"] == 0
        h.chunk(T1, 2 * T1)                          # and the three run on in agreement
        assert h.vote.report()["raw"] == [2, 2 * T1, 3, 0, 0, 0, 0, 0] and h.vote.last()["elements"] == 0
        assert a.state_diff(c)["words"] == 0
        with pytest.raises(E.CmxError, match="same handle"):
            a.state_repair(a)
    finally:
        h.close()


# ---- the bare pipeline: no fxcm / paq8 stage, the caller's columns ------------------------------------------------------------------

N_CHUNK = 256
N_CHUNKS = 7


def _bare(shadow, repair=0, before=None, verify=False):
    """a Pipeline over up to N_CHUNKS chunks of 256 synthetic text bytes; columns 3..2024 are the caller's (a seeded grid)"""
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    data = np.frombuffer(S.enwik_like(N_CHUNKS * N_CHUNK, 21), np.uint8)
    rng = np.random.default_rng(8)
    cols = (rng.integers(1, 4095, (8 * N_CHUNKS * N_CHUNK, 2078)).astype(np.float32) * np.float32(1.0 / 4095)).astype(np.float32)
    layer0 = torch.from_numpy(cols).cuda()
    p = torch.full((8 * N_CHUNKS * N_CHUNK,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)
    if verify:
        pipe.set_verify(True)
    if before:
        before(pipe)
    if shadow:
        pipe.set_shadow(shadow)
    if repair:
        pipe.set_shadow_repair(repair)

    def submit(i):
        a, b = i * N_CHUNK, (i + 1) * N_CHUNK
        pipe.submit(data[a:b].tobytes(), layer0[8 * a:8 * b], p[8 * a:8 * b])
    return pipe, p, submit


@pytest.fixture(scope="module")
def unperturbed_run():
    return _unperturbed_run()


@pytest.fixture(scope="module")
def unperturbed(unperturbed_run):
    """p of chunks 0 .. N_CHUNKS - 1 from a run without shadows"""
    return unperturbed_run[0]


def _unperturbed_run():
    import torch
    pipe, p, submit = _bare(0)
    try:
        mix = torch.zeros((8 * N_CHUNKS * N_CHUNK, 47), dtype=torch.float32, device="cuda")
        pipe.debug_mix_out(mix)
        for i in range(N_CHUNKS):
            submit(i)
            pipe.wait(i)
        pipe.sync()
        return p.cpu().numpy().copy(), mix.cpu().numpy().copy()
    finally:
        pipe.close()


@pytest.fixture(scope="module")
def unperturbed_mix(unperturbed_run):
    """and every bit's 47 mixer outputs, through the debug area"""
    return unperturbed_run[1]


def _three_clean_chunks(pipe, submit):
    for i in range(3):
        submit(i)
        pipe.wait(i)


@pytest.mark.parametrize("inst", [0, 2])
def test_pipeline_repairs_the_odd_instance_and_carries_on(unperturbed, inst):
    pipe, p, submit = _bare(2, repair=2)
    try:
        _three_clean_chunks(pipe, submit)
        assert pipe.shadow_repairs() == {"total": 0, "log": []}
        # mixer 26 is keyed by the constant zero context: its row 0 is used by every bit; weight 28 meets the LSTM's stretched prediction
        pipe.debug_shadow_xor(inst, "rows1", 26, 0, 28, MASK)
        for i in (3, 4, 5):      # in flight across the event
            submit(i)
        for i in (3, 4, 5):
            pipe.wait(i)
        rep = pipe.shadow_repairs()
        assert rep["total"] == 1 and len(rep["log"]) == 1
        e = rep["log"][0]
        assert (e["chunk"], e["bit"], e["column"], e["odd"], e["chunks"]) == (3, 8 * 3 * N_CHUNK, 26, inst, 3)
        assert e["words"] >= 1 and e["elements"] >= 1 and e["layer0_mask"] == 0 and e["layer12_mask"] & 1   # the origin lies in layer 1, mixer 26
        assert "stream bit %d" % (8 * 3 * N_CHUNK) in e["text"] and "origin mixer 26" in e["text"]
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert pipe.shadow_state_diff(a, b)["words"] == 0
        assert pipe.shadow_report()["events"] == 3   # the sticky record went on counting
        submit(6)                                     # the handle stays usable
        pipe.wait(6)
        pipe.sync()
        assert bits_equal(p.cpu().numpy(), unperturbed).all()
        assert pipe.shadow_repairs()["total"] == 1 and pipe.shadow_report()["events"] == 3
    finally:
        pipe.close()


def test_the_debug_areas_mixer_outputs_are_replaced_with_the_majoritys(unperturbed, unperturbed_mix):
    import torch
    pipe, p, submit = _bare(2, repair=1)
    try:
        mix = torch.zeros((8 * N_CHUNKS * N_CHUNK, 47), dtype=torch.float32, device="cuda")
        pipe.debug_mix_out(mix)
        _three_clean_chunks(pipe, submit)
        pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, MASK)
        submit(3)
        submit(4)
        pipe.wait(3)
        n = 8 * 5 * N_CHUNK     # both chunks in flight have the majority's values by now, before wait(4)
        assert bits_equal(mix.cpu().numpy()[:n], unperturbed_mix[:n]).all() and bits_equal(p.cpu().numpy()[:n], unperturbed[:n]).all()
        pipe.wait(4)
        assert pipe.shadow_repairs()["log"][0]["chunks"] == 2
    finally:
        pipe.close()


def test_no_majority_still_stops():
    from cmix_amd import engine as E
    pipe, _, submit = _bare(2, repair=2)
    try:
        _three_clean_chunks(pipe, submit)
        pipe.debug_shadow_xor(1, "rows1", 26, 0, 28, MASK)
        pipe.debug_shadow_xor(2, "rows1", 26, 0, 28, MASK2)
        submit(3)
        with pytest.raises(E.CmxError, match="no majority between 3 instances") as e:
            pipe.wait(3)
        assert "chunk 3" in str(e.value) and "mixer 26" in str(e.value) and "void" in str(e.value)
        assert pipe.shadow_repairs()["total"] == 0
        with pytest.raises(E.CmxError, match="void"):
            submit(4)
    finally:
        pipe.close()


def test_budget_used_up_stops_with_the_log():
    from cmix_amd import engine as E
    pipe, _, submit = _bare(2, repair=1)
    try:
        _three_clean_chunks(pipe, submit)
        pipe.debug_shadow_xor(1, "rows1", 26, 0, 28, MASK)
        submit(3)
        pipe.wait(3)
        assert pipe.shadow_repairs()["total"] == 1
        pipe.debug_shadow_xor(1, "rows1", 26, 0, 28, MASK)
        submit(4)
        with pytest.raises(E.CmxError, match="instance 1 is the odd one") as e:
            pipe.wait(4)
        msg = str(e.value)
        assert "chunk 4" in msg and "void" in msg and "1 repair(s) on the majority before it" in msg and "stream bit %d" % (8 * 4 * N_CHUNK) in msg
        assert pipe.shadow_repairs()["total"] == 1
    finally:
        pipe.close()


def test_refusals():
    from cmix_amd import engine as E

    def before(pipe):
        with pytest.raises(E.CmxError, match="needs 2 shadow"):
            pipe.set_shadow_repair(1)
        pipe.set_shadow(1)
        with pytest.raises(E.CmxError, match="needs 2 shadow"):
            pipe.set_shadow_repair(1)
        pipe.set_shadow_repair(0)      # off is always allowed
        pipe.set_shadow(2)
        with pytest.raises(E.CmxError, match="max_repairs"):
            pipe.set_shadow_repair(-1)
    pipe, _, submit = _bare(2, before=before)
    try:
        submit(0)
        pipe.wait(0)
        with pytest.raises(E.CmxError, match="before the first chunk"):
            pipe.set_shadow_repair(1)
    finally:
        pipe.close()


def test_verify_shadow_and_repair_combine(unperturbed):
    """Layer-0 mixer 8 is keyed by the zero context: every chunk reloads its row 0. One of that row's extra weights (not covered by a digest) is
    changed in the verifying instance: from then on it stores row 0 with digests of what IT computed. The repair rewrites the row's digested words;
    the next reload raises verify mode's row-segment alarm unless the stored digests were recomputed."""
    pipe, p, submit = _bare(2, repair=2, verify=True)
    try:
        _three_clean_chunks(pipe, submit)
        pipe.debug_shadow_xor(0, "rows0", 8, 0, 2080, MASK)
        for i in (3, 4, 5):
            submit(i)
        for i in (3, 4, 5):
            pipe.wait(i)
        rep = pipe.shadow_repairs()
        assert rep["total"] == 1
        e = rep["log"][0]
        assert (e["chunk"], e["column"], e["odd"]) == (3, 8, 0) and e["layer0_mask"] & ((1 << 9) - 1) == 1 << 8
        assert e["first"]["region"] == 0 and e["words"] > 2078   # the row's digested weights were among the repaired words
        submit(6)
        pipe.wait(6)
        pipe.sync()
        v = pipe.verify_report()
        assert v["mismatches"] == 0 and v["chunks"] == N_CHUNKS
        assert bits_equal(p.cpu().numpy(), unperturbed).all()
        assert pipe.shadow_state_diff(0, 1)["words"] == 0 and pipe.shadow_state_diff(1, 2)["words"] == 0
    finally:
        pipe.close()


# ---- the whole engine --------------------------------------------------------------------------------------------------------

def _golden_64k():
    with np.load(os.path.join(GOLDEN, "dropin_64k.npz")) as z:
        return z["sha256"].tobytes(), int(z["size"][0]), int(z["seed"][0]), int(z["seed"][1])


def _engine_run(repair):
    from cmix_amd import synth as S
    from cmix_amd.pipeline import EngineStream, text_file_stream
    _, _, n, seed = _golden_64k()
    stream = text_file_stream(S.enwik_like(n, seed))
    eng = EngineStream(0, stream, 4096, shadow=2, repair=repair)
    try:
        eng.feed(5 * 4096)
        eng.pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, MASK)   # mid-stream, in the stream's own network
        eng.feed(len(stream))
        return eng.finish(), eng.pipe.shadow_repairs()
    finally:
        eng.close()


def test_engine_stream_64k_repairs_an_event_and_writes_the_reference_file():
    want_sha, want_size, _, _ = _golden_64k()
    got, rep = _engine_run(4)
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
    assert rep["total"] == 1 and (rep["log"][0]["chunk"], rep["log"][0]["odd"], rep["log"][0]["column"]) == (5, 0, 26)


def test_engine_stream_64k_without_repair_fails_as_before():
    from cmix_amd import engine as E
    with pytest.raises(E.CmxError, match="instance 0 is the odd one"):
        _engine_run(0)


def test_predictor_debug_shadow_xor_is_repaired_behind_predict():
    """the C ABI's look-ahead mode (cmx_set_shadow_repair, cmx_debug_shadow_xor): three chunks of 4096 bytes, an event armed between chunks 0 and 1"""
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    data = S.enwik_like(3 * 4096, 33)
    vocab = np.zeros(256, np.uint8)
    vocab[np.unique(np.frombuffer(data, np.uint8))] = 1

    def walk(shadow):
        pr = E.Predictor(vocab, 0)
        try:
            if shadow:
                with pytest.raises(E.CmxError, match="needs 2 shadow"):
                    pr.set_shadow_repair(2)
                pr.set_shadow(2)
                pr.set_shadow_repair(2)
                pr.debug_shadow_xor(0, 0, "rows1", 26, 0, 28, MASK)
            pr.stage_input(data)
            out = np.empty(8 * len(data), np.float32)
            t = 0
            for byte in data:
                for j in range(7, -1, -1):
                    out[t] = pr.Predict()
                    pr.Perceive((byte >> j) & 1)
                    t += 1
            return out, pr.shadow_repairs()
        finally:
            pr.close()
    want, none = walk(False)
    assert none == {"total": 0, "log": []}
    got, rep = walk(True)
    assert bits_equal(got, want).all()
    assert rep["total"] == 1 and (rep["log"][0]["chunk"], rep["log"][0]["bit"], rep["log"][0]["odd"]) == (1, 8 * 4096, 0)


def test_dropin_program_with_repair_armed_and_no_event_prints_no_repair_line():
    from cmix_amd import synth as S
    exe = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    want_sha, want_size, n, seed = _golden_64k()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(S.enwik_like(n, seed))
        r = subprocess.run([exe, "-c", src, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                           env=dict(os.environ, CMIX_SHADOW="2", CMIX_SHADOW_REPAIR="2"))
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
        got = open(out, "rb").read()
        assert b"repair" not in r.stderr
    assert len(got) == want_size and hashlib.sha256(got).digest() == want_sha
