"""GPU: every stage kernel against poisoned LDS between launches.

On a quiet device the previous occupant of a compute unit is the same kernel's previous launch, so an LDS word a kernel reads before it has
written it holds what that launch left there -- usually the right value or a harmless one -- and no parity test notices. Here the LDS of
EVERY compute unit is overwritten with a pattern (cmx_probe_lds_fill, E.lds_fill) before a stage's handle is created and before each of its
run() / submit() calls -- one such call may launch several kernels in a row (the LSTM's forward, BPTT and Adam kernels; paq8's media kernels one
after the other; a pipeline chunk's stages): LDS handed from one kernel to the next INSIDE a call still sees the quiet-device predecessor, only
what a call finds when it begins is controlled -- and each case runs four times: clean (no fill), 0xFFFFFFFF (a NaN as f32, -1 as an integer, every flag / tag / index bit set),
0xA5A5A5A5 (non-trivial bytes, int16 values and indices; -2.9e-16 as f32, which could hide in a sum: hence the NaN pattern as well) and
0x00000000 (what a fresh device tends to hold). The four runs must agree in every output word and the clean one must equal the case's
reference -- oracle or trace of the unmodified reference, compared as the stage's own parity test compares -- because a clean run that reads
stale LDS can itself be the wrong one. A fill that did not reach every compute unit FAILS the case (a pass would prove less than it claims).
All shapes are ones the suite already uses, but for one: the LSTM at V = 62 (tests/golden/lstm_vocab_sweep.npz), where the gate workgroup's LDS
holds a trailing partial quad and the output workgroups a partial last row -- words no other LSTM case here has. The host twins (what models
LDS in tests/host/*_emul.cpp, poisoned at every run) are the test_poisoned_lds_* cases of tests/test_*_host.py."""
import numpy as np
import pytest

from conftest import bits_equal, load_golden, synth_mixnet_inputs
import make_golden as mg

pytestmark = pytest.mark.gpu

PATTERNS = [None, 0xFFFFFFFF, 0xA5A5A5A5, 0x00000000]   # None: the clean run


class _Fill:
    """fill() overwrites every compute unit's LDS with the run's pattern (nothing in the clean run) and fails unless the fill was complete"""

    def __init__(self):
        self.pattern, self.calls = None, 0

    def __call__(self):
        if self.pattern is None:
            return
        from cmix_amd import engine as E
        r = E.lds_fill(self.pattern)
        assert r["full"] and r["workgroups"] >= r["compute_units"] > 0, "LDS fill 0x%08X did not cover the device: %r" % (self.pattern, r)
        self.calls += 1


@pytest.fixture
def fill():
    return _Fill()


def _before_every(monkeypatch, cls, method, fill):
    """every cls.method call (one run / submit of the stage: one kernel launch for the mixing network, the context models and fxcm, several in
    a row for the LSTM, paq8 and the pipeline) is preceded by a fill: the probe synchronises the device first, so the stage's previous call
    has finished, and synchronises after, so the fill is complete when the call's first kernel is submitted"""
    orig = getattr(cls, method)

    def wrapped(self, *a, **k):
        fill()
        return orig(self, *a, **k)
    monkeypatch.setattr(cls, method, wrapped)


def _words(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _four_runs(fill, run, check, min_fills=2):
    """run() -> tuple of arrays, once per pattern with a fill before the handle exists (creation launches init kernels) and whatever fills the
    case places between launches; check(outputs of the clean run) asserts the case's reference"""
    outs = []
    for pat in PATTERNS:
        fill.pattern, fill.calls = pat, 0
        fill()
        outs.append(tuple(run()))
        assert pat is None or fill.calls >= min_fills, (pat, fill.calls)
    check(*outs[0])
    for pat, o in zip(PATTERNS[1:], outs[1:]):
        assert len(o) == len(outs[0])
        for k, (a, b) in enumerate(zip(outs[0], o)):
            wa, wb = _words(a), _words(b)
            assert wa.shape == wb.shape, (k, a.shape, b.shape)
            bad = np.flatnonzero(wa != wb)
            assert bad.size == 0, "LDS pattern 0x%08X: output %d differs from the clean run in %d bytes, first at byte %d (element %d of shape %r)" % (
                pat, k, bad.size, bad[0], bad[0] // np.asarray(a).itemsize, np.asarray(a).shape)


def test_fill_covers_every_compute_unit():
    """the probe itself: every workgroup saw all the others resident (two do not fit one compute unit's LDS, so they sat on all of them); its
    numbers and the wall time of a call are printed for profiles/"""
    import time
    from cmix_amd import engine as E
    E.lds_fill(0)
    t0 = time.perf_counter()
    r = [E.lds_fill(p) for p in (0xFFFFFFFF, 0xA5A5A5A5, 0)]
    ms = (time.perf_counter() - t0) * 1000 / 3
    print("cmx_probe_lds_fill:", r[0], "%.3f ms per call" % ms)
    for x in r:
        assert x["full"] and x["resident"] == x["workgroups"] and x["uncovered_bytes_per_cu"] == 0, x
        assert x["workgroups"] % x["compute_units"] == 0 and x["bytes_per_workgroup"] * (x["workgroups"] // x["compute_units"]) == x["bytes_per_cu"], x
        assert 1 <= x["launches"] <= 8


# ---- the mixing network --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixnet_case():
    """3000 bits with few distinct contexts (rows pass 1024 steps: the decay path) and the oracle's final probabilities"""
    from oracle import oracle as O
    probs, sel, bits = synth_mixnet_inputs(3000, seed=11, n_ctx_bits=1)
    return probs, sel, bits, O.MixNet().run(probs, sel, bits)


def test_mixnet_chunk_kernel(monkeypatch, fill, mixnet_case):
    """cmx_mixnet_spec_kernel (27 workgroups, the main one holds 144 KB of LDS): launches cut at bits 1, 9, 700, 1500"""
    from cmix_amd import engine as E
    from test_gpu_mixnet import _gpu_run
    probs, sel, bits, ref = mixnet_case
    _before_every(monkeypatch, E.MixNet, "run", fill)

    def check(p, mix):
        bad = np.nonzero(~bits_equal(p, ref))[0]
        assert len(bad) == 0, f"clean run != oracle, first at bit {bad[0]}"
    _four_runs(fill, lambda: _gpu_run(probs, sel, bits, chunks=[1, 9, 700, 1500]), check, min_fills=6)


def test_mixnet_chunk_kernel_verify_mode(monkeypatch, fill, mixnet_case):
    """cmx_mixnet_spec_verify_kernel + the digest fold kernels: the first 1024 bits, launches cut at 1 and 512; the verify report stays clean"""
    from cmix_amd import engine as E
    from test_gpu_verify import _stage
    probs, sel, bits, ref = mixnet_case
    T = 1024
    _before_every(monkeypatch, E.MixNet, "run", fill)

    def run():
        (p, mix), rep = _stage(probs[:T], sel[:T], bits[:T], [0, 1, 512, T], True)
        assert rep == {"chunks": 3, "bits": T, "mismatches": 0, "cls": None, "first_bit": None, "mixer": None, "row": None, "segment": None}, (fill.pattern, rep)
        return p, mix

    def check(p, mix):
        bad = np.nonzero(~bits_equal(p, ref[:T]))[0]
        assert len(bad) == 0, f"clean run != oracle, first at bit {bad[0]}"
    _four_runs(fill, run, check, min_fills=4)


def test_mixnet_bit_synchronous_kernel(fill):
    """cmx_mixnet_kernel (predict / perceive, one bit at a time): 200 bits of text_96, a fill every 50 bits -- and, 25 bits after each, one
    between a bit's predict and its perceive"""
    from cmix_amd import engine as E
    g = load_golden("text_96")
    probs = mg.unpack_probs(g)
    sel32 = (g["sel"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    T = 200

    def run():
        net = E.MixNet(0)
        out = np.empty(T, np.float32)
        for t in range(T):
            if t % 50 == 0:
                fill()
            out[t] = net.predict(probs[t], sel32[t])
            if t % 50 == 25:
                fill()   # predict and perceive are two launches of the kernel: nothing may pass from one to the other through LDS
            net.perceive(int(g["bits"][t]))
        net.close()
        return (out,)

    def check(out):
        assert bits_equal(out, g["p_final"][:T]).all()
    _four_runs(fill, run, check, min_fills=9)


def test_shadow_vote_two_chunks(monkeypatch, fill):
    """Pipeline.set_shadow(2) over two chunks (three network instances + the vote kernel of mixnet_vote.hip), a fill between the chunks: the
    instances agree on every word, and p is what the pipeline gives without shadows"""
    from cmix_amd import engine as E
    from test_gpu_shadow import N_CHUNK, _bare
    pipe, p_off, _ = _bare(0, 2)
    try:
        pipe.sync()
        want = p_off.cpu().numpy()[:8 * 2 * N_CHUNK]
    finally:
        pipe.close()
    _before_every(monkeypatch, E.Pipeline, "submit", fill)   # (_bare waits for chunk i before it submits chunk i + 1)

    def run():
        pipe, p, _ = _bare(2, 2)
        try:
            pipe.sync()
            assert pipe.shadow_report()["raw"] == [2, 8 * 2 * N_CHUNK, 3, 0, 0, 0, 0, 0], (fill.pattern, pipe.shadow_report())
            assert pipe.shadow_state_diff(0, 1)["words"] == 0 and pipe.shadow_state_diff(1, 2)["words"] == 0
            return (p.cpu().numpy()[:8 * 2 * N_CHUNK],)
        finally:
            pipe.close()

    def check(p):
        assert bits_equal(p, want).all()
    _four_runs(fill, run, check, min_fills=3)


# ---- the LSTM ------------------------------------------------------------------------------------------------------------------

def test_lstm_across_two_bptt_rounds(monkeypatch, fill):
    """forward / BPTT block kernels + lstm_kernels.hip: 230 bytes of text_2k_nofull in chunks cut at 1, 2, 99, 100, 101, 199, 205 (BPTT + Adam
    at bytes 100 and 200) against the reference's 256-way distributions; the bit predictions and the arg-max symbols take part in the
    four-way comparison"""
    from cmix_amd import engine as E
    from test_gpu_lstm import _run_gpu
    g = load_golden("text_2k_nofull")
    N = 230
    _before_every(monkeypatch, E.Lstm, "run", fill)

    def check(out, bp, bx):
        bad = np.nonzero(~bits_equal(out, g["lstm_probs"][1:N + 1]).all(axis=1))[0]
        assert len(bad) == 0, f"LSTM distribution differs first after byte {bad[0]}"
        if "probs_q" in g:   # (as tests/test_gpu_lstm.py: the trace's LSTM column where the fixture holds the columns)
            want = mg.unpack_probs(g)[:8 * N, 2077].reshape(N, 8)
            badb = np.argwhere(~bits_equal(bp, want))
            assert len(badb) == 0, f"bit prediction differs first at (byte, bit) {badb[0]}"
    _four_runs(fill, lambda: _run_gpu(g["vocab"], g["ppmd_probs"][1:N + 1], g["stream"][:N], [1, 2, 99, 100, 101, 199, 205]), check, min_fills=9)


def test_lstm_small_vocabulary(monkeypatch, fill):
    """V = 3 (ragged rows, tiny softmax), 130 bytes cut at 1, 100, 101, against the oracle"""
    from cmix_amd import engine as E
    from oracle import oracle as O
    from test_gpu_lstm import _run_gpu
    rng = np.random.default_rng(2)
    vocab = np.zeros(256, np.uint8)
    vocab[[10, 65, 200]] = 1
    N = 130
    data = rng.choice([10, 65, 200], N).astype(np.uint8)
    probs = np.zeros((N, 256), np.float32)
    probs[:, [10, 65, 200]] = rng.dirichlet([1, 1, 1], N).astype(np.float32)
    orc = O.Lstm(vocab)
    want, wantb = [], []
    for n in range(N):
        for j in range(7, -1, -1):
            wantb.append(orc.bit_predict())
            orc.bit_perceive((int(data[n]) >> j) & 1)
        want.append(orc.byte_update(probs[n], data[n]))
    _before_every(monkeypatch, E.Lstm, "run", fill)

    def check(out, bp, bx):
        assert bits_equal(out, np.array(want)).all()
        assert bits_equal(bp.reshape(-1), np.array(wantb, np.float32)).all()
    _four_runs(fill, lambda: _run_gpu(vocab, probs, data, [1, 100, 101]), check, min_fills=5)


def test_lstm_vocabulary_62(monkeypatch, fill):
    """V = 62 ((V + 1) % 4 == 3: the gate rows end in a partial quad; seven output workgroups of 8 rows and one of 6), the 230 bytes of the
    vocabulary sweep cut at 1, 100, 101, against the reference's distributions, bit predictions and arg-max symbols"""
    from cmix_amd import engine as E
    from test_gpu_lstm import _run_gpu
    import make_lstm_vocab as mk
    c = mk.load_sweep()[62]
    _before_every(monkeypatch, E.Lstm, "run", fill)

    def check(out, bp, bx):
        bad = np.nonzero(~bits_equal(out, c["lstm"]).all(axis=1))[0]
        assert len(bad) == 0, f"LSTM distribution differs first after byte {bad[0]}"
        badb = np.argwhere(~bits_equal(bp, c["bitp"]))
        assert len(badb) == 0, f"bit prediction differs first at (byte, bit) {badb[0]}"
        assert (bx == c["ex"]).all()
    _four_runs(fill, lambda: _run_gpu(c["vocab"], c["ppmd"], c["stream"], [1, 100, 101]), check, min_fills=5)


# ---- contexts + small models ---------------------------------------------------------------------------------------------------

def test_ctxmodels_brackets_1k_ragged_chunks(monkeypatch, fill):
    """cmx_ctxmodels_kernel on brackets_1k in chunks cut at 1, 2, 9, 100, 101, 640: model outputs, selectors, manager registers and contexts
    at every chunk end against the reference's trace"""
    from cmix_amd import engine as E
    from test_gpu_ctxmodels import COLS, _run_gpu
    g = load_golden("brackets_1k")
    stream = g["stream"]
    _before_every(monkeypatch, E.CtxModels, "run", fill)

    def run():
        p, s, mgr = _run_gpu(g["vocab"], stream, [1, 2, 9, 100, 101, 640], want_mgr=True)
        flat = []
        for n, (regs, ctx, bctx) in mgr:
            flat += [np.asarray(regs), np.asarray(ctx), np.asarray(bctx)]
        return [p, s] + flat

    def check(p, s, *flat):
        want_p = mg.unpack_probs(g)[:, COLS] if "probs_q" in g else g["small_probs"][:, :54]
        bad = np.argwhere(~bits_equal(p, want_p))
        assert len(bad) == 0, f"model {bad[0][1]} (col {COLS[bad[0][1]]}) differs first at bit {bad[0][0]}"
        want_s = (g["sel"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        want_s[:, 12] = 0
        bad = np.argwhere(s != want_s)
        assert len(bad) == 0, f"selector {bad[0][1]} differs first at bit {bad[0][0]}"
        ends = [1, 2, 9, 100, 101, 640, len(stream)]
        assert len(flat) == 3 * len(ends)
        for i, n in enumerate(ends):
            regs, ctx, bctx = flat[3 * i:3 * i + 3]
            want = g["regs"][n].copy()
            want[6] = 0
            assert (regs == want).all(), f"manager registers after byte {n}: {regs} vs {want}"
            assert (ctx == g["ctx"][n]).all(), f"contexts after byte {n}"
            if n < len(stream):
                assert (bctx == g["bitctx"][8 * n]).all(), f"bit contexts after byte {n}"
    _four_runs(fill, run, check, min_fills=8)


# ---- fxcm ----------------------------------------------------------------------------------------------------------------------

def test_fxcm_role_kernels_ragged_chunks(monkeypatch, fill):
    """cmx_fxcm_roles_kernel (roles M, U, X: FxShared + FxLocal + the roles' own LDS): 2500 bytes of enwik-like text in chunks
    1, 1, 7, 100, 1000, 3, 2000 against the oracle's 431 values per bit"""
    from cmix_amd import engine as E
    from test_fxcm_stage_host import _poison_case, compare
    from test_zgpu_stage_fxcm import run_device
    data, pr, ex, want = _poison_case()
    _before_every(monkeypatch, E.Fxcm, "run", fill)
    _four_runs(fill, lambda: (run_device(data, pr, ex, [1, 1, 7, 100, 1000, 3, 2000]),), lambda got: compare(got, want, "clean run"), min_fills=8)


# ---- paq8 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["text_96", "binary_64"])
def test_paq8_role_kernels_golden_columns(monkeypatch, fill, name):
    """the role kernels of a chunk without media (ContextMap2 x 3, the ContextMap family, the lanes, the DMC forest, the mixer's main and helper
    workgroups): chunks 1, 1, 7, 30 against columns 434..2024 of the reference's trace"""
    from cmix_amd import engine as E
    from test_zgpu_p8stage import run_device
    g = load_golden(name)
    want = np.ascontiguousarray(mg.unpack_probs(g)[:, 434:2025])
    _before_every(monkeypatch, E.P8Stage, "run", fill)

    def check(got):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, "first mismatch (step, column):", bad[0], got[tuple(bad[0])] * 4095, want[tuple(bad[0])] * 4095)
    _four_runs(fill, lambda: (run_device(g["stream"], [1, 1, 7, 30]),), check, min_fills=5)


@pytest.mark.parametrize("name", ["pgm8_4k", "jpeg_rst_raw_3k", "wav8m_2k"])
def test_paq8_media_kernels_vs_reference_hashes(monkeypatch, fill, name):
    """the plain kernels of the models with tables of their own (cmx_p8s_xfam_kernel / _xlanes_ / _xmix_) and the hand-over kernels between them
    and the generic ones: an 8-bit image, the smallest JPEG and the smallest audio fixture, in chunks of 1024, 1, 700, 333, ..."""
    from cmix_amd import engine as E
    from make_paq8_hashes import row_hash
    from test_p8stage_host import load_hashes
    from test_zgpu_p8stage import run_device
    stream, want = load_hashes(name)
    _before_every(monkeypatch, E.P8Stage, "run", fill)

    def check(got):
        bad = np.nonzero(row_hash(got) != want)[0]
        assert bad.size == 0, (name, "first differing step:", bad[0], "of", len(want))
    _four_runs(fill, lambda: (run_device(stream, [1024, 1, 700, 333]),), check, min_fills=4)


# ---- every stage at once -------------------------------------------------------------------------------------------------------

def test_whole_pipeline_every_stage_stream(fill):
    """the engine's chunk pipeline with fxcm and paq8 enabled (every stage kernel on its own stream, overlapping within a chunk) on text_96 in
    ragged chunks, a fill after each chunk's wait + sync: all 2078 layer-0 inputs and the final probability against the reference's trace"""
    import torch
    from cmix_amd import engine as E
    g = load_golden("text_96")
    stream = np.ascontiguousarray(g["stream"])
    n = len(stream)
    ref = np.ascontiguousarray(mg.unpack_probs(g), np.float32)
    edges = sorted(set([0, n, 1, 2, 3, 10, 11, 50, 51]))

    def run():   # tests/test_gpu_pipeline.py::_native, restated: fxcm + paq8 on, all 2078 columns computed (from -1), a fill after each chunk's wait + sync -- keep the two in step
        pipe = E.Pipeline(g["vocab"], 0, n)
        try:
            pipe.enable_fxcm(None)
            pipe.enable_paq8()
            l0 = torch.full((8 * n, E.N_INPUTS), -1.0, dtype=torch.float32, device="cuda")
            pf = torch.full((8 * n,), -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                pipe.submit(stream[a:b].tobytes(), l0[8 * a:8 * b], pf[8 * a:8 * b])
                pipe.wait(i)
                pipe.sync()
                fill()
            return l0.cpu().numpy(), pf.cpu().numpy()
        finally:
            pipe.close()

    def check(l0, pf):
        bad = np.argwhere(~bits_equal(l0, ref))
        assert len(bad) == 0, f"layer-0 input {bad[0][1]} differs first at bit {bad[0][0]}"
        bad = np.nonzero(~bits_equal(pf, g["p_final"]))[0]
        assert len(bad) == 0, f"final probability differs first at bit {bad[0]} of {8 * n}"
    _four_runs(fill, run, check, min_fills=len(edges))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_decoders_late_kernels_first_launch(pattern):
    """The decoder's form of every stage (the late kernels: resident from late_start to late_stop, fed bit by bit by the host) on text_96, every
    layer-0 input, selector and final probability of every bit against the reference's trace, with ONE fill immediately before late_start. No
    fill is possible while the patient kernels are resident -- the probe synchronises the device, which would wait for kernels that wait
    for the host -- so the late kernels are covered at their first launch only. Each pattern is a fresh process (as tests/test_gpu_late.py
    starts its children); all four equal the trace, hence each other."""
    from conftest import GOLDEN, ROOT
    from test_gpu_late import _CHILD, _run_child
    code = _CHILD.format(root=ROOT, golden=GOLDEN, name="text_96", rows=True)
    start = "pipe.late_start(last)\n"
    assert code.count(start) == 1
    if pattern is not None:
        code = code.replace(start, "_r = E.lds_fill(%d)\nassert _r['full'], 'LDS fill did not cover the device: %%r' %% (_r,)\nprint('lds_fill', _r)\n" % pattern + start)
    out = _run_child(code)
    assert out.count("OK bits") == 1 and (pattern is None) == ("lds_fill" not in out)
