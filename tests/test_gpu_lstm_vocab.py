"""GPU parity: the HIP LSTM stage across vocabulary sizes against the unmodified reference (tests/golden/lstm_vocab_sweep.npz,
tests/golden/make_lstm_vocab.py: the table of what each V exercises is there) and, for the gate weights, element by element against the oracle,
which tests/test_oracle_lstm_vocab.py pins to the same fixture -- the weights' digests included -- on the CPU. Every size of the stage follows
from V: row lengths, the transposed weight layout, the LDS carve-up of the forward block, the grid of the update kernels, head and tail of
every ordered chain. Bit-exact on every float, except where the tolerance-mode case says otherwise."""
import functools
import hashlib

import numpy as np
import pytest

from conftest import bits_equal
import make_lstm_vocab as mk
from test_oracle_lstm_vocab import oracle_run

pytestmark = pytest.mark.gpu

CHUNKS = [1, 2, 99, 100, 101, 199, 205]


@pytest.fixture(scope="module")
def sweep():
    return mk.load_sweep()


@functools.lru_cache(maxsize=None)
def _oracle_weights(V, nbytes):
    return oracle_run(mk.load_sweep()[V], nbytes)[3]


def _run(c, nbytes, chunks=None, tolerance=False):
    """-> (dist [n,256], bitp [n,8], ex [n,8], six gate matrices, cmx_lstm_failed)"""
    import torch
    from cmix_amd import engine as E
    l = E.Lstm(c["vocab"], 0)
    if tolerance:
        l.set_tolerance(True)
    d_in = torch.from_numpy(np.ascontiguousarray(c["ppmd"][:nbytes], np.float32)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(c["stream"][:nbytes], np.uint8)).cuda()
    edges = sorted(set([0, nbytes] + [x for x in (chunks or []) if x < nbytes]))
    outs, bps, bxs = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        o, bp, bx = l.run(d_in[a:b], d_b[a:b])
        outs.append(o); bps.append(bp); bxs.append(bx)
    torch.cuda.synchronize()
    res = (torch.cat(outs).cpu().numpy(), torch.cat(bps).cpu().numpy(), torch.cat(bxs).cpu().numpy())
    w = [l.gate_weights(layer, gate) for layer in range(2) for gate in range(3)]
    failed = E.lib().cmx_lstm_failed(l.h)
    l.close()
    return res + (w, failed)


def _column_kind(c, V, rowlen):
    return "one-hot" if c < V else "symbol input" if c < 2 * V else "recurrent" if c < rowlen - 1 else "bias"


def _check_outputs(V, c, what, out, bp, bx):
    bad = np.nonzero(~bits_equal(out, c["lstm"]).all(axis=1))[0]
    assert len(bad) == 0, f"V = {V}, {what}: LSTM distribution differs from the reference's first after byte {bad[0]}"
    badb = np.argwhere(~bits_equal(bp, c["bitp"]))
    assert len(badb) == 0, f"V = {V}, {what}: bit prediction differs first at (byte, bit) {badb[0]}"
    bade = np.argwhere(bx.astype(np.int64) != c["ex"])
    assert len(bade) == 0, f"V = {V}, {what}: ex differs first at (byte, bit) {bade[0]}"


def _check_weights(V, what, got, want, cols=None):
    """element-wise and bit-exact; cols: compare these columns only"""
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == (200, (201 if i < 3 else 401) + 2 * V)
        ne = ~bits_equal(a, b)
        if cols is not None:
            ne = ne[:, cols]
        bad = np.argwhere(ne)
        if len(bad):
            r, cc = bad[0]
            col = int(cc if cols is None else np.arange(a.shape[1])[cols][cc])
            raise AssertionError(f"V = {V}, {what}: gate weights of layer {i // 3}, gate {i % 3} differ in {len(bad)} elements, first at (row, column) "
                                 f"({r}, {col}), a {_column_kind(col, V, a.shape[1])} column: {a[r, col]!r} vs {b[r, col]!r}")


@pytest.mark.parametrize("V", mk.VOCABS)
def test_vocabulary_vs_reference(sweep, V):
    """230 bytes (BPTT + Adam at bytes 0, 100, 200) in one piece and cut at 1, 2, 99, 100, 101, 199, 205: distributions, bit predictions and
    `ex` against the reference; the six gate matrices after the run against the oracle's and against the reference's digests"""
    c = sweep[V]
    want_w = _oracle_weights(V, mk.N)
    for what, chunks in (("one run", None), ("ragged chunks", CHUNKS)):
        out, bp, bx, w, failed = _run(c, mk.N, chunks)
        assert failed == 0, f"V = {V}, {what}: cmx_lstm_failed"
        _check_outputs(V, c, what, out, bp, bx)
        _check_weights(V, what, w, want_w)
        for i, m in enumerate(w):
            assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == c["wsha"][i], (V, what, i)


@pytest.mark.parametrize("V", [9, 62])
def test_tolerance_mode_after_one_real_round(sweep, V):
    """TOLERANCE mode (cmx_lstm_bptt_acc_mfma; NOT bit-exact) where the one-hot / dense split c < V falls inside a 16-column tile: 101 bytes,
    strict and tolerant. The round at byte 0 sees all-zero caches and changes nothing, so the round at byte 100 sees the same error signals
    in both modes; the MFMA kernel keeps the reference's order for the one-hot columns. Hence (derived, not measured): columns c < V of all
    six matrices are bit-identical between the modes and equal to the oracle's, and so are the outputs of bytes 0..99. The dense columns must
    differ somewhere (the mode is on) and stay within the bound of test_gpu_lstm.py::test_tolerance_mode_mfma_weight_update_deviation, 2e-5 of
    max |w| -- measured there at V = 256 after five rounds. Measured here on the MI355X after the one round (profiles/r15_lstm_vocab_sweep.txt):
    V = 9: 1.03e-7, V = 62: 1.13e-6."""
    c = sweep[V]
    N = 101
    s_out, s_bp, s_bx, s_w, s_failed = _run(c, N)
    t_out, t_bp, t_bx, t_w, t_failed = _run(c, N, tolerance=True)
    assert s_failed == 0 and t_failed == 0
    onehot = np.arange(V)
    want_w = _oracle_weights(V, N)
    _check_weights(V, "strict, 101 bytes", s_w, want_w)
    _check_weights(V, "tolerance mode, one-hot columns vs the oracle", t_w, want_w, cols=onehot)
    _check_weights(V, "tolerance mode, one-hot columns vs strict mode", t_w, s_w, cols=onehot)
    bad = np.nonzero(~bits_equal(s_out[:100], t_out[:100]).all(axis=1))[0]
    assert len(bad) == 0, f"V = {V}: tolerance mode changes the distribution after byte {bad[0]}, before the first real round"
    assert bits_equal(s_bp[:100], t_bp[:100]).all() and (s_bx[:100] == t_bx[:100]).all()
    bad = np.nonzero(~bits_equal(s_out[:100], c["lstm"][:100]).all(axis=1))[0]
    assert len(bad) == 0, f"V = {V}: LSTM distribution differs from the reference's first after byte {bad[0]}"
    differ = sum(int((~bits_equal(a[:, V:], b[:, V:])).sum()) for a, b in zip(s_w, t_w))
    dw = max(float(np.abs(a[:, V:].astype(np.float64) - b[:, V:]).max() / np.abs(a).max()) for a, b in zip(s_w, t_w))
    line = "LSTM tolerance mode, V = %d, after the one real BPTT round (byte 100): %d dense weights differ, max deviation %.3g of max |w|" % (V, differ, dw)
    print(line)
    assert differ > 0, "tolerance mode left every dense weight bit-identical: is it on?"
    assert dw < 2e-5


def _bytemodel_model(dists, data, reverse=False):
    """byte-model.cpp:8-24 in ordered float32 adds: the upper half of the interval first, then the lower half added onto it
    (reverse: every run of adds from its other end -- NOT the reference's order, to show that the order matters for a case)"""
    p = np.empty((len(data), 8), np.float32)
    for n, byte in enumerate(data):
        pr = dists[n]
        top, bot = 255, 0
        for k in range(8):
            mid = bot + (top - bot) // 2
            num = np.float32(0)
            for i in (range(top, mid, -1) if reverse else range(mid + 1, top + 1)):
                num = np.float32(num + pr[i])
            den = num
            for i in (range(mid, bot - 1, -1) if reverse else range(bot, mid + 1)):
                den = np.float32(den + pr[i])
            p[n, k] = np.float32(0.5) if den == 0 else np.float32(num / den)
            if (int(byte) >> (7 - k)) & 1:
                bot = mid + 1
            else:
                top = mid
    return p


def test_bytemodel_bits_crafted_distributions():
    """E.bytemodel_bits (cmx_bytemodel_bits without an `ex` buffer) on 16 crafted bytes, all 8 bit depths of each: distributions that are zero on
    the whole interval of the coded byte (denom == 0 -> 0.5, which no vocabulary-respecting LSTM output reaches), a single non-zero symbol,
    sums whose float32 value depends on the order of the adds (1e-8 mixed with 0.5), and seeded noise"""
    import torch
    from cmix_amd import engine as E
    rng = np.random.default_rng(11)
    N = 16
    d = np.zeros((N, 256), np.float32)
    data = np.zeros(N, np.uint8)
    d[0, 128:] = rng.random(128, dtype=np.float32); data[0] = 3          # zero from bit 1 on
    data[1] = 0xC7                                                       # all zero: 0.5 at every depth
    d[2, 77] = 1.0; data[2] = 77                                         # a single symbol, coded
    d[3, 77] = 1.0; data[3] = 79                                         # ... another byte coded: zero interval at the last bit
    d[4, 255] = 0.25; data[4] = 255
    d[5, 0] = 0.25; data[5] = 0
    d[6, :] = 1e-8; d[6, [0, 255]] = 0.5; data[6] = 0x55                 # 0.5 first, then 1e-8s that vanish; and the other way round
    d[7, :] = 1e-8; d[7, [127, 128]] = 0.5; data[7] = 0x80
    d[8, :] = 1e-8; d[8, ::37] = 0.5; data[8] = 0xAA
    d[9, :] = 1e-8; d[9, 200] = 0.5; d[9, 13] = 0.5; data[9] = 13
    d[10, :] = np.where(rng.random(256) < 0.5, 1e-8, 0.5); data[10] = 0x7F
    d[11, :] = np.where(rng.random(256) < 0.9, 1e-8, 0.5); data[11] = 0xFE
    d[12] = rng.dirichlet(np.ones(256)).astype(np.float32); data[12] = 0x01
    d[13] = rng.dirichlet(np.full(256, 0.05)).astype(np.float32); data[13] = int(np.argmax(d[13]))
    d[14, 100:104] = [0.5, 1e-8, 1e-8, 0.5]; data[14] = 101
    d[15, 3] = 1e-30; data[15] = 2                                       # a tiny but non-zero denominator: not the 0.5 branch
    want = _bytemodel_model(d, data)
    other_order = _bytemodel_model(d, data, reverse=True)
    assert all((~bits_equal(want[n], other_order[n])).any() for n in (6, 7, 8, 9)), "the mixed cases do not depend on the order of the adds"
    assert (want[0, 1:] == 0.5).all() and (want[1] == 0.5).all() and want[3, 7] == 0.5 and want[15, 7] == 1.0
    dd = torch.from_numpy(d).cuda()
    layer0 = torch.full((8 * N, E.N_INPUTS), -1.0, dtype=torch.float32, device="cuda")
    E.bytemodel_bits(dd[0], dd[1:].contiguous(), torch.from_numpy(data).cuda(), layer0, 2076)
    torch.cuda.synchronize()
    got = layer0.cpu().numpy()
    bad = np.argwhere(~bits_equal(got[:, 2076].reshape(N, 8), want))
    assert len(bad) == 0, f"bit prediction differs first at (byte, bit) {bad[0]}: {got[:, 2076].reshape(N, 8)[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"
    other = np.delete(got, 2076, axis=1)
    assert (other == -1.0).all(), "cmx_bytemodel_bits wrote outside its column"
