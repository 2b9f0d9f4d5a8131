"""CPU: the oracle's LSTM byte mixer (oracle/lstm_oracle.c) against the unmodified reference across vocabulary sizes.

tests/golden/lstm_vocab_sweep.npz (tests/golden/make_lstm_vocab.py) holds, for fourteen vocabulary sizes between 1 and 255, what the reference's
LSTM byte mixer produced over 230 bytes: its distribution after every byte, its Predict value and `ex` at every bit, and digests of the six gate
weight matrices after the last byte (three BPTT + Adam rounds: bytes 0, 100, 200). The oracle, fed the same PPMd rows, must reproduce all of it
bit for bit: that is what makes it the per-element reference of tests/test_gpu_lstm_vocab.py at V != 256. A missing fixture FAILS."""
import hashlib

import numpy as np
import pytest

from conftest import bits_equal
import make_lstm_vocab as mk


@pytest.fixture(scope="module")
def sweep():
    return mk.load_sweep()


def oracle_run(c, nbytes=mk.N):
    """the oracle over the first nbytes of case c -> (dist [n,256], bitp [n,8], ex [n,8], the six gate matrices)"""
    from oracle import oracle as O
    orc = O.Lstm(c["vocab"])
    dist = np.empty((nbytes, 256), np.float32)
    bitp = np.empty((nbytes, 8), np.float32)
    ex = np.empty((nbytes, 8), np.int64)
    for n in range(nbytes):
        byte = int(c["stream"][n])
        for k in range(8):
            bitp[n, k] = orc.bit_predict()
            ex[n, k] = orc.ex()
            orc.bit_perceive((byte >> (7 - k)) & 1)
        dist[n] = orc.byte_update(c["ppmd"][n], byte)
    return dist, bitp, ex, [orc.gate_weights(layer, gate) for layer in range(2) for gate in range(3)]


def test_fixture_covers_every_class():
    mk.check_classes()
    sweep = mk.load_sweep()
    assert sorted(sweep) == sorted(mk.VOCABS)
    for V, c in sweep.items():
        assert int(c["vocab"].sum()) == V and c["stream"].shape == (mk.N,) and c["vocab"][c["stream"]].all()
        assert c["lstm"].shape == c["ppmd"].shape == (mk.N, 256) and c["bitp"].shape == c["ex"].shape == (mk.N, 8)
    assert sum(1 for c in sweep.values() if c["vocab"][0] and c["vocab"][255]) >= 3


@pytest.mark.parametrize("V", mk.VOCABS)
def test_oracle_matches_reference(sweep, V):
    c = sweep[V]
    dist, bitp, ex, w = oracle_run(c)
    bad = np.nonzero(~bits_equal(dist, c["lstm"]).all(axis=1))[0]
    assert len(bad) == 0, f"V = {V}: oracle's LSTM distribution differs from the reference's first after byte {bad[0]}"
    badb = np.argwhere(~bits_equal(bitp, c["bitp"]))
    assert len(badb) == 0, f"V = {V}: bit prediction differs first at (byte, bit) {badb[0]}"
    bade = np.argwhere(ex != c["ex"])
    assert len(bade) == 0, f"V = {V}: ex differs first at (byte, bit) {bade[0]}"
    for i, m in enumerate(w):
        assert m.shape == (200, (201 if i < 3 else 401) + 2 * V)
        assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == c["wsha"][i], \
            f"V = {V}: gate weights of layer {i // 3}, gate {i % 3} after byte {mk.N - 1} differ from the reference's"
