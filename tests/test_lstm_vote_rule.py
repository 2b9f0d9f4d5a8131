"""CPU: the LSTM-stage vote's rule (cmix_amd/lstmvote.py, the host twin and specification of cmx_lstmvote_run in cmix_amd/csrc/lstm_vote.hip) on
crafted arrays, the strided form of instance 0, and the plumbing of the shadow LSTM stages through the header, the bindings and EngineStream.
tests/test_gpu_lstm_shadow.py holds the kernel to this twin."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cmix_amd.lstmvote import COLS, NONE, LstmVoteTwin, bit_predictions, chunk_result, element_name, lstm_vote_reference


def _agree(n, N, seed=3):
    """n instances that agree: distributions [N, 256] f32, bit predictions [N, 8] f32, ex [N, 8] i32"""
    rng = np.random.default_rng(seed)
    d = rng.random((N, 256), dtype=np.float32)
    p = rng.random((N, 8), dtype=np.float32)
    x = rng.integers(0, 256, (N, 8)).astype(np.int32)
    return [d.copy() for _ in range(n)], [p.copy() for _ in range(n)], [x.copy() for _ in range(n)]


def _plant(ds, ps, xs, inst, b, c, mask=1):
    a = ds[inst] if c < 256 else ps[inst] if c < 264 else xs[inst]
    a.view(np.uint32)[b, c if c < 256 else (c - 256) % 8] ^= np.uint32(mask)


@pytest.mark.parametrize("n", [2, 3])
def test_agreeing_instances_leave_a_clean_record(n):
    ds, ps, xs = _agree(n, 37)
    rec, words = lstm_vote_reference(ds, ps, xs, 900)
    assert rec == [1, 37, n, 0, 0, 0, 0, 0] and words is None
    assert chunk_result(ds, ps, xs, 900) == [0, 0, 0, 0]
    assert COLS == 272


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("c", [0, 255, 256, 263, 264, 271])
def test_one_planted_word_is_found_with_its_element_and_instance(n, c):
    ds, ps, xs = _agree(n, 20)
    inst = n - 1
    _plant(ds, ps, xs, inst, 11, c)
    rec, words = lstm_vote_reference(ds, ps, xs, 1000)
    assert rec == [1, 20, n, 1, 1011, c, inst if n == 3 else NONE, 1]
    assert words.shape == (n, 272) and words[inst, c] == words[0, c] ^ 1 and (words[:, np.arange(272) != c] == words[0, np.arange(272) != c]).all()
    assert chunk_result(ds, ps, xs, 1000) == [1, 1011, c, inst if n == 3 else NONE]


def test_first_is_the_lowest_byte_then_the_lowest_element():
    ds, ps, xs = _agree(3, 30)
    _plant(ds, ps, xs, 1, 9, 3)       # a later byte, low element
    _plant(ds, ps, xs, 2, 4, 270)     # the first byte that differs, high element ...
    _plant(ds, ps, xs, 0, 4, 258)     # ... and a lower element of the same byte: this one is first
    rec, words = lstm_vote_reference(ds, ps, xs, 0)
    assert rec == [1, 30, 3, 1, 4, 258, 0, 3]
    assert words[0, 258] != words[1, 258] == words[2, 258]
    assert chunk_result(ds, ps, xs, 0) == [3, 4, 258, NONE]   # three different odd instances in one chunk: no single one


def test_odd_instance_and_no_majority():
    for inst in range(3):
        ds, ps, xs = _agree(3, 8)
        _plant(ds, ps, xs, inst, 2, 100)
        assert lstm_vote_reference(ds, ps, xs)[0][6] == inst
    ds, ps, xs = _agree(3, 8)
    _plant(ds, ps, xs, 1, 2, 100, 1)
    _plant(ds, ps, xs, 2, 2, 100, 2)      # all three differ
    rec, _ = lstm_vote_reference(ds, ps, xs)
    assert rec[3:] == [1, 2, 100, NONE, 1]
    ds, ps, xs = _agree(2, 8)
    _plant(ds, ps, xs, 0, 7, 271)
    assert lstm_vote_reference(ds, ps, xs)[0] == [1, 8, 2, 1, 7, 271, NONE, 1]


def test_words_not_floats():
    ds, ps, xs = _agree(3, 5)
    for d in ds:
        d[3, 17] = 0.0
        d[1, 1] = np.float32("nan")            # one NaN pattern in every instance: equal words
    assert lstm_vote_reference(ds, ps, xs)[0][3] == 0
    ds[2][3, 17] = -0.0                        # == 0.0 as a float, another word
    assert ds[2][3, 17] == ds[0][3, 17]
    assert lstm_vote_reference(ds, ps, xs)[0] == [1, 5, 3, 1, 3, 17, 2, 1]
    ds[2][3, 17] = 0.0
    ds[1].view(np.uint32)[1, 1] ^= 1           # another NaN pattern
    assert np.isnan(ds[1][1, 1]) and lstm_vote_reference(ds, ps, xs)[0] == [1, 5, 3, 1, 1, 1, 1, 1]


def test_a_second_chunk_leaves_the_first_event_and_advances_the_counters():
    tw = LstmVoteTwin(3)
    a = _agree(3, 10, 1)
    assert tw.run(*a, stream_byte0=0) == [0, 0, 0, 0] and tw.record == [1, 10, 3, 0, 0, 0, 0, 0] and tw.words is None
    b = _agree(3, 12, 2)
    _plant(*b, 2, 5, 260)
    assert tw.run(*b, stream_byte0=10) == [1, 15, 260, 2]
    assert tw.record == [2, 22, 3, 1, 15, 260, 2, 1]
    first_words = tw.words.copy()
    c = _agree(3, 7, 3)
    _plant(*c, 0, 0, 0)
    _plant(*c, 0, 1, 0)
    assert tw.run(*c, stream_byte0=22) == [2, 22, 0, 0]
    assert tw.record == [3, 29, 3, 2, 15, 260, 2, 1] and np.array_equal(tw.words, first_words)
    assert tw.run(*_agree(3, 4, 4), stream_byte0=29) == [0, 0, 0, 0] and tw.record == [4, 33, 3, 2, 15, 260, 2, 1]


@pytest.mark.parametrize("n", [2, 3])
def test_strided_instance_0_equals_a_dense_copy(n):
    N = 19
    ds, ps, xs = _agree(n, N)
    rng = np.random.default_rng(5)
    layer0 = rng.random((8 * N, 2078), dtype=np.float32)
    layer0[:, 2077] = ps[0].reshape(-1)
    assert np.array_equal(bit_predictions(layer0), ps[0].view(np.uint32))
    for plant in (None, (0, 6, 259), (n - 1, 18, 263)):
        dd, pp, xx = [d.copy() for d in ds], [p.copy() for p in ps], [x.copy() for x in xs]
        l0 = layer0.copy()
        if plant:
            _plant(dd, pp, xx, *plant)
            l0[:, 2077] = pp[0].reshape(-1)
        dense = lstm_vote_reference(dd, pp, xx, 77)
        strided = lstm_vote_reference(dd, [l0] + pp[1:], xx, 77)
        assert dense[0] == strided[0] and (dense[1] is None) == (strided[1] is None) == (plant is None)
        if plant:
            assert np.array_equal(dense[1], strided[1]) and dense[0][4:6] == [77 + plant[1], plant[2]]
        assert chunk_result(dd, pp, xx, 77) == chunk_result(dd, [l0] + pp[1:], xx, 77)
    l0 = layer0.copy()
    l0[:, :2077] += 1.0                        # the other 2077 columns are not the vote's business
    assert lstm_vote_reference(ds, [l0] + ps[1:], xs)[0][3] == 0


def test_element_names():
    assert element_name(0) == "distribution entry 0" and element_name(255) == "distribution entry 255"
    assert element_name(256) == "bit 0's prediction (layer-0 column 2077)" and element_name(263) == "bit 7's prediction (layer-0 column 2077)"
    assert element_name(264) == "bit 0's ex" and element_name(271) == "bit 7's ex"


def test_bad_arguments():
    ds, ps, xs = _agree(3, 4)
    with pytest.raises(ValueError, match="2 or 3"):
        lstm_vote_reference(ds[:1], ps[:1], xs[:1])
    with pytest.raises(ValueError, match="4-byte"):
        lstm_vote_reference([d.astype(np.float64) for d in ds], ps, xs)


# ---- plumbing ----------------------------------------------------------------------------------------------------------------

def test_engine_stream_takes_lstm_shadow():
    from cmix_amd.pipeline import EngineStream
    p = inspect.signature(EngineStream.__init__).parameters
    assert "lstm_shadow" in p and p["lstm_shadow"].default == 0


def test_the_header_declares_the_new_names():
    text = open(os.path.join(ROOT, "include", "cmix_amd.h")).read()
    for name in ("cmx_lstmvote_create", "cmx_lstmvote_destroy", "cmx_lstmvote_run", "cmx_lstmvote_report", "cmx_lstmvote_record", "cmx_lstmvote_values",
                 "cmx_lstmvote_last", "cmx_lstm_state_diff", "cmx_lstm_debug_state_xor", "cmx_lstm_debug_layout", "cmx_pipeline_set_lstm_shadow",
                 "cmx_pipeline_lstm_shadow_report", "cmx_pipeline_lstm_shadow_values", "cmx_pipeline_lstm_shadow_state_diff",
                 "cmx_pipeline_debug_lstm_shadow_xor", "cmx_set_lstm_shadow", "cmx_lstm_shadow_report"):
        assert re.search(r"\b%s\(" % name, text), name
    assert re.search(r"#define CMX_LSTMVOTE_COLS 272\b", text)


def test_the_bindings_mirror_the_header():
    from cmix_amd import engine as E
    assert E.LSTMVOTE_COLS == COLS and len(E.LSTM_STATE_REGIONS) == 11 and len(E.LSTM_STATE_ARRAYS) == 80 and len(set(E.LSTM_STATE_ARRAYS)) == 80
    assert E.LSTM_STATE_ARRAYS[24] == "gb[0][0]" and E.LSTM_STATE_REGIONS[4] == "gb" and E.LSTM_STATE_REGIONS[9] == "indices"
    for cls, names in ((E.Lstm, ("state_diff", "debug_state_xor")), (E.LstmVote, ("run", "report", "last", "values", "close")),
                       (E.Pipeline, ("set_lstm_shadow", "lstm_shadow_report", "lstm_shadow_values", "lstm_shadow_state_diff", "debug_lstm_shadow_xor")),
                       (E.Predictor, ("set_lstm_shadow", "lstm_shadow_report"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(E.lstm_layout)


def test_lstm_vote_without_a_gpu_is_an_error():
    from cmix_amd import engine as E
    if E.device_count() > 0:
        pytest.skip("a HIP device is visible: the refusal cannot be shown")
    with pytest.raises(E.CmxError, match="no HIP device"):
        E.LstmVote(3)
