"""CPU: the fxcm-stage vote's rule (cmix_amd/fxcmvote.py, the host twin and specification of cmx_fxcmvote_run in cmix_amd/csrc/fxcm_vote.hip) on
hand-made rows, the refusals of the new entry points that need no device, and the constants the header, the bindings and the sources share."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cmix_amd.fxcmvote import COLS, FIRST_COL, NONE, FxcmVoteTwin, chunk_result, column_name, fxcm_vote_reference, rows_of

CSRC = os.path.join(ROOT, "cmix_amd", "csrc")


def _agree(n, T, seed=3):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 32, (T, COLS), dtype=np.uint64).astype(np.uint32)
    return [base.copy() for _ in range(n)]


# ---- the rule ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_agreeing_instances_leave_a_clean_record(n):
    rows = _agree(n, 24)
    rec, words = fxcm_vote_reference(rows, 800)
    assert rec == [1, 24, n, 0, 0, 0, 0, 0] and words is None
    assert chunk_result(rows, 800) == [0, 0, 0, 0]


@pytest.mark.parametrize("c", [0, 63, 64, 430])
@pytest.mark.parametrize("inst", [0, 1, 2])
def test_one_planted_word_names_its_bit_column_and_instance(inst, c):
    rows = _agree(3, 16)
    rows[inst][5, c] ^= np.uint32(1)
    rec, words = fxcm_vote_reference(rows, 1000)
    assert rec == [1, 16, 3, 1, 1005, c, inst, 1]
    assert words.shape == (3, COLS) and all(np.array_equal(words[i], rows[i][5]) for i in range(3))
    assert chunk_result(rows, 1000) == [1, 1005, c, inst]


@pytest.mark.parametrize("inst", [0, 1])
def test_two_instances_have_no_majority(inst):
    rows = _agree(2, 8)
    rows[inst][7, 430] ^= np.uint32(0x80000000)
    rec, _ = fxcm_vote_reference(rows, 0)
    assert rec == [1, 8, 2, 1, 7, 430, NONE, 1]
    assert chunk_result(rows, 0) == [1, 7, 430, NONE]


def test_three_different_words_have_no_majority():
    rows = _agree(3, 8)
    rows[1][2, 10] ^= np.uint32(1)
    rows[2][2, 10] ^= np.uint32(2)
    rec, _ = fxcm_vote_reference(rows, 0)
    assert rec == [1, 8, 3, 1, 2, 10, NONE, 1]


def test_first_is_the_lowest_bit_then_the_lowest_column():
    rows = _agree(3, 32)
    rows[2][9, 3] ^= np.uint32(1)      # a later bit, a low column
    rows[1][4, 400] ^= np.uint32(1)    # the lowest bit, a high column ...
    rows[0][4, 17] ^= np.uint32(1)     # ... and a lower column of the same bit: the first
    rec, words = fxcm_vote_reference(rows, 64)
    assert rec == [1, 32, 3, 1, 68, 17, 0, 3]
    assert np.array_equal(words[1], rows[1][4])
    assert chunk_result(rows, 64) == [3, 68, 17, NONE]   # the chunk's elements have different odd instances


def test_words_not_floats():
    a = np.zeros((4, COLS), np.float32)
    b = a.copy()
    b[1, 2] = -0.0
    assert fxcm_vote_reference([a, b], 0)[0][3:6] == [1, 1, 2]
    nan = np.full((4, COLS), np.nan, np.float32)
    assert fxcm_vote_reference([nan, nan.copy(), nan.copy()], 0)[0][3] == 0


def test_a_second_chunk_leaves_the_first_event_and_advances_the_counters():
    tw = FxcmVoteTwin(3)
    rows = _agree(3, 16)
    assert tw.run(rows, 0) == [0, 0, 0, 0] and tw.record == [1, 16, 3, 0, 0, 0, 0, 0]
    rows = _agree(3, 16, 4)
    rows[1][3, 64] ^= np.uint32(4)
    assert tw.run(rows, 16) == [1, 19, 64, 1]
    first = list(tw.record)
    assert first == [2, 32, 3, 1, 19, 64, 1, 1]
    rows2 = _agree(3, 16, 5)
    rows2[0][0, 0] ^= np.uint32(1)
    assert tw.run(rows2, 32) == [1, 32, 0, 0]
    assert tw.record == [3, 48, 3, 2] + first[4:] and np.array_equal(tw.words[1], rows[1][3])
    with pytest.raises(ValueError, match="3 instances"):
        tw.run(rows[:2], 48)


@pytest.mark.parametrize("n", [2, 3])
def test_instance_0_in_place_equals_a_dense_copy(n):
    """instance 0 as columns 3..433 of layer-0 rows of 2078 words, the shadows as rows of 434"""
    rng = np.random.default_rng(11)
    rows = _agree(n, 12)
    rows[n - 1][11, 430] ^= np.uint32(1)
    l0 = rng.integers(0, 1 << 32, (12, 2078), dtype=np.uint64).astype(np.uint32)
    l0[:, FIRST_COL:FIRST_COL + COLS] = rows[0]
    wide = [l0]
    for r in rows[1:]:
        w = rng.integers(0, 1 << 32, (12, 434), dtype=np.uint64).astype(np.uint32)
        w[:, FIRST_COL:] = r
        wide.append(w)
    assert np.array_equal(rows_of(l0), rows[0])
    got, want = fxcm_vote_reference(wide, 7), fxcm_vote_reference(rows, 7)
    assert got[0] == want[0] == [1, 12, n, 1, 18, 430, n - 1 if n == 3 else NONE, 1] and np.array_equal(got[1], want[1])


def test_column_names_and_bad_arguments():
    assert column_name(0) == "fxcm column 0 (layer-0 column 3)" and column_name(430) == "fxcm column 430 (layer-0 column 433)"
    rows = _agree(3, 4)
    with pytest.raises(ValueError, match="2 or 3"):
        fxcm_vote_reference(rows[:1])
    with pytest.raises(ValueError, match="4-byte"):
        fxcm_vote_reference([r.astype(np.float64) for r in rows])
    with pytest.raises(ValueError, match="431"):
        fxcm_vote_reference([r[:, :100] for r in rows])
    with pytest.raises(ValueError, match="row counts"):
        fxcm_vote_reference([rows[0], rows[1][:2]])


# ---- refusals that need no device ---------------------------------------------------------------------------------------------

def test_refusals_without_a_device():
    from cmix_amd import engine as E
    L = E.lib()
    out = (E.C.c_uint64 * 17)()
    cases = [(lambda: L.cmx_fxcmvote_create(0, 4), "n must be 2 or 3"), (lambda: L.cmx_fxcmvote_create(0, 1), "n must be 2 or 3"),
             (lambda: L.cmx_fxcmvote_run(None, None, None, 8, 0, None, None), "cmx_fxcmvote_run: bad argument"),
             (lambda: L.cmx_fxcmvote_report(None, out), "cmx_fxcmvote_report: bad argument"),
             (lambda: L.cmx_fxcm_run_shared(None, None, None, 1, None, None, None, 434, None), "cmx_fxcm_run_shared: null handle"),
             (lambda: L.cmx_fxcm_state_diff(None, None, out), "cmx_fxcm_state_diff: bad argument"),
             (lambda: L.cmx_fxcm_debug_state_xor(None, 9, 0, 1), "cmx_fxcm_debug_state_xor: null handle"),
             (lambda: L.cmx_fxcm_debug_layout(None, None), "cmx_fxcm_debug_layout: bad argument"),
             (lambda: L.cmx_pipeline_set_fxcm_shadow(None, 1), "cmx_pipeline_set_fxcm_shadow: null handle"),
             (lambda: L.cmx_pipeline_fxcm_shadow_report(None, out), "cmx_pipeline_fxcm_shadow_report: bad argument"),
             (lambda: L.cmx_pipeline_fxcm_shadow_state_diff(None, 0, 1, out), "cmx_pipeline_fxcm_shadow_state_diff: bad argument"),
             (lambda: L.cmx_pipeline_debug_fxcm_shadow_xor(None, 0, 9, 0, 1), "cmx_pipeline_debug_fxcm_shadow_xor: null handle"),
             (lambda: L.cmx_set_fxcm_shadow(None, 1), "cmx_set_fxcm_shadow: null handle"),
             (lambda: L.cmx_fxcm_shadow_report(None, out), "cmx_fxcm_shadow_report: bad argument")]
    for call, text in cases:
        r = call()
        assert r is None or r != 0, text   # NULL or non-zero: refused
        assert text in E.last_error(), (text, E.last_error())
    assert L.cmx_fxcmvote_record(None) is None


# ---- plumbing and shared constants ---------------------------------------------------------------------------------------------

def test_engine_stream_takes_fxcm_shadow():
    from cmix_amd.pipeline import EngineStream
    p = inspect.signature(EngineStream.__init__).parameters
    assert "fxcm_shadow" in p and p["fxcm_shadow"].default == 0


def test_the_header_declares_the_new_names():
    text = open(os.path.join(ROOT, "include", "cmix_amd.h")).read()
    for name in ("cmx_fxcm_create_shadow", "cmx_fxcm_run_shared", "cmx_fxcm_state_diff", "cmx_fxcm_debug_state_xor", "cmx_fxcm_debug_layout",
                 "cmx_fxcmvote_create", "cmx_fxcmvote_destroy", "cmx_fxcmvote_run", "cmx_fxcmvote_report", "cmx_fxcmvote_record", "cmx_fxcmvote_values",
                 "cmx_fxcmvote_last", "cmx_pipeline_set_fxcm_shadow", "cmx_pipeline_fxcm_shadow_report", "cmx_pipeline_fxcm_shadow_values",
                 "cmx_pipeline_fxcm_shadow_state_diff", "cmx_pipeline_debug_fxcm_shadow_xor", "cmx_set_fxcm_shadow", "cmx_fxcm_shadow_report"):
        assert re.search(r"\b%s\(" % name, text), name


def _enum(text, name):
    return int(re.search(r"\b%s = (\d+)" % name, text).group(1))


def test_the_constants_of_header_sources_and_bindings_agree():
    from cmix_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "cmix_amd.h")).read()
    rec = open(os.path.join(CSRC, "fxcm_rec.h")).read()
    bld = open(os.path.join(CSRC, "fxcm_build.h")).read()
    st = open(os.path.join(CSRC, "fxcm_state.h")).read()
    define = lambda text, name: int(re.search(r"#define %s (\d+)\b" % name, text).group(1))
    assert define(hdr, "CMX_FXCMVOTE_COLS") == _enum(rec, "FX_OUTPUTS") == COLS == E.FXCMVOTE_COLS == 431
    # the blocks fxb::build asks its policy for: three tables and six state tables; per map buckets, `tab`, StateMaps; the SSCMs; three sm1_t; rcm_t,
    # mhash, sp_table, buffer; twelve wx; per APM its table and (inside pattern16) the fill pattern
    nmaps, nsscm = _enum(rec, "FX_NMAPS"), _enum(rec, "FX_NSSCM")
    assert "for (int k = 0; k < 12; k++)" in bld and "for (int j = 0; j < 6; j++)" in bld and "sm1_n[3]" in bld and "k < 6; k++) h.sta[k]" in bld
    blocks = 3 + 6 + nmaps * 3 + nsscm + 3 + 4 + 12 + 6 * 2
    assert define(hdr, "CMX_FXCM_STATE_ARRAYS") == define(st, "FX_STATE_ARRAYS") == blocks + 1 == len(E.FXCM_STATE_ARRAYS) == len(set(E.FXCM_STATE_ARRAYS))
    assert define(hdr, "CMX_FXCM_STATE_REGIONS") == define(st, "FX_STATE_REGIONS") == len(E.FXCM_STATE_REGIONS) == 12
    assert define(hdr, "CMX_FXCM_STATE_OUT") == 5 + 12
    assert E.FXCM_STATE_REGIONS.index("wx") == 9 and E.FXCM_STATE_REGIONS.index("apm") == 10 and E.FXCM_STATE_REGIONS.index("map_statemaps") == 2
    assert E.FXCM_STATE_ARRAYS[9] == "maps[0].tab" and E.FXCM_STATE_ARRAYS[46] == "maps[0].t" and E.FXCM_STATE_ARRAYS[-1] == "FxDev"
    for cls, names in ((E.Fxcm, ("run_shared", "state_diff", "debug_state_xor")), (E.FxcmVote, ("run", "report", "last", "values", "close")),
                       (E.Pipeline, ("set_fxcm_shadow", "fxcm_shadow_report", "fxcm_shadow_values", "fxcm_shadow_state_diff", "debug_fxcm_shadow_xor")),
                       (E.Predictor, ("set_fxcm_shadow", "fxcm_shadow_report"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(E.fxcm_layout)
    assert "shadow" in inspect.signature(E.Fxcm.__init__).parameters
