"""CPU: the redundant context-stage vote's rule (cmix_amd/ctxvote.py::ctx_vote_reference, the host twin and specification of cmx_ctxvote_run in
cmix_amd/csrc/ctxmodels_vote.hip) on hand-made arrays, and the new entry points at every layer: declared in include/cmix_amd.h, bound by
cmix_amd.engine.lib(), exported by the built library."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["cmx_ctxmodels_create_compact", "cmx_ctxmodels_state_diff", "cmx_ctxmodels_debug_state_xor", "cmx_ctxmodels_debug_layout",
       "cmx_ctxvote_create", "cmx_ctxvote_destroy", "cmx_ctxvote_run", "cmx_ctxvote_report", "cmx_ctxvote_record", "cmx_ctxvote_values", "cmx_ctxvote_last",
       "cmx_pipeline_set_ctx_shadow", "cmx_pipeline_ctx_shadow_report", "cmx_pipeline_ctx_shadow_values", "cmx_pipeline_ctx_shadow_state_diff",
       "cmx_pipeline_debug_ctx_shadow_xor", "cmx_set_ctx_shadow", "cmx_ctx_shadow_report", "cmx_debug_ctx_shadow_xor"]


def _arrays(n, T, seed=3):
    """n identical instances: model outputs [T, 54] and selectors [T, 47] of random words"""
    rng = np.random.default_rng(seed)
    o = rng.integers(0, 1 << 32, (T, 54), dtype=np.uint64).astype(np.uint32)
    s = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
    return [o.copy() for _ in range(n)], [s.copy() for _ in range(n)]


def test_all_agree():
    from cmix_amd.ctxvote import chunk_result, ctx_vote_reference
    os_, ss = _arrays(3, 16)
    rec, words = ctx_vote_reference(os_, ss, 700)
    assert rec == [1, 16, 3, 0, 0, 0, 0, 0] and words is None
    rec, words = ctx_vote_reference(os_[:2], ss[:2])
    assert rec == [1, 16, 2, 0, 0, 0, 0, 0] and words is None
    assert chunk_result(os_, ss, 700) == [0, 0, 0, 0]


def test_every_instance_can_be_the_odd_one():
    from cmix_amd.ctxvote import chunk_result, ctx_vote_reference
    T = 24
    for odd in range(3):
        os_, ss = _arrays(3, T)
        os_[odd][5, 7] ^= 0x10
        rec, words = ctx_vote_reference(os_, ss, 1000)
        assert rec == [1, T, 3, 1, 1005, 7, odd, 1]
        assert words.shape == (3, 101) and len({int(x) for x in words[:, 7]}) == 2
        assert (words[:, :54] == np.stack([o[5] for o in os_])).all() and (words[:, 54:] == ss[0][5]).all()
        assert chunk_result(os_, ss, 1000) == [1, 1005, 7, odd]


def test_all_three_differ_is_no_majority():
    from cmix_amd.ctxvote import NONE, chunk_result, ctx_vote_reference
    os_, ss = _arrays(3, 8)
    ss[1][2, 0] ^= 1
    ss[2][2, 0] ^= 2
    rec, words = ctx_vote_reference(os_, ss, 40)
    assert NONE == (1 << 64) - 1 and rec == [1, 8, 3, 1, 42, 54, NONE, 1]
    assert len({int(x) for x in words[:, 54]}) == 3
    assert chunk_result(os_, ss, 40)[3] == NONE


def test_two_instances_mismatch_is_no_majority():
    from cmix_amd.ctxvote import NONE, ctx_vote_reference
    os_, ss = _arrays(2, 8)
    ss[1][4, 46] ^= 1   # the last element of a row
    assert ctx_vote_reference(os_, ss, 0)[0] == [1, 8, 2, 1, 4, 100, NONE, 1]


def test_first_element_in_the_model_columns_or_in_the_selectors():
    from cmix_amd.ctxvote import NONE, chunk_result, ctx_vote_reference, element_name
    os_, ss = _arrays(3, 16)
    ss[1][10, 0] ^= 4       # e = 10 * 101 + 54: the first selector, right behind the seam
    os_[2][10, 53] ^= 4     # e = 10 * 101 + 53: the last model column of the same bit comes first
    rec, _ = ctx_vote_reference(os_, ss, 0)
    assert rec == [1, 16, 3, 1, 10, 53, 2, 2] and element_name(53) == "layer-0 column 2075"
    assert chunk_result(os_, ss, 0) == [2, 10, 53, NONE]   # two elements with different odd instances
    os_[2][10, 53] ^= 4
    rec, _ = ctx_vote_reference(os_, ss, 0)
    assert rec == [1, 16, 3, 1, 10, 54, 1, 1] and element_name(54) == "selector 0"
    ss[2][9, 46] ^= 4       # the bit before: its last selector comes before every element of bit 10
    rec, _ = ctx_vote_reference(os_, ss, 0)
    assert rec == [1, 16, 3, 1, 9, 100, 2, 2] and element_name(100) == "selector 46"
    assert [element_name(c) for c in (0, 2, 3)] == ["layer-0 column 0", "layer-0 column 2", "layer-0 column 2025"]


def test_values_are_compared_as_words_not_floats():
    from cmix_amd.ctxvote import ctx_vote_reference
    T = 8
    os_ = [np.zeros((T, 54), np.float32) for _ in range(3)]
    ss = [np.zeros((T, 47), np.uint32) for _ in range(3)]
    os_[1][1, 0] = -0.0   # == 0.0 as a float, another word
    assert ctx_vote_reference(os_, ss, 0)[0] == [1, T, 3, 1, 1, 0, 1, 1]
    os_[1][1, 0] = 0.0
    nan = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    for o in os_:
        o[2, 5] = nan   # nan != nan as floats, the same word
    rec, words = ctx_vote_reference(os_, ss, 0)
    assert rec == [1, T, 3, 0, 0, 0, 0, 0] and words is None
    os_[0][2, 5] = np.array([0x7FC00124], np.uint32).view(np.float32)[0]   # another NaN pattern
    assert ctx_vote_reference(os_, ss, 0)[0] == [1, T, 3, 1, 2, 5, 0, 1]


def test_model_outputs_of_a_full_and_a_compact_matrix():
    from cmix_amd.ctxvote import LAYER0_COLS, model_outputs
    rng = np.random.default_rng(1)
    full = rng.integers(0, 1 << 32, (8, 2078), dtype=np.uint64).astype(np.uint32)
    compact = np.zeros((8, 64), np.uint32)
    compact[:, :54] = full[:, LAYER0_COLS]
    assert LAYER0_COLS == [0, 1, 2] + list(range(2025, 2076)) and len(LAYER0_COLS) == 54
    assert np.array_equal(model_outputs(full, False), model_outputs(compact, True))


def test_header_declares_every_new_function():
    src = open(os.path.join(ROOT, "include", "cmix_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmx_[a-z0-9_]+)\s*\(", src))
    assert not [n for n in NEW if n not in declared]


def test_library_exports_and_python_binds_every_new_function():
    from cmix_amd import build, engine
    build.build()
    raw = C.CDLL(engine.LIB_PATH)
    assert not [n for n in NEW if not hasattr(raw, n)]
    L = engine.lib()
    assert not [n for n in NEW if getattr(L, n).argtypes is None]
    for cls, names in ((engine.CtxModels, ("state_diff", "debug_state_xor")), (engine.CtxVote, ("run", "report", "values", "last")),
                       (engine.Pipeline, ("set_ctx_shadow", "ctx_shadow_report", "ctx_shadow_values", "ctx_shadow_state_diff", "debug_ctx_shadow_xor")),
                       (engine.Predictor, ("set_ctx_shadow", "ctx_shadow_report", "debug_ctx_shadow_xor"))):
        assert not [n for n in names if not callable(getattr(cls, n, None))]
    import inspect
    from cmix_amd.pipeline import EngineStream
    assert "ctx_shadow" in inspect.signature(EngineStream.__init__).parameters and "compact" in inspect.signature(engine.CtxModels.__init__).parameters
