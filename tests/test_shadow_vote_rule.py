"""CPU: the redundant mixing-network vote's rule (cmix_amd/vote.py::vote_reference, the host twin and specification of cmx_vote_run in
cmix_amd/csrc/mixnet_vote.hip) on hand-made arrays, and the new entry points at every layer: declared in include/cmix_amd.h, bound by
cmix_amd.engine.lib(), exported by the built library."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["cmx_vote_create", "cmx_vote_destroy", "cmx_vote_run", "cmx_vote_report", "cmx_vote_record", "cmx_vote_values",
       "cmx_mixnet_state_diff", "cmx_mixnet_debug_state_xor",
       "cmx_pipeline_set_shadow", "cmx_pipeline_shadow_report", "cmx_pipeline_shadow_values", "cmx_pipeline_shadow_state_diff",
       "cmx_pipeline_debug_shadow_xor", "cmx_set_shadow", "cmx_shadow_report"]


def _arrays(n, T, seed=3):
    """n identical instances: p [T] and mix [T, 47] of random words"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)
    m = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
    return [p.copy() for _ in range(n)], [m.copy() for _ in range(n)]


def test_all_agree():
    from cmix_amd.vote import vote_reference
    ps, ms = _arrays(3, 20)
    rec, words = vote_reference(ps, ms, 700)
    assert rec == [1, 20, 3, 0, 0, 0, 0, 0] and words is None
    rec, words = vote_reference(ps[:2], ms[:2])
    assert rec == [1, 20, 2, 0, 0, 0, 0, 0] and words is None


def test_instance_2_odd_at_the_last_element():
    from cmix_amd.vote import vote_reference
    T = 20
    ps, ms = _arrays(3, T)
    ps[2][T - 1] ^= 1   # e = (T - 1) * 48 + 47: the last element of the chunk
    rec, words = vote_reference(ps, ms, 1000)
    assert rec == [1, T, 3, 1, 1000 + T - 1, 47, 2, 1]
    assert words.shape == (3, 48) and words[0, 47] == ps[0][T - 1] and words[2, 47] == ps[2][T - 1] and (words[:, :47] == ms[0][T - 1]).all()


def test_the_primary_odd_at_column_47_only():
    from cmix_amd.vote import vote_reference
    ps, ms = _arrays(3, 9)
    ps[0][4] ^= 0x80
    rec, words = vote_reference(ps, ms, 8)
    assert rec == [1, 9, 3, 1, 12, 47, 0, 1]
    assert words[0, 47] != words[1, 47] and words[1, 47] == words[2, 47]


def test_two_instances_deviate_at_different_elements_the_earliest_wins():
    from cmix_amd.vote import vote_reference
    ps, ms = _arrays(3, 30)
    ms[1][10, 31] ^= 4      # e = 10 * 48 + 31
    ms[2][10, 30] ^= 4      # e = 10 * 48 + 30: earlier in the causal order of the same bit
    rec, _ = vote_reference(ps, ms, 0)
    assert rec == [1, 30, 3, 1, 10, 30, 2, 2]
    ms[2][10, 30] ^= 4
    ps[2][9] ^= 4           # the bit before: its final p comes before every column of bit 10
    rec, _ = vote_reference(ps, ms, 0)
    assert rec == [1, 30, 3, 1, 9, 47, 2, 2]
    ps[2][9] ^= 4
    rec, _ = vote_reference(ps, ms, 0)
    assert rec == [1, 30, 3, 1, 10, 31, 1, 1]


def test_all_three_differ_is_no_majority():
    from cmix_amd.vote import NONE, vote_reference
    ps, ms = _arrays(3, 5)
    ms[1][2, 0] ^= 1
    ms[2][2, 0] ^= 2
    rec, words = vote_reference(ps, ms, 40)
    assert NONE == (1 << 64) - 1 and rec == [1, 5, 3, 1, 42, 0, NONE, 1]
    assert len({int(x) for x in words[:, 0]}) == 3


def test_two_instances_mismatch_is_no_majority():
    from cmix_amd.vote import NONE, vote_reference
    ps, ms = _arrays(2, 5)
    ms[1][4, 46] ^= 1
    assert vote_reference(ps, ms, 0)[0] == [1, 5, 2, 1, 4, 46, NONE, 1]


def test_values_are_compared_as_words_not_floats():
    from cmix_amd.vote import vote_reference
    T = 3
    ps = [np.zeros(T, np.float32) for _ in range(3)]
    ms = [np.zeros((T, 47), np.float32) for _ in range(3)]
    ps[1][1] = -0.0   # == 0.0 as a float, another word
    assert vote_reference(ps, ms, 0)[0] == [1, T, 3, 1, 1, 47, 1, 1]
    ps[1][1] = 0.0
    nan = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    for m in ms:
        m[2, 5] = nan   # nan != nan as floats, the same word
    rec, words = vote_reference(ps, ms, 0)
    assert rec == [1, T, 3, 0, 0, 0, 0, 0] and words is None
    ms[0][2, 5] = np.array([0x7FC00124], np.uint32).view(np.float32)[0]   # another NaN pattern
    assert vote_reference(ps, ms, 0)[0] == [1, T, 3, 1, 2, 5, 0, 1]


def test_a_chunk_of_one_bit():
    from cmix_amd.vote import NONE, vote_reference
    ps, ms = _arrays(3, 1)
    assert vote_reference(ps, ms, 77)[0] == [1, 1, 3, 0, 0, 0, 0, 0]
    ms[0][0, 0] ^= 1
    assert vote_reference(ps, ms, 77)[0] == [1, 1, 3, 1, 77, 0, 0, 1]
    ps2, ms2 = _arrays(2, 1)
    ps2[1][0] ^= 1
    assert vote_reference(ps2, ms2, 77)[0] == [1, 1, 2, 1, 77, 47, NONE, 1]


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
    for cls, names in ((engine.MixNet, ("state_diff", "debug_state_xor")), (engine.Vote, ("run", "report", "values")),
                       (engine.Pipeline, ("set_shadow", "shadow_report", "shadow_values", "shadow_state_diff", "debug_shadow_xor")),
                       (engine.Predictor, ("set_shadow",))):
        assert not [n for n in names if not callable(getattr(cls, n, None))]
