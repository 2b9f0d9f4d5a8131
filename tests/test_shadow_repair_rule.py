"""CPU: the rule by which an outvoted mixing network is repaired from the majority (cmix_amd/vote.py::repair_decision, the specification of
shadow_repair in cmix_amd/csrc/pipeline_api.hip) over hand-made per-chunk results, the chunk's own result (chunk_result, the twin of
cmx_vote_last), and the new entry points at every layer: declared in include/cmix_amd.h, exported by the built library, bound in Python."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NEW = ["cmx_vote_last", "cmx_mixnet_state_repair", "cmx_pipeline_set_shadow_repair", "cmx_pipeline_shadow_repairs",
       "cmx_set_shadow_repair", "cmx_shadow_repairs", "cmx_debug_shadow_xor", "cmx_repair_text"]
AGREE = (0, 0)


def test_every_chunk_agrees():
    from cmix_amd.vote import repair_decision
    assert repair_decision(2, [AGREE] * 8, 0, 2) == ("clean", None)
    assert repair_decision(2, [], 0, 2) == ("clean", None)
    assert repair_decision(2, [AGREE], 0, 0) == ("clean", None)


def test_one_odd_instance_is_repaired():
    from cmix_amd.vote import repair_decision
    for o in (0, 1, 2):
        assert repair_decision(2, [AGREE, (5, o), (900, o), (7, o)], 0, 2) == ("repair", o)
    # a chunk in flight behind the event may agree again (the difference has not reached an output): still one odd instance
    assert repair_decision(2, [(1, 2), AGREE, (3, 2)], 1, 2) == ("repair", 2)


def test_the_odd_instance_changes_between_chunks_in_flight():
    from cmix_amd.vote import repair_decision
    assert repair_decision(2, [(5, 0), (5, 1)], 0, 4) == ("stop", "second odd instance")
    assert repair_decision(2, [AGREE, (1, 2), AGREE, (1, 0)], 0, 4) == ("stop", "second odd instance")


def test_no_majority_at_any_chunk_stops():
    from cmix_amd.vote import NONE, repair_decision
    assert repair_decision(2, [(5, NONE)], 0, 4) == ("stop", "no majority")
    assert repair_decision(2, [(5, 1), (1, 1), (2, NONE)], 0, 4) == ("stop", "no majority")


def test_budget_exhausted_and_time_out():
    from cmix_amd.vote import repair_decision
    assert repair_decision(2, [(5, 1)], 1, 2) == ("repair", 1)
    assert repair_decision(2, [(5, 1)], 2, 2) == ("stop", "budget")
    assert repair_decision(2, [(5, 1)], 0, 0) == ("stop", "no repair")
    assert repair_decision(2, [(5, 1)], 0, 2, timed_out=True) == ("stop", "time-out")


def test_one_shadow_has_no_majority_to_continue_on():
    from cmix_amd.vote import NONE, repair_decision
    assert repair_decision(1, [(5, NONE)], 0, 4) == ("stop", "no repair")
    assert repair_decision(0, [(5, 0)], 0, 4) == ("stop", "no repair")


def _arrays(n, T, seed=3):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)
    m = rng.integers(0, 1 << 32, (T, 47), dtype=np.uint64).astype(np.uint32)
    return [p.copy() for _ in range(n)], [m.copy() for _ in range(n)]


def test_the_chunks_own_result():
    from cmix_amd.vote import NONE, chunk_result
    ps, ms = _arrays(3, 30)
    assert chunk_result(ps, ms, 100) == [0, 0, 0, 0]
    ms[1][10, 31] ^= 4
    ps[1][29] ^= 1
    assert chunk_result(ps, ms, 100) == [2, 110, 31, 1]
    ms[2][10, 30] ^= 4          # another instance odd at another element: no ONE odd instance
    assert chunk_result(ps, ms, 100) == [3, 110, 30, NONE]
    ms[2][10, 30] ^= 4
    ms[0][3, 0] ^= 1
    ms[2][3, 0] ^= 2            # all three differ at one element
    assert chunk_result(ps, ms, 0) == [3, 3, 0, NONE]
    ps2, ms2 = _arrays(2, 5)
    ps2[0][4] ^= 1
    assert chunk_result(ps2, ms2, 8) == [1, 12, 47, NONE]


def test_header_declares_every_new_function_and_no_longer_calls_continuation_out_of_scope():
    raw = open(os.path.join(ROOT, "include", "cmix_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(cmx_[a-z0-9_]+)\s*\(", src))
    assert not [n for n in NEW if n not in declared]
    assert "Out of scope: continuing on the majority" not in raw


def test_library_exports_and_python_binds_every_new_function():
    from cmix_amd import build, engine, pipeline
    build.build()
    raw = C.CDLL(engine.LIB_PATH)
    assert not [n for n in NEW if not hasattr(raw, n)]
    L = engine.lib()
    assert not [n for n in NEW if getattr(L, n).argtypes is None]
    for cls, names in ((engine.MixNet, ("state_repair",)), (engine.Vote, ("last",)), (engine.Pipeline, ("set_shadow_repair", "shadow_repairs")),
                       (engine.Predictor, ("set_shadow_repair", "shadow_repairs", "debug_shadow_xor"))):
        assert not [n for n in names if not callable(getattr(cls, n, None))]
    assert "repair" in pipeline.EngineStream.__init__.__code__.co_varnames
