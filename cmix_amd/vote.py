"""The redundant mixing-network vote's rule in pure numpy: the host twin of cmx_vote_run (cmix_amd/csrc/mixnet_vote.hip) and its specification.

n = 2 or 3 instances each produce, per bit t, 47 mixer outputs and the final p. Values are compared as 32-bit words, never as floats (-0.0 differs
from 0.0; equal NaN patterns are equal). Elements are ordered by e = t * 48 + c, c = 0..46 the mixer and c = 47 the final p: the causal order
within a bit. n = 3: all equal agree, exactly two equal make the third the odd instance, all different is no majority; n = 2: different is no
majority.

repair_decision is the rule by which the pipeline, with repair armed, chooses between repairing the outvoted instance from the majority and
stopping (cmx_pipeline_set_shadow_repair); chunk_result is the twin of cmx_vote_last, the per-chunk result that rule reads."""
import numpy as np

from .votecore import NONE, chunk_rule, vote_rule, words  # noqa: F401 (NONE is this module's too)

COLS = 48


def _stack(ps, mixes):
    n = len(ps)
    if n not in (2, 3) or len(mixes) != n:
        raise ValueError("vote_reference: 2 or 3 instances")
    T = words(ps[0], "vote_reference").size
    w = np.empty((n, T, COLS), np.uint32)
    for i in range(n):
        w[i, :, :47] = words(mixes[i], "vote_reference").reshape(T, 47)
        w[i, :, 47] = words(ps[i], "vote_reference").reshape(T)
    return w


def vote_reference(ps, mixes, stream_bit0=0):
    """ps: n arrays [T]; mixes: n arrays [T, 47] (float32 or uint32, taken as words). Returns (record, words) as votecore.vote_rule: the eight fields
    one cmx_vote_run call on a fresh handle leaves ([1] bits, [4] the stream bit, [5] the column) and the captured [n, 48] uint32 words of that bit."""
    return vote_rule(_stack(ps, mixes), stream_bit0)


def repair_decision(shadow, results, repairs_made, max_repairs, timed_out=False):
    """The pipeline's rule for an event with repair armed (cmx_pipeline_set_shadow_repair; its twin is shadow_repair in cmix_amd/csrc/pipeline_api.hip).
    results: the own result of every chunk the instances have run since the last repair, oldest first, each (elements, odd) as cmx_vote_last gives
    them -- elements == 0 agrees, odd = 0 / 1 / 2 the chunk's odd instance, NONE no majority. Returns ("clean", None) when every chunk agrees,
    ("repair", o) when instance o is to be repaired from a member of the majority, else ("stop", reason): repair is off or the vote has fewer than
    three instances, a shadow timed out, some chunk has no majority, two chunks name different odd instances, or the budget is used up."""
    events = [(int(n), int(o)) for n, o in results if n]
    if not events:
        return "clean", None
    if max_repairs <= 0 or shadow != 2:
        return "stop", "no repair"
    if timed_out:
        return "stop", "time-out"
    if any(o == NONE for _, o in events):
        return "stop", "no majority"
    if len({o for _, o in events}) > 1:
        return "stop", "second odd instance"
    if repairs_made >= max_repairs:
        return "stop", "budget"
    return "repair", events[0][1]


def chunk_result(ps, mixes, stream_bit0=0):
    """The chunk's own result as cmx_vote_last reports it: [elements, stream bit, column, odd] (votecore.chunk_rule)."""
    return chunk_rule(_stack(ps, mixes), stream_bit0)
