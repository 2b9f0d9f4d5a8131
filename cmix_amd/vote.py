"""The redundant mixing-network vote's rule in pure numpy: the host twin of cmx_vote_run (cmix_amd/csrc/mixnet_vote.hip) and its specification.

n = 2 or 3 instances each produce, per bit t, 47 mixer outputs and the final p. Values are compared as 32-bit words, never as floats (-0.0 differs
from 0.0; equal NaN patterns are equal). Elements are ordered by e = t * 48 + c, c = 0..46 the mixer and c = 47 the final p: the causal order
within a bit. n = 3: all equal agree, exactly two equal make the third the odd instance, all different is no majority; n = 2: different is no
majority.

repair_decision is the rule by which the pipeline, with repair armed, chooses between repairing the outvoted instance from the majority and
stopping (cmx_pipeline_set_shadow_repair); chunk_result is the twin of cmx_vote_last, the per-chunk result that rule reads."""
import numpy as np

NONE = (1 << 64) - 1   # "no majority" in field [6]
COLS = 48


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError("vote_reference: arrays of 4-byte words")
    return a.view(np.uint32)


def vote_reference(ps, mixes, stream_bit0=0):
    """ps: n arrays [T]; mixes: n arrays [T, 47] (float32 or uint32, taken as words). Returns (record, words): record = the eight fields one
    cmx_vote_run call on a fresh handle leaves -- [0] chunks (1), [1] bits, [2] n, [3] 1 if any element does not agree, then [4] the stream bit of
    the smallest non-agreeing e, [5] its column, [6] the odd instance there or NONE, [7] the non-agreeing elements (0 in [4..7] without an event) --
    and words = the captured [n, 48] uint32 words of that bit (None without an event)."""
    n = len(ps)
    if n not in (2, 3) or len(mixes) != n:
        raise ValueError("vote_reference: 2 or 3 instances")
    T = _words(ps[0]).size
    w = np.empty((n, T, COLS), np.uint32)
    for i in range(n):
        w[i, :, :47] = _words(mixes[i]).reshape(T, 47)
        w[i, :, 47] = _words(ps[i]).reshape(T)
    differ = (w != w[0]).any(axis=0)
    if n == 3:
        differ |= w[1] != w[2]
    rec = [1, T, n, 0, 0, 0, 0, 0]
    if not differ.any():
        return rec, None
    e = int(np.flatnonzero(differ.reshape(-1))[0])
    t, c = divmod(e, COLS)
    v = [int(w[i, t, c]) for i in range(n)]
    odd = NONE
    if n == 3:
        if v[1] == v[2]:
            odd = 0
        elif v[0] == v[2]:
            odd = 1
        elif v[0] == v[1]:
            odd = 2
    rec[3:] = [1, stream_bit0 + t, c, odd, int(differ.sum())]
    return rec, w[:, t, :].copy()


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
    """The chunk's own result as cmx_vote_last reports it: [elements, stream bit, column, odd]. odd is the ONE instance that is odd at every
    non-agreeing element, else NONE (an element at which all differ, two instances, or elements with different odd instances)."""
    rec, _ = vote_reference(ps, mixes, stream_bit0)
    if not rec[3]:
        return [0, 0, 0, 0]
    n = len(ps)
    w = np.stack([np.concatenate([_words(mixes[i]).reshape(-1, 47), _words(ps[i]).reshape(-1, 1)], axis=1) for i in range(n)])
    odd = set()
    if n == 2:
        odd.add(NONE)
    else:
        a, b, c = w[0] == w[1], w[1] == w[2], w[0] == w[2]
        if (b & ~a).any():
            odd.add(0)
        if (c & ~a).any():
            odd.add(1)
        if (a & ~b).any():
            odd.add(2)
        if (~a & ~b & ~c).any():
            odd.add(NONE)
    return [rec[7], rec[4], rec[5], odd.pop() if len(odd) == 1 else NONE]
