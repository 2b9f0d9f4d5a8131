"""The rule of the four redundant votes in pure numpy: the host twin and specification of what cmix_amd/csrc/cmx_vote_core.h computes on the device.

n = 2 or 3 instances each produce rows of COLS values, stacked here as w [n, rows, COLS] uint32. Values are compared as 32-bit words, never as floats
(-0.0 differs from 0.0; equal NaN patterns are equal). Elements are ordered by e = row * COLS + c. n = 3: all equal agree, exactly two equal make the
third the odd instance, all different is no majority; n = 2: different is no majority. vote.py, ctxvote.py, lstmvote.py and fxcmvote.py build the
stack of their stage and name its elements."""
import numpy as np

NONE = (1 << 64) - 1   # "no majority" in field [6]


def words(a, who):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError("%s: arrays of 4-byte words" % who)
    return a.view(np.uint32)


def _differ(w):
    differ = (w != w[0]).any(axis=0)
    if w.shape[0] == 3:
        differ |= w[1] != w[2]
    return differ


def vote_rule(w, unit0=0):
    """(record, words): record = the eight fields one vote call on a fresh handle leaves -- [0] chunks (1), [1] rows, [2] n, [3] 1 if any element does
    not agree, then [4] the stream position (unit0 + row) of the smallest non-agreeing e, [5] its column, [6] the odd instance there or NONE, [7] the
    non-agreeing elements (0 in [4..7] without an event) -- and words = the captured [n, COLS] words of that row (None without an event)."""
    n, rows, cols = w.shape
    differ = _differ(w)
    rec = [1, rows, n, 0, 0, 0, 0, 0]
    if not differ.any():
        return rec, None
    t, c = divmod(int(np.flatnonzero(differ.reshape(-1))[0]), cols)
    v = [int(w[i, t, c]) for i in range(n)]
    odd = NONE
    if n == 3:
        if v[1] == v[2]:
            odd = 0
        elif v[0] == v[2]:
            odd = 1
        elif v[0] == v[1]:
            odd = 2
    rec[3:] = [1, unit0 + t, c, odd, int(differ.sum())]
    return rec, w[:, t, :].copy()


def chunk_rule(w, unit0=0):
    """The chunk's own result as cmx_*vote_last reports it: [elements, stream position, column, odd]. odd is the ONE instance that is odd at every
    non-agreeing element, else NONE (an element at which all differ, two instances, or elements with different odd instances)."""
    rec, _ = vote_rule(w, unit0)
    if not rec[3]:
        return [0, 0, 0, 0]
    odd = set()
    if w.shape[0] == 2:
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


class VoteTwin:
    """The sticky record over several chunks, as a vote handle keeps it: run() folds one chunk's stack; record [8], last [4], words (the first
    event's row). A stage's twin overrides run() to take that stage's arrays."""

    def __init__(self, n):
        self.n = int(n)
        self.record = [0, 0, self.n, 0, 0, 0, 0, 0]
        self.last = [0, 0, 0, 0]
        self.words = None

    def run(self, w, unit0=0):
        if w.shape[0] != self.n:
            raise ValueError("%s.run: %d instances" % (type(self).__name__, self.n))
        rec, words = vote_rule(w, unit0)
        self.last = chunk_rule(w, unit0)
        self.record[0] += 1
        self.record[1] += rec[1]
        if rec[3]:
            if not self.record[3]:
                self.record[4:] = rec[4:]
                self.words = words
            self.record[3] += 1
        return self.last
