"""The redundant mixing-network vote's rule in pure numpy: the host twin of cmx_vote_run (cmix_amd/csrc/mixnet_vote.hip) and its specification.

n = 2 or 3 instances each produce, per bit t, 47 mixer outputs and the final p. Values are compared as 32-bit words, never as floats (-0.0 differs
from 0.0; equal NaN patterns are equal). Elements are ordered by e = t * 48 + c, c = 0..46 the mixer and c = 47 the final p: the causal order
within a bit. n = 3: all equal agree, exactly two equal make the third the odd instance, all different is no majority; n = 2: different is no
majority."""
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
