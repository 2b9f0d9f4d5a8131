"""The redundant fxcm-stage vote's rule in pure numpy: the host twin of cmx_fxcmvote_run (cmix_amd/csrc/fxcm_vote.hip) and its specification; the
counterpart of cmix_amd/lstmvote.py for the producer of layer-0 columns 3..433.

n = 2 or 3 instances each produce, per BIT t of a chunk, the 431 values FXCM::Predict() returns before that bit is coded. Values are compared as
32-bit words, never as floats (-0.0 differs from 0.0; equal NaN patterns are equal). Elements are ordered by e = t * 431 + c, c = 0..430 = layer-0
column 3 + c; "first" is the lowest bit, then the lowest column. n = 3: all equal agree, exactly two equal make the third the odd instance, all
different is no majority; n = 2: different is no majority."""
import numpy as np

NONE = (1 << 64) - 1   # "no majority" in field [6]
COLS = 431
FIRST_COL = 3          # of the 431 in a layer-0 row or in a shadow's dense row
LAYER0_STRIDE, SHADOW_STRIDE = 2078, 434


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError("fxcm_vote_reference: arrays of 4-byte words")
    return a.view(np.uint32)


def rows_of(r):
    """the [T, 431] words of an instance: a [T, 431] array as it is, or columns 3..433 of a wider one ([T, 2078] layer-0 rows read in place, [T, 434]
    a shadow's dense rows)"""
    w = _words(r)
    if w.ndim != 2 or w.shape[1] < COLS:
        raise ValueError("fxcm_vote_reference: rows of at least 431 words")
    return w if w.shape[1] == COLS else w[:, FIRST_COL:FIRST_COL + COLS]


def column_name(c):
    return "fxcm column %d (layer-0 column %d)" % (c, FIRST_COL + c)


def _stack(rows):
    n = len(rows)
    if n not in (2, 3):
        raise ValueError("fxcm_vote_reference: 2 or 3 instances")
    w = [rows_of(r) for r in rows]
    if any(x.shape != w[0].shape for x in w):
        raise ValueError("fxcm_vote_reference: the instances have different row counts")
    return np.stack(w)


def _differ(w):
    differ = (w != w[0]).any(axis=0)
    if w.shape[0] == 3:
        differ |= w[1] != w[2]
    return differ


def fxcm_vote_reference(rows, stream_bit0=0):
    """rows: n arrays of T rows (see rows_of). Returns (record, words): record = the eight fields one cmx_fxcmvote_run call on a fresh handle leaves --
    [0] chunks (1), [1] bits, [2] n, [3] 1 if any element does not agree, then [4] the stream bit of the smallest non-agreeing e, [5] its c, [6] the
    odd instance there or NONE, [7] the non-agreeing elements (0 in [4..7] without an event) -- and words = the captured [n, 431] uint32 words of that
    bit (None without an event)."""
    w = _stack(rows)
    n, T = w.shape[0], w.shape[1]
    differ = _differ(w)
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


def chunk_result(rows, stream_bit0=0):
    """The chunk's own result as cmx_fxcmvote_last reports it: [elements, stream bit, c, odd]. odd is the ONE instance that is odd at every
    non-agreeing element, else NONE (an element at which all differ, two instances, or elements with different odd instances)."""
    rec, _ = fxcm_vote_reference(rows, stream_bit0)
    if not rec[3]:
        return [0, 0, 0, 0]
    w = _stack(rows)
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


class FxcmVoteTwin:
    """The sticky record over several chunks, as a cmx_fxcmvote_t keeps it: run() folds one chunk; record [8], last [4], words (the first event's row)."""

    def __init__(self, n):
        self.n = int(n)
        self.record = [0, 0, self.n, 0, 0, 0, 0, 0]
        self.last = [0, 0, 0, 0]
        self.words = None

    def run(self, rows, stream_bit0=0):
        if len(rows) != self.n:
            raise ValueError("FxcmVoteTwin.run: %d instances" % self.n)
        rec, words = fxcm_vote_reference(rows, stream_bit0)
        self.last = chunk_result(rows, stream_bit0)
        self.record[0] += 1
        self.record[1] += rec[1]
        if rec[3]:
            if not self.record[3]:
                self.record[4:] = rec[4:]
                self.words = words
            self.record[3] += 1
        return self.last
