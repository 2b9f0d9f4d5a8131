"""The redundant LSTM-stage vote's rule in pure numpy: the host twin of cmx_lstmvote_run (cmix_amd/csrc/lstm_vote.hip) and its specification; the
counterpart of cmix_amd/ctxvote.py for the producer of layer-0 column 2077 and of fxcm's LSTM hints.

n = 2 or 3 instances each produce, per byte b of a chunk, the distribution after that byte (256 words, zeros outside the vocabulary), the
ByteModel::Predict value of each of the byte's eight bits and the eight `ex` words. Values are compared as 32-bit words, never as floats (-0.0 differs
from 0.0; equal NaN patterns are equal). Elements are ordered by e = b * 272 + c: c = 0..255 the distribution entry, c = 256..263 bit c - 256's
prediction, c = 264..271 bit c - 264's ex; "first" is the lowest byte, then the lowest element. n = 3: all equal agree, exactly two equal make the
third the odd instance, all different is no majority; n = 2: different is no majority."""
import numpy as np

NONE = (1 << 64) - 1   # "no majority" in field [6]
DIST, BITS = 256, 8
COLS = DIST + 2 * BITS
LAYER0_STRIDE, LSTM_COL = 2078, 2077


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError("lstm_vote_reference: arrays of 4-byte words")
    return a.view(np.uint32)


def bit_predictions(p):
    """the [N, 8] words of an instance's bit predictions: a dense array of 8 N words, or column 2077 of a [8 N, 2078] layer-0 matrix (read in place)"""
    w = _words(p)
    if w.ndim == 2 and w.shape[1] == LAYER0_STRIDE:
        return w[:, LSTM_COL].reshape(-1, BITS).copy()
    return w.reshape(-1, BITS).copy()


def element_name(c):
    if c < DIST:
        return "distribution entry %d" % c
    if c < DIST + BITS:
        return "bit %d's prediction (layer-0 column 2077)" % (c - DIST)
    return "bit %d's ex" % (c - DIST - BITS)


def _stack(dists, bit_ps, exs):
    n = len(dists)
    if n not in (2, 3) or len(bit_ps) != n or len(exs) != n:
        raise ValueError("lstm_vote_reference: 2 or 3 instances")
    N = _words(exs[0]).size // BITS
    w = np.empty((n, N, COLS), np.uint32)
    for i in range(n):
        w[i, :, :DIST] = _words(dists[i]).reshape(N, DIST)
        w[i, :, DIST:DIST + BITS] = bit_predictions(bit_ps[i])
        w[i, :, DIST + BITS:] = _words(exs[i]).reshape(N, BITS)
    return w


def _differ(w):
    differ = (w != w[0]).any(axis=0)
    if w.shape[0] == 3:
        differ |= w[1] != w[2]
    return differ


def lstm_vote_reference(dists, bit_ps, exs, stream_byte0=0):
    """dists: n arrays [N, 256]; bit_ps: n arrays of 8 N words or [8 N, 2078] layer-0 matrices; exs: n arrays [N, 8] (all taken as words). Returns
    (record, words): record = the eight fields one cmx_lstmvote_run call on a fresh handle leaves -- [0] chunks (1), [1] bytes, [2] n, [3] 1 if any
    element does not agree, then [4] the stream byte of the smallest non-agreeing e, [5] its c, [6] the odd instance there or NONE, [7] the
    non-agreeing elements (0 in [4..7] without an event) -- and words = the captured [n, 272] uint32 words of that byte (None without an event)."""
    w = _stack(dists, bit_ps, exs)
    n, N = w.shape[0], w.shape[1]
    differ = _differ(w)
    rec = [1, N, n, 0, 0, 0, 0, 0]
    if not differ.any():
        return rec, None
    e = int(np.flatnonzero(differ.reshape(-1))[0])
    b, c = divmod(e, COLS)
    v = [int(w[i, b, c]) for i in range(n)]
    odd = NONE
    if n == 3:
        if v[1] == v[2]:
            odd = 0
        elif v[0] == v[2]:
            odd = 1
        elif v[0] == v[1]:
            odd = 2
    rec[3:] = [1, stream_byte0 + b, c, odd, int(differ.sum())]
    return rec, w[:, b, :].copy()


def chunk_result(dists, bit_ps, exs, stream_byte0=0):
    """The chunk's own result as cmx_lstmvote_last reports it: [elements, stream byte, c, odd]. odd is the ONE instance that is odd at every
    non-agreeing element, else NONE (an element at which all differ, two instances, or elements with different odd instances)."""
    rec, _ = lstm_vote_reference(dists, bit_ps, exs, stream_byte0)
    if not rec[3]:
        return [0, 0, 0, 0]
    w = _stack(dists, bit_ps, exs)
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


class LstmVoteTwin:
    """The sticky record over several chunks, as a cmx_lstmvote_t keeps it: run() folds one chunk; record [8], last [4], words (the first event's row)."""

    def __init__(self, n):
        self.n = int(n)
        self.record = [0, 0, self.n, 0, 0, 0, 0, 0]
        self.last = [0, 0, 0, 0]
        self.words = None

    def run(self, dists, bit_ps, exs, stream_byte0=0):
        if len(dists) != self.n:
            raise ValueError("LstmVoteTwin.run: %d instances" % self.n)
        rec, words = lstm_vote_reference(dists, bit_ps, exs, stream_byte0)
        self.last = chunk_result(dists, bit_ps, exs, stream_byte0)
        self.record[0] += 1
        self.record[1] += rec[1]
        if rec[3]:
            if not self.record[3]:
                self.record[4:] = rec[4:]
                self.words = words
            self.record[3] += 1
        return self.last
