"""The redundant LSTM-stage vote's rule in pure numpy: the host twin of cmx_lstmvote_run (cmix_amd/csrc/lstm_vote.hip) and its specification; the
counterpart of cmix_amd/ctxvote.py for the producer of layer-0 column 2077 and of fxcm's LSTM hints.

n = 2 or 3 instances each produce, per byte b of a chunk, the distribution after that byte (256 words, zeros outside the vocabulary), the
ByteModel::Predict value of each of the byte's eight bits and the eight `ex` words. Values are compared as 32-bit words, never as floats (-0.0 differs
from 0.0; equal NaN patterns are equal). Elements are ordered by e = b * 272 + c: c = 0..255 the distribution entry, c = 256..263 bit c - 256's
prediction, c = 264..271 bit c - 264's ex; "first" is the lowest byte, then the lowest element. n = 3: all equal agree, exactly two equal make the
third the odd instance, all different is no majority; n = 2: different is no majority."""
import numpy as np

from .votecore import NONE, VoteTwin, chunk_rule, vote_rule, words  # noqa: F401 (NONE is this module's too)

DIST, BITS = 256, 8
COLS = DIST + 2 * BITS
LAYER0_STRIDE, LSTM_COL = 2078, 2077
WHO = "lstm_vote_reference"


def bit_predictions(p):
    """the [N, 8] words of an instance's bit predictions: a dense array of 8 N words, or column 2077 of a [8 N, 2078] layer-0 matrix (read in place)"""
    w = words(p, WHO)
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
    N = words(exs[0], WHO).size // BITS
    w = np.empty((n, N, COLS), np.uint32)
    for i in range(n):
        w[i, :, :DIST] = words(dists[i], WHO).reshape(N, DIST)
        w[i, :, DIST:DIST + BITS] = bit_predictions(bit_ps[i])
        w[i, :, DIST + BITS:] = words(exs[i], WHO).reshape(N, BITS)
    return w


def lstm_vote_reference(dists, bit_ps, exs, stream_byte0=0):
    """dists: n arrays [N, 256]; bit_ps: n arrays of 8 N words or [8 N, 2078] layer-0 matrices; exs: n arrays [N, 8] (all taken as words). Returns
    (record, words) as votecore.vote_rule: the eight fields one cmx_lstmvote_run call on a fresh handle leaves ([1] bytes, [4] the stream byte, [5] the
    element's c) and the captured [n, 272] uint32 words of that byte."""
    return vote_rule(_stack(dists, bit_ps, exs), stream_byte0)


def chunk_result(dists, bit_ps, exs, stream_byte0=0):
    """The chunk's own result as cmx_lstmvote_last reports it: [elements, stream byte, c, odd] (votecore.chunk_rule)."""
    return chunk_rule(_stack(dists, bit_ps, exs), stream_byte0)


class LstmVoteTwin(VoteTwin):
    """votecore.VoteTwin over the LSTM stage's arrays, as a cmx_lstmvote_t keeps its record"""

    def run(self, dists, bit_ps, exs, stream_byte0=0):
        return VoteTwin.run(self, _stack(dists, bit_ps, exs), stream_byte0)
