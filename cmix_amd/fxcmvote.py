"""The redundant fxcm-stage vote's rule in pure numpy: the host twin of cmx_fxcmvote_run (cmix_amd/csrc/fxcm_vote.hip) and its specification; the
counterpart of cmix_amd/lstmvote.py for the producer of layer-0 columns 3..433.

n = 2 or 3 instances each produce, per BIT t of a chunk, the 431 values FXCM::Predict() returns before that bit is coded. Values are compared as
32-bit words, never as floats (-0.0 differs from 0.0; equal NaN patterns are equal). Elements are ordered by e = t * 431 + c, c = 0..430 = layer-0
column 3 + c; "first" is the lowest bit, then the lowest column. n = 3: all equal agree, exactly two equal make the third the odd instance, all
different is no majority; n = 2: different is no majority."""
import numpy as np

from .votecore import NONE, VoteTwin, chunk_rule, vote_rule, words  # noqa: F401 (NONE is this module's too)

COLS = 431
FIRST_COL = 3          # of the 431 in a layer-0 row or in a shadow's dense row
LAYER0_STRIDE, SHADOW_STRIDE = 2078, 434


def rows_of(r):
    """the [T, 431] words of an instance: a [T, 431] array as it is, or columns 3..433 of a wider one ([T, 2078] layer-0 rows read in place, [T, 434]
    a shadow's dense rows)"""
    w = words(r, "fxcm_vote_reference")
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


def fxcm_vote_reference(rows, stream_bit0=0):
    """rows: n arrays of T rows (see rows_of). Returns (record, words) as votecore.vote_rule: the eight fields one cmx_fxcmvote_run call on a fresh
    handle leaves ([1] bits, [4] the stream bit, [5] the fxcm column c) and the captured [n, 431] uint32 words of that bit."""
    return vote_rule(_stack(rows), stream_bit0)


def chunk_result(rows, stream_bit0=0):
    """The chunk's own result as cmx_fxcmvote_last reports it: [elements, stream bit, c, odd] (votecore.chunk_rule)."""
    return chunk_rule(_stack(rows), stream_bit0)


class FxcmVoteTwin(VoteTwin):
    """votecore.VoteTwin over the fxcm stage's rows, as a cmx_fxcmvote_t keeps its record"""

    def run(self, rows, stream_bit0=0):
        return VoteTwin.run(self, _stack(rows), stream_bit0)
