"""The redundant context-stage vote's rule in pure numpy: the host twin of cmx_ctxvote_run (cmix_amd/csrc/ctxmodels_vote.hip) and its specification;
the counterpart of cmix_amd/vote.py for the producer of the selectors.

n = 2 or 3 instances each produce, per bit t, the 54 model outputs of the context stage (lane order: layer-0 columns 0, 1, 2, 2025..2075) and the 47
mixer selectors. Values are compared as 32-bit words, never as floats (-0.0 differs from 0.0; equal NaN patterns are equal). Elements are ordered by
e = t * 101 + c, c = 0..53 the model output and c = 54..100 selector c - 54. n = 3: all equal agree, exactly two equal make the third the odd
instance, all different is no majority; n = 2: different is no majority."""
import numpy as np

from .votecore import NONE, chunk_rule, vote_rule, words  # noqa: F401 (NONE is this module's too)

MODELS, SELECTORS = 54, 47
COLS = MODELS + SELECTORS
LAYER0_COLS = [0, 1, 2] + list(range(2025, 2076))   # the layer-0 column of model output c
WHO = "ctx_vote_reference"


def model_outputs(probs, compact):
    """the [T, 54] words an instance's matrix holds: columns 0..53 of the compact form ([T, >= 64]), columns LAYER0_COLS of the full one ([T, >= 2078])"""
    w = words(probs, WHO)
    return w[:, :MODELS].copy() if compact else w[:, LAYER0_COLS].copy()


def element_name(c):
    return "layer-0 column %d" % LAYER0_COLS[c] if c < MODELS else "selector %d" % (c - MODELS)


def _stack(outs, sels):
    n = len(outs)
    if n not in (2, 3) or len(sels) != n:
        raise ValueError("ctx_vote_reference: 2 or 3 instances")
    T = words(sels[0], WHO).size // SELECTORS
    w = np.empty((n, T, COLS), np.uint32)
    for i in range(n):
        w[i, :, :MODELS] = words(outs[i], WHO).reshape(T, MODELS)
        w[i, :, MODELS:] = words(sels[i], WHO).reshape(T, SELECTORS)
    return w


def ctx_vote_reference(outs, sels, stream_bit0=0):
    """outs: n arrays [T, 54] (model_outputs); sels: n arrays [T, 47] (taken as words). Returns (record, words) as votecore.vote_rule: the eight fields
    one cmx_ctxvote_run call on a fresh handle leaves ([1] bits, [4] the stream bit, [5] the element's c) and the captured [n, 101] uint32 words of that
    bit."""
    return vote_rule(_stack(outs, sels), stream_bit0)


def chunk_result(outs, sels, stream_bit0=0):
    """The chunk's own result as cmx_ctxvote_last reports it: [elements, stream bit, c, odd] (votecore.chunk_rule)."""
    return chunk_rule(_stack(outs, sels), stream_bit0)
