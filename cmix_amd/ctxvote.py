"""The redundant context-stage vote's rule in pure numpy: the host twin of cmx_ctxvote_run (cmix_amd/csrc/ctxmodels_vote.hip) and its specification;
the counterpart of cmix_amd/vote.py for the producer of the selectors.

n = 2 or 3 instances each produce, per bit t, the 54 model outputs of the context stage (lane order: layer-0 columns 0, 1, 2, 2025..2075) and the 47
mixer selectors. Values are compared as 32-bit words, never as floats (-0.0 differs from 0.0; equal NaN patterns are equal). Elements are ordered by
e = t * 101 + c, c = 0..53 the model output and c = 54..100 selector c - 54. n = 3: all equal agree, exactly two equal make the third the odd
instance, all different is no majority; n = 2: different is no majority."""
import numpy as np

NONE = (1 << 64) - 1   # "no majority" in field [6]
MODELS, SELECTORS = 54, 47
COLS = MODELS + SELECTORS
LAYER0_COLS = [0, 1, 2] + list(range(2025, 2076))   # the layer-0 column of model output c


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError("ctx_vote_reference: arrays of 4-byte words")
    return a.view(np.uint32)


def model_outputs(probs, compact):
    """the [T, 54] words an instance's matrix holds: columns 0..53 of the compact form ([T, >= 64]), columns LAYER0_COLS of the full one ([T, >= 2078])"""
    w = _words(probs)
    return w[:, :MODELS].copy() if compact else w[:, LAYER0_COLS].copy()


def element_name(c):
    return "layer-0 column %d" % LAYER0_COLS[c] if c < MODELS else "selector %d" % (c - MODELS)


def _stack(outs, sels):
    n = len(outs)
    if n not in (2, 3) or len(sels) != n:
        raise ValueError("ctx_vote_reference: 2 or 3 instances")
    T = _words(sels[0]).size // SELECTORS
    w = np.empty((n, T, COLS), np.uint32)
    for i in range(n):
        w[i, :, :MODELS] = _words(outs[i]).reshape(T, MODELS)
        w[i, :, MODELS:] = _words(sels[i]).reshape(T, SELECTORS)
    return w


def ctx_vote_reference(outs, sels, stream_bit0=0):
    """outs: n arrays [T, 54] (model_outputs); sels: n arrays [T, 47] (taken as words). Returns (record, words): record = the eight fields one
    cmx_ctxvote_run call on a fresh handle leaves -- [0] chunks (1), [1] bits, [2] n, [3] 1 if any element does not agree, then [4] the stream bit of
    the smallest non-agreeing e, [5] its c, [6] the odd instance there or NONE, [7] the non-agreeing elements (0 in [4..7] without an event) -- and
    words = the captured [n, 101] uint32 words of that bit (None without an event)."""
    w = _stack(outs, sels)
    n, T = w.shape[0], w.shape[1]
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


def chunk_result(outs, sels, stream_bit0=0):
    """The chunk's own result as cmx_ctxvote_last reports it: [elements, stream bit, c, odd]. odd is the ONE instance that is odd at every
    non-agreeing element, else NONE (an element at which all differ, two instances, or elements with different odd instances)."""
    rec, _ = ctx_vote_reference(outs, sels, stream_bit0)
    if not rec[3]:
        return [0, 0, 0, 0]
    w = _stack(outs, sels)
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
