"""The stream journal: per-block digests of what the final mixing network reads and writes, in the form of the reference-side trace tools
(ref_long_trace, ref_ctx_trace, scripts/gpu_stage_hashes.py; the HIP kernel is cmix_amd/csrc/journal.hip).

    A[c] = splitmix64(c) | 1, B[i] = splitmix64(0x1000000 + i) | 1, u32(x) = the word's bit pattern; sums mod 2^64 over the bits t of a block of
    2^log2 stream bits, i = t mod 2^19:
      column group g (0..129): sum_t sum_{c in [16 g, min(16 g + 16, 2078))} (u32(row[t][c]) + 1) * A[c] * B[i]
      p                      : sum_t (u32(p[t]) + 1) * B[i]
      selector m (0..46)     : sum_t (sel[t][m] + 1) * B[i]
      bits                   : sum_t (bit[t] + 1) * B[i]

A record is 179 words (130 groups, p, 47 selectors, bits) and carries the block's end byte position. B's index does not depend on the block
size, so the records of the sub-blocks of a 64 KB block add up to the reference's line. On disk a journal is two text files: `path` holds
"<end byte> <131 hex words>" per block (groups, then p: what ref_long_trace writes and takes as its fourth argument), `path.inputs`
"<end byte> <48 hex words>" (selectors, then bits).

    python -m cmix_amd.journal diff a b     the first block and word in which two journals differ (exit status 1 if they do)

This module is numpy only: digests() is the model the kernel is tested against, and needs no GPU."""
import os
import sys

import numpy as np

NG = 130          # column groups
N_COLS = 2078
N_SEL = 47
WORDS = 179       # NG groups, p, N_SEL selectors, bits
W_P = NG
W_SEL = NG + 1
W_BITS = NG + 1 + N_SEL
MIN_LOG2, MAX_LOG2 = 6, 19
_MASK19 = np.uint64((1 << 19) - 1)


def splitmix64(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def A():
    return splitmix64(np.arange(N_COLS, dtype=np.uint64)) | np.uint64(1)


def B(t):
    """B of stream bits t (any integer array): its index is t mod 2^19 whatever the block size."""
    t = np.asarray(t, np.uint64)
    with np.errstate(over="ignore"):
        return splitmix64(np.uint64(0x1000000) + (t & _MASK19)) | np.uint64(1)


def _u32(x):
    """the words' bit patterns, zero-extended to u64 (floats are taken as they lie; integers keep their low 32 bits)"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        x = x.view(np.uint32)
    elif x.dtype.kind == "f":
        raise TypeError("journal: float words must be float32")
    return x.astype(np.uint64) & np.uint64(0xFFFFFFFF)


def digests(rows, sel, bits, p, stream_bit0=0, log2=MAX_LOG2):
    """The records of the T bits whose first is stream bit stream_bit0: (ends, words) with ends [nblocks] u64 (each block's end byte position
    so far) and words [nblocks, 179] u64. rows [T, 2078] f32 (or u32), sel [T, 47], bits [T], p [T] f32; any of them may be None: its words
    stay zero."""
    if not MIN_LOG2 <= log2 <= MAX_LOG2:
        raise ValueError("journal: log2 must be 6..19")
    T = next((len(x) for x in (rows, sel, bits, p) if x is not None), 0)
    if T == 0:
        return np.zeros(0, np.uint64), np.zeros((0, WORDS), np.uint64)
    t = np.uint64(stream_bit0) + np.arange(T, dtype=np.uint64)
    blk = (t >> np.uint64(log2)) - (np.uint64(stream_bit0) >> np.uint64(log2))
    starts = np.flatnonzero(np.r_[True, blk[1:] != blk[:-1]])
    b = B(t)
    words = np.zeros((len(starts), WORDS), np.uint64)
    with np.errstate(over="ignore"):
        if rows is not None:
            v = _u32(rows)
            assert v.shape == (T, N_COLS)
            w = np.zeros((T, 16 * NG), np.uint64)
            w[:, :N_COLS] = (v + np.uint64(1)) * A()[None, :]
            g = w.reshape(T, NG, 16).sum(2, dtype=np.uint64) * b[:, None]
            words[:, :NG] = np.add.reduceat(g, starts, axis=0, dtype=np.uint64)
        if p is not None:
            words[:, W_P] = np.add.reduceat((_u32(p).reshape(T) + np.uint64(1)) * b, starts, dtype=np.uint64)
        if sel is not None:
            s = _u32(sel)
            assert s.shape == (T, N_SEL)
            words[:, W_SEL:W_BITS] = np.add.reduceat((s + np.uint64(1)) * b[:, None], starts, axis=0, dtype=np.uint64)
        if bits is not None:
            words[:, W_BITS] = np.add.reduceat((_u32(bits).reshape(T) + np.uint64(1)) * b, starts, dtype=np.uint64)
    first = int(stream_bit0) >> log2
    end = int(stream_bit0) + T
    ends = np.array([min((first + i + 1) << log2, end) >> 3 for i in range(len(starts))], np.uint64)
    return ends, words


def group_name(g):
    """Who owns the columns of group g; g = 130 is the final p."""
    if g == NG:
        return "final p"
    lo, hi = 16 * g, min(N_COLS, 16 * g + 16) - 1

    def owner(c):
        return ("contexts" if c < 3 or 2025 <= c < 2076 else "PPMd" if c == 2076 else "LSTM" if c == 2077 else "fxcm" if c < 434 else "paq8[%d]" % (c - 434))
    a, b = owner(lo), owner(hi)
    return "cols %d..%d (%s)" % (lo, hi, a if a == b else a + " .. " + b)


def word_name(w):
    """What word w (0..178) of a record digests."""
    if w < NG:
        return "column group %d: %s" % (w, group_name(w))
    if w == W_P:
        return "p"
    if w < W_BITS:
        return "selector %d" % (w - W_SEL)
    return "bits"


def write(path, ends, words):
    """`path` (groups + p) and `path.inputs` (selectors + bits)."""
    words = np.asarray(words, np.uint64).reshape(-1, WORDS)
    with open(path, "w") as f, open(path + ".inputs", "w") as fi:
        for e, w in zip(ends, words):
            f.write("%d %s\n" % (int(e), " ".join("%016x" % int(x) for x in w[:W_SEL])))
            fi.write("%d %s\n" % (int(e), " ".join("%016x" % int(x) for x in w[W_SEL:])))


def _read_lines(path, n):
    ends, rows = [], []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if len(tok) < 1 + n:
                raise ValueError("%s: a line of %d words, expected %d" % (path, len(tok) - 1, n))
            ends.append(int(tok[0]))
            rows.append([int(x, 16) for x in tok[1:1 + n]])   # (ref_long_trace's WITH_ORACLE_MIXNET build appends text: ignored)
    return np.array(ends, np.uint64), np.array(rows, np.uint64).reshape(-1, n)


def read(path):
    """(ends, words [nblocks, 179]) from `path` and, where it exists, `path.inputs` (else the selector and bits words are zero)."""
    ends, main = _read_lines(path, W_SEL)
    words = np.zeros((len(ends), WORDS), np.uint64)
    words[:, :W_SEL] = main
    if os.path.exists(path + ".inputs"):
        ei, inputs = _read_lines(path + ".inputs", WORDS - W_SEL)
        if not np.array_equal(ei, ends):
            raise ValueError("%s and %s.inputs list different blocks" % (path, path))
        words[:, W_SEL:] = inputs
    return ends, words


_CAUSAL = [W_BITS] + list(range(W_SEL, W_BITS)) + list(range(NG)) + [W_P]


def first_difference(a, b):
    """a, b: (ends, words). None if the blocks both hold are equal (and equally many), else a dict: block, byte range [byte0, byte1), word, kind
    (word_name), a / b (the two values), words (every differing word of that block). Within the block the word named is the first in CAUSAL order,
    not in record order: the coded bits (the two streams differ), then the selectors, the column groups, the final p -- a changed input byte moves
    columns and p of the same block too, and what the reader wants named is the cause. One journal ending before the other: kind "length"."""
    ea, wa = a
    eb, wb = b
    wa = np.asarray(wa, np.uint64).reshape(-1, WORDS)
    wb = np.asarray(wb, np.uint64).reshape(-1, WORDS)
    n = min(len(ea), len(eb))
    for k in range(n):
        byte0 = int(ea[k - 1]) if k else 0
        if int(ea[k]) != int(eb[k]):
            return {"block": k, "byte0": byte0, "byte1": int(min(ea[k], eb[k])), "word": None, "kind": "end position", "a": int(ea[k]), "b": int(eb[k])}
        bad = np.flatnonzero(wa[k] != wb[k])
        if bad.size:
            bad = sorted((int(x) for x in bad), key=_CAUSAL.index)
            w = bad[0]
            return {"block": k, "byte0": byte0, "byte1": int(ea[k]), "word": w, "kind": word_name(w), "a": int(wa[k, w]), "b": int(wb[k, w]),
                    "words": [int(x) for x in bad]}
    if len(ea) != len(eb):
        return {"block": n, "byte0": int(ea[n - 1]) if n else 0, "byte1": None, "word": None, "kind": "length", "a": len(ea), "b": len(eb)}
    return None


def describe(d):
    if d is None:
        return "no difference"
    if d["kind"] == "length":
        return "the journals agree in their first %d block(s); one holds %d, the other %d" % (d["block"], d["a"], d["b"])
    if d["kind"] == "end position":
        return "block %d (from byte %d): ends at byte %d in one journal, %d in the other (different block sizes or lengths)" % (d["block"], d["byte0"], d["a"], d["b"])
    more = len(d["words"]) - 1
    return "first difference in block %d (bytes %d..%d): %s: %016x != %016x%s" % (
        d["block"], d["byte0"], d["byte1"] - 1, d["kind"], d["a"], d["b"],
        "" if not more else "; %d more word(s) of the block differ: %s" % (more, ", ".join(word_name(w) for w in d["words"][1:9]) + (" ..." if more > 8 else "")))


def main(argv):
    if len(argv) != 3 or argv[0] != "diff":
        print("usage: python -m cmix_amd.journal diff a b", file=sys.stderr)
        return 2
    a, b = read(argv[1]), read(argv[2])
    d = first_difference(a, b)
    print("compared %d block(s): %s" % (min(len(a[0]), len(b[0])), describe(d)))
    return 0 if d is None else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
