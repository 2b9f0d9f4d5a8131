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

THE STATE JOURNAL (include/cmix_amd.h, "State digest"; the kernel is cmix_amd/csrc/state_digest.hip) is a file of its own: per record the stream's byte
position and one digest per state array of every device stage,

    D = sum over i of splitmix64((i << 32) | w[i])  (mod 2^64)  over the array's 32-bit words w[0..n),

behind header lines that carry the layout ("# col k stage region offset words"). state_digest() is the numpy model of D.

    python -m cmix_amd.journal state-diff a b    the first record in which two state journals differ: the byte range since the last equal record,
                                                 every differing column by stage, region and array, and per stage the first record at which it
                                                 differs at all (divergence spreads from stage to stage: the order is the finding)

This module is numpy only: digests() and state_digest() are the models the kernels are tested against, and need no GPU."""
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


# ---- the state journal ----
STATE_MAGIC = "# cmix_amd state journal 1"
STATE_STAGES = ["mixnet", "context", "LSTM", "fxcm", "paq8"]   # a column's stage number (cmx_pipeline_state_layout)
STATE_REGIONS = [   # a column's region number, per stage (include/cmix_amd.h: cmx_*_state_diff, "State digest")
    ["layer-0 rows", "layer-1 rows", "layer-2 rows", "row_steps", "map_keys", "map_vals", "s6", "s7", "x1", "x2", "scalar words"],
    ["CtxPersist", "history ring", "shared map", "bracket stack", "pred", "cnt", "chk", "Match map", "ihash"],
    ["W", "WT", "M", "Vv", "gb", "caches", "recurrent", "layer_input", "output_layer", "indices", "probs_rings", "host counters"],
    ["constant tables", "map buckets", "map StateMaps", "SSCM tables", "sm1_t", "rcm_t", "mhash", "sp_table", "buffer", "wx", "APM tables", "FxDev scalars"],
    ["ContextMap family", "ContextMap2", "lanes' learners", "DMC forest", "mixer", "tail / APM", "image families", "image lanes", "image mixer maps", "role structs' scalars"],
]


def state_digest(words):
    """D of an array of 32-bit words (any 4-byte dtype, taken as it lies): the model of cmx_state_digest_host and of the kernel."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(splitmix64((np.arange(len(w), dtype=np.uint64) << np.uint64(32)) | w).sum(dtype=np.uint64))


def state_term(i, w):
    """splitmix64((i << 32) | w): what word i with value w adds to D (a changed word moves D by state_term(i, w') - state_term(i, w) mod 2^64)."""
    return int(splitmix64(np.uint64((int(i) << 32) | (int(w) & 0xFFFFFFFF))))


def column_name(layout, c):
    """Column c of a layout [ncols, 4] (stage, region, offset, words) by stage, region name and array: the k-th array of its region, counted from 0."""
    st, rg, off, n = (int(x) for x in layout[c])
    k = sum(1 for j in range(c) if int(layout[j][0]) == st and int(layout[j][1]) == rg)
    stage = STATE_STAGES[st] if st < len(STATE_STAGES) else "stage %d" % st
    names = STATE_REGIONS[st] if st < len(STATE_REGIONS) else []
    return "%s region %d (%s) array %d (words %d..%d of the region)" % (stage, rg, names[rg] if rg < len(names) else "?", k, off, off + n - 1 if n else off)


def write_state(path, layout, pos, words):
    """The state journal's file: the header lines with the layout, then "<byte position> <one word of 16 hex digits per column>" per record."""
    layout = np.asarray(layout, np.uint64).reshape(-1, 4)
    words = np.asarray(words, np.uint64).reshape(-1, len(layout))
    with open(path, "w") as f:
        f.write("%s\n# columns %d\n" % (STATE_MAGIC, len(layout)))
        for c, l in enumerate(layout):
            f.write("# col %d %d %d %d %d\n" % (c, int(l[0]), int(l[1]), int(l[2]), int(l[3])))
        for e, w in zip(pos, words):
            f.write("%d%s\n" % (int(e), "".join(" %016x" % int(x) for x in w)))


def read_state(path):
    """(layout [ncols, 4], positions [nrecords], words [nrecords, ncols]). A truncated last line, as a killed run leaves it, is ignored."""
    with open(path) as f:
        text = f.read()
    lines = text.split("\n")
    whole = lines[:-1]          # every line that ends in a newline; what a killed run left behind the last newline (lines[-1]) is no record
    if not whole or whole[0].strip() != STATE_MAGIC:
        raise ValueError("%s: not a state journal (its first line is not %r)" % (path, STATE_MAGIC))
    ncols, layout, pos, rows = None, [], [], []
    for i, line in enumerate(whole[1:], 2):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "#":
            if len(tok) == 3 and tok[1] == "columns":
                ncols = int(tok[2])
            elif len(tok) == 7 and tok[1] == "col":
                if int(tok[2]) != len(layout):
                    raise ValueError("%s: line %d: column %s listed out of order" % (path, i, tok[2]))
                layout.append([int(x) for x in tok[3:7]])
            continue
        if ncols is None or len(layout) != ncols:
            raise ValueError("%s: line %d: a record before the layout is complete" % (path, i))
        if len(tok) != 1 + ncols or any(len(x) != 16 for x in tok[1:]):
            raise ValueError("%s: line %d: %d words, expected %d of 16 hex digits" % (path, i, len(tok) - 1, ncols))
        pos.append(int(tok[0]))
        rows.append([int(x, 16) for x in tok[1:]])
    if ncols is None or len(layout) != ncols:
        raise ValueError("%s: the header lists %d of %s columns" % (path, len(layout), ncols))
    return np.array(layout, np.uint64).reshape(-1, 4), np.array(pos, np.uint64), np.array(rows, np.uint64).reshape(-1, ncols)


def first_state_difference(a, b):
    """a, b: (layout, positions, words). Raises ValueError if the layouts differ. None if the records both hold are equal (and equally many), else a
    dict: record, byte range (byte0, byte1] = since the last equal record, kind ("state", "position" or "length"), columns (every differing column of
    that record), names (column_name of each), a / b (the first of them in the two files), stages: per stage that differs anywhere, in the order in
    which they first do, (stage name, first record, its byte position)."""
    la, pa, wa = a
    lb, pb, wb = b
    la = np.asarray(la, np.uint64).reshape(-1, 4)
    lb = np.asarray(lb, np.uint64).reshape(-1, 4)
    if la.shape != lb.shape or not np.array_equal(la, lb):
        raise ValueError("the two state journals have different layouts (%d and %d columns): other stages enabled, another vocabulary or another build" % (len(la), len(lb)))
    wa = np.asarray(wa, np.uint64).reshape(-1, len(la))
    wb = np.asarray(wb, np.uint64).reshape(-1, len(la))
    n = min(len(pa), len(pb))
    apart = np.flatnonzero(np.asarray(pa[:n], np.uint64) != np.asarray(pb[:n], np.uint64))
    m = int(apart[0]) if apart.size else n   # records [0, m) were taken at the same positions
    for k in range(n):
        byte0 = int(pa[k - 1]) if k else 0
        if int(pa[k]) != int(pb[k]):
            return {"record": k, "byte0": byte0, "byte1": int(min(pa[k], pb[k])), "kind": "position", "a": int(pa[k]), "b": int(pb[k])}
        bad = np.flatnonzero(wa[k] != wb[k])
        if bad.size:
            stages = []
            for st in sorted(set(int(x) for x in la[:, 0])):
                cols = np.flatnonzero(la[:, 0] == np.uint64(st))
                hit = np.flatnonzero((wa[k:m][:, cols] != wb[k:m][:, cols]).any(axis=1))
                if hit.size:
                    r = k + int(hit[0])
                    stages.append((STATE_STAGES[st] if st < len(STATE_STAGES) else "stage %d" % st, r, int(pa[r])))
            stages.sort(key=lambda s: s[1])
            c = int(bad[0])
            return {"record": k, "byte0": byte0, "byte1": int(pa[k]), "kind": "state", "columns": [int(x) for x in bad], "names": [column_name(la, int(x)) for x in bad],
                    "a": int(wa[k, c]), "b": int(wb[k, c]), "stages": stages}
    if len(pa) != len(pb):
        return {"record": n, "byte0": int(pa[n - 1]) if n else 0, "byte1": None, "kind": "length", "a": len(pa), "b": len(pb)}
    return None


def describe_state(d):
    if d is None:
        return "no difference"
    if d["kind"] == "length":
        return "the state journals agree in their first %d record(s); one holds %d, the other %d" % (d["record"], d["a"], d["b"])
    if d["kind"] == "position":
        return "record %d (after byte %d): taken at byte %d in one journal, %d in the other (different periods or chunk sizes)" % (d["record"], d["byte0"], d["a"], d["b"])
    out = ["first difference in record %d: the state changed differently in bytes %d..%d (the last equal record is %s)" % (
        d["record"], d["byte0"], d["byte1"] - 1, "record %d" % (d["record"] - 1) if d["record"] else "none: the files differ from their first record")]
    out.append("%d column(s) of that record differ:" % len(d["columns"]))
    for c, nm in zip(d["columns"], d["names"]):
        out.append("  column %d: %s" % (c, nm))
    out.append("the first of them: %016x != %016x" % (d["a"], d["b"]))
    out.append("per stage, the first record at which it differs at all:")
    for nm, r, at in d["stages"]:
        out.append("  %-8s record %d (byte %d)" % (nm, r, at))
    return "\n".join(out)


def main(argv):
    if len(argv) == 3 and argv[0] == "state-diff":
        a, b = read_state(argv[1]), read_state(argv[2])
        try:
            d = first_state_difference(a, b)
        except ValueError as e:
            print("state-diff: %s" % e, file=sys.stderr)
            return 2
        print("compared %d record(s) of %d column(s): %s" % (min(len(a[1]), len(b[1])), len(a[0]), describe_state(d)))
        return 0 if d is None else 1
    if len(argv) != 3 or argv[0] != "diff":
        print("usage: python -m cmix_amd.journal diff a b\n       python -m cmix_amd.journal state-diff a b", file=sys.stderr)
        return 2
    a, b = read(argv[1]), read(argv[2])
    d = first_difference(a, b)
    print("compared %d block(s): %s" % (min(len(a[0]), len(b[0])), describe(d)))
    return 0 if d is None else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
