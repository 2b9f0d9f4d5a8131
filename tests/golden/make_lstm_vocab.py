#!/usr/bin/env python3
"""The LSTM byte mixer of the UNMODIFIED reference across vocabulary sizes (tests/golden/lstm_vocab_sweep.npz, 0.7 MB).

Every size of the LSTM stage is a function of the vocabulary size V (rowlen = insz + V, lstm_wt_index, the LDS carve-up of
cmx_lstm_fwdblk, the grid of cmx_lstm_bptt_acc, head and tail of every ordered chain in lds_chain); the other golden traces
have V = 256. For each V of VOCABS the reference predictor (oracle/refharness.py, one child process per vocabulary: the harness
holds one predictor per process) codes a seeded stream of N = 230 bytes over a seeded, non-contiguous vocabulary, and this is
recorded (keys carry V):

    vocab_V   [256]   u8   the vocabulary mask
    stream_V  [N]     u8   bytes 0..99 draw from the lower half of the vocabulary's symbols only (V = 1: nothing to split), so
                           the upper half's one-hot columns get their first non-zero gradient in the round at byte 200; a few
                           short repeats make the softmax peaked
    ppmd_V    [N,V]   f32  the reference's PPMd distribution after each byte (the LSTM's input), vocabulary columns in byte order
    lstm_V    [N,V]   f32  the LSTM byte mixer's distribution after each byte, likewise
                           (both are exactly zero outside the vocabulary -- asserted here -- so expand() loses nothing)
    bitp_V    [N,8]   f32  the byte mixer's Predict value of every bit (layer-0 input 2077)
    ex_V      [N,8]   u8   ByteModel::ex after that Predict and before the bit's Perceive (byte-model.cpp:13-20)
    wsha_V    [6]     S64  SHA-256 of the six gate weight matrices after byte N - 1, reference layout [200][rowlen], index
                           3 * layer + gate

What each V exercises (C = 200 cells; insz % 4 == (V + 1) % 4 in both layers; RO = ceil(V / 8) rows per output workgroup):

      V  V%4 (V+1)%4 V%8  fb_out_wg: workgroups x rows            lds_chain [0,V)        p1_chain
      1   1     2     1   1 x 1, seven with nr == 0               scalar tail only       tail only
      2   2     3     2   2 x 1, six with nr == 0                 scalar tail only       tail only
      5   1     2     5   5 x 1, three with nr == 0               1 quad (< 4) + tail    tail only
      9   1     2     1   4 x 2, one partial (1), three nr == 0   2 quads (< 4) + tail   loop + tail
     14   2     3     6   7 x 2, one with nr == 0                 3 quads (< 4) + tail   loop + tail
     17   1     2     1   5 x 3, one partial (2), two nr == 0     4 quads (4..7) + tail  loop + tail
     31   3     0     7   7 x 4, one partial (3)                  7 quads (4..7) + tail  loop + tail
     32   0     1     0   8 x 4, all full                         8 quads (loop)         loop only
     62   2     3     6   7 x 8, one partial (6)                  15 quads (loop) + tail loop + tail
     65   1     2     1   7 x 9, one partial (2)                  16 quads (loop) + tail loop + tail
    127   3     0     7   7 x 16, one partial (15)                31 quads (loop) + tail loop + tail
    201   1     2     1   7 x 26, one partial (19)                50 quads (loop) + tail loop + tail
    250   2     3     2   7 x 32, one partial (26)                62 quads (loop) + tail loop + tail
    255   3     0     7   7 x 32, one partial (31)                63 quads (loop) + tail loop + tail

(V % 4 is also where the segments [V, V+C) and [V+C, insz) of a gate row begin inside a quad; (V+1) % 4 is fb_gate_wg's
trailing partial quad `rem`; V % 16 and V % 64 place the one-hot / dense split inside a tile of cmx_lstm_bptt_acc(_mfma).)
V = 1 checks layout and indexing only: the softmax of one logit is exactly 1, so the error vector is identically zero, no weight
ever moves and a wrong operand in a BPTT chain cannot show there; V = 2 and V = 5 are the tail-only cases where it can.
check_classes() asserts that VOCABS covers every class, so that an edit of the list cannot silently lose one.

The file is written with fixed member dates (save_npz), so a second run gives the same file byte for byte.

    python tests/golden/make_lstm_vocab.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

VOCABS = [1, 2, 5, 9, 14, 17, 31, 32, 62, 65, 127, 201, 250, 255]
N = 230
WITH_0_AND_255 = (2, 9, 17, 32, 65, 201, 255)   # vocabularies forced to hold byte 0 and byte 255 (byte_map / sym2byte)
NAME = "lstm_vocab_sweep"
MAX_FILE = 1 << 20   # a committed file stays below 1 MiB


def quad_path(V):
    """lds_chain over the symbol segment [0, V): by the number of whole quads"""
    nq = V >> 2
    return "lt4" if nq < 4 else "4to7" if nq < 8 else "loop"


def p1_path(V):
    return "tail" if V < 8 else "loop" if V % 8 == 0 else "loop+tail"


def out_rows(V):
    """rows of the eight output workgroups (fb_out_wg)"""
    ro = (V + 7) // 8
    return [max(0, min(ro, V - w * ro)) for w in range(8)]


def check_classes(vocabs=VOCABS):
    assert {v % 4 for v in vocabs} == {0, 1, 2, 3}, "V % 4"
    assert {(v + 1) % 4 for v in vocabs} == {0, 1, 2, 3}, "(V + 1) % 4: fb_gate_wg's trailing columns"
    assert {quad_path(v) for v in vocabs} == {"lt4", "4to7", "loop"}, "lds_chain quad-count paths"
    assert {p1_path(v) for v in vocabs} == {"tail", "loop", "loop+tail"}, "p1_chain"
    kinds = set()
    for v in vocabs:
        ro = (v + 7) // 8
        rows = out_rows(v)
        assert sum(rows) == v
        kinds |= {"zero" if r == 0 else "full" if r == ro else "partial" for r in rows}
        if all(r == ro for r in rows):
            kinds.add("all full")
    assert kinds == {"zero", "partial", "full", "all full"}, "fb_out_wg row split"
    assert any(v % 16 and v < 64 for v in vocabs) and any(v % 64 for v in vocabs), "one-hot / dense split inside a tile"


def vocab_and_stream(V):
    rng = np.random.default_rng(7000 + V)
    forced = [0, 255] if V in WITH_0_AND_255 else []
    rest = [b for b in range(256) if b not in forced]
    syms = np.sort(np.concatenate([np.array(forced, np.int64), rng.choice(rest, V - len(forced), replace=False)])).astype(np.uint8)
    assert len(set(syms.tolist())) == V
    vocab = np.zeros(256, np.uint8)
    vocab[syms] = 1
    lower = syms[:max(1, V // 2)]
    stream = np.concatenate([rng.choice(lower, 100), rng.choice(syms, N - 100)]).astype(np.uint8)
    if V > 1:   # up to 40 distinct symbols of the upper half are placed behind byte 100, whatever the draw gave
        upper = syms[V // 2:]
        at = 100 + rng.permutation(N - 100)[:min(len(upper), 40)]
        stream[at] = rng.permutation(upper)[:len(at)]
    for dst, src, n in ((20, 12, 8), (60, 48, 12), (140, 124, 16), (200, 190, 10)):   # short repeats
        stream[dst:dst + n] = stream[src:src + n]
    assert vocab[stream].all() and np.isin(stream[:100], lower).all()
    return vocab, stream


def expand(cols, vocab):
    """[N,V] vocabulary columns -> [N,256] rows, zero outside the vocabulary"""
    out = np.zeros((len(cols), 256), np.float32)
    out[:, np.flatnonzero(vocab)] = cols
    return out


def trace(V):
    from oracle import refharness as R
    vocab, stream = vocab_and_stream(V)
    r = R.Ref(vocab)
    d = r.lstm_dims()
    assert d["output_size"] == V and d["cells"] == 200 and d["layers"] == 2 and d["horizon"] == 100, d
    ppmd = np.empty((N, 256), np.float32)
    lstm = np.empty((N, 256), np.float32)
    bitp = np.empty((N, 8), np.float32)
    ex = np.empty((N, 8), np.int64)
    for n, byte in enumerate(stream):
        for k in range(8):
            r.predict()
            bitp[n, k] = r.model_probs()[2077]
            ex[n, k] = r.byte_probs(1)[1][2]
            r.perceive((int(byte) >> (7 - k)) & 1)
        ppmd[n] = r.byte_probs(0)[0]
        lstm[n] = r.byte_probs(1)[0]
    on = np.flatnonzero(vocab)
    off = np.flatnonzero(vocab == 0)
    assert not ppmd[:, off].any() and not lstm[:, off].any(), "a distribution is non-zero outside the vocabulary"
    assert ex.min() >= 0 and ex.max() <= 255
    wsha = []
    for layer in range(2):
        assert r.lib.ref_lstm_gate_row_len(layer) == (1 + 200 + V if layer == 0 else 1 + 400 + V) + V
        for gate in range(3):
            wsha.append(hashlib.sha256(np.ascontiguousarray(r.lstm_gate_weights(layer, gate)).tobytes()).hexdigest())
    return {"vocab_%d" % V: vocab, "stream_%d" % V: stream, "ppmd_%d" % V: np.ascontiguousarray(ppmd[:, on]),
            "lstm_%d" % V: np.ascontiguousarray(lstm[:, on]), "bitp_%d" % V: bitp, "ex_%d" % V: ex.astype(np.uint8),
            "wsha_%d" % V: np.array(wsha, "S64")}


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same file, byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def load_sweep():
    """{V: dict(vocab, stream, ppmd [N,256], lstm [N,256], bitp, ex, wsha)} from the committed file. A missing file FAILS the caller
    (conftest.load_golden would skip, hence the check of the path first)."""
    from conftest import GOLDEN, load_golden
    path = os.path.join(GOLDEN, NAME + ".npz")
    assert os.path.exists(path), "%s is missing: regenerate it with tests/golden/make_lstm_vocab.py" % path
    g = load_golden(NAME)
    out = {}
    for V in VOCABS:
        c = {k: g["%s_%d" % (k, V)] for k in ("vocab", "stream", "ppmd", "lstm", "bitp", "ex", "wsha")}
        c["ppmd"], c["lstm"] = expand(c["ppmd"], c["vocab"]), expand(c["lstm"], c["vocab"])
        c["wsha"] = [s.decode() for s in c["wsha"]]
        out[V] = c
    return out


if __name__ == "__main__":
    check_classes()
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        np.savez(sys.argv[3], **trace(int(sys.argv[2])))
        sys.exit(0)
    import tempfile
    from oracle import refharness as R
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for V in VOCABS:
            path = os.path.join(tmp, "v%d.npz" % V)
            R.run_in_subprocess(os.path.abspath(__file__), "--child", V, path)
            with np.load(path) as z:
                out.update({k: z[k] for k in z.files})
    dst = os.path.join(HERE, NAME + ".npz")
    save_npz(dst, out)
    size = os.path.getsize(dst)
    assert size < MAX_FILE, (dst, size)
    print("wrote", dst, size, "bytes, sha256", hashlib.sha256(open(dst, "rb").read()).hexdigest())
