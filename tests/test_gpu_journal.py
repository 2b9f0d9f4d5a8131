"""GPU: the stream journal (cmix_amd/csrc/journal.hip; include/cmix_amd.h "Stream journal") against its numpy model (cmix_amd/journal.py, pinned on the
unmodified reference's trace line by test_journal_model.py): the stand-alone handle at the smallest shapes where the kernel can go wrong, then the
journal of the whole pipeline on the trace fixtures -- every block's column-group, p, selector and bits words against the reference's rows, and the
blocks adding up to the line the reference's own tool printed (tests/golden/journal_ref_lines.npz)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, bits_equal, load_golden, synth_mixnet_inputs
from cmix_amd import journal as J

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
T_MAX = 300   # five workgroups of 64 rows, the last one ragged


@pytest.fixture(scope="module")
def synth():
    """One seeded set of mixing-network inputs, shared and never written: host arrays and their device copies."""
    import torch
    probs, sel, bits = synth_mixnet_inputs(T_MAX, seed=7)
    sel32 = (sel & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    p = np.random.default_rng(8).random(T_MAX, dtype=np.float32)
    dev = dict(rows=torch.from_numpy(probs).cuda(), sel=torch.from_numpy(sel32.view(np.int32)).cuda(), bits=torch.from_numpy(bits).cuda(), p=torch.from_numpy(p).cuda())
    return dict(rows=probs, sel=sel32, bits=bits, p=p), dev


def _run(dev, T, bit0, k, rows="rows", parts=("rows", "sel", "bits", "p"), pieces=None):
    from cmix_amd import engine as E
    j = E.Journal(0, k)
    try:
        edges = [0, T] if not pieces else sorted(set([0, T] + list(pieces)))
        for a, b in zip(edges[:-1], edges[1:]):
            arg = {n: (dev[rows if n == "rows" else n][a:b] if n in parts else None) for n in ("rows", "sel", "bits", "p")}
            j.run(arg["rows"], arg["sel"], arg["bits"], arg["p"], bit0 + a)
        return j.read()
    finally:
        j.close()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    bad = np.argwhere(got[1] != want[1])
    assert len(bad) == 0, "block %d, %s differs (%d words differ)" % (bad[0][0], J.word_name(int(bad[0][1])), len(bad))


@pytest.mark.parametrize("T,k,bit0", [(1, 19, 0), (7, 6, (1 << 19) - 3), (300, 8, (1 << 32) - 100), (300, 19, 5)],
                         ids=["one_bit", "block_edge_and_B_wrap", "64_bit_positions", "five_workgroups_one_block"])
def test_handle_equals_model(synth, T, k, bit0):
    host, dev = synth
    _same(_run(dev, T, bit0, k), J.digests(host["rows"][:T], host["sel"][:T], host["bits"][:T], host["p"][:T], bit0, k))


def test_row_stride_2080(synth):
    """ld = 2078 (above) and a wider matrix whose rows are 16-byte aligned: the same words"""
    import torch
    host, dev = synth
    wide = torch.full((T_MAX, 2080), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :2078] = dev["rows"]
    d2 = dict(dev, wide=wide[:, :2078])
    assert d2["wide"].stride(0) == 2080
    _same(_run(d2, T_MAX, 11, 7, rows="wide"), J.digests(host["rows"], host["sel"], host["bits"], host["p"], 11, 7))


def test_two_runs_equal_one(synth):
    """consecutive runs accumulate: cut inside a block, at a block edge and inside a workgroup's 64 rows; a run that does not continue is refused"""
    from cmix_amd import engine as E
    host, dev = synth
    whole = _run(dev, T_MAX, 100, 6)
    _same(_run(dev, T_MAX, 100, 6, pieces=[1, 28, 130, 131]), whole)   # (bit 100 + 28 = 128 is a block edge)
    _same(whole, J.digests(host["rows"], host["sel"], host["bits"], host["p"], 100, 6))
    j = E.Journal(0, 6)
    j.run(None, None, dev["bits"][:10], None, 0)
    with pytest.raises(E.CmxError, match="does not continue"):
        j.run(None, None, dev["bits"][:10], None, 11)
    j.close()


@pytest.mark.parametrize("parts", [("rows",), ("sel", "bits"), ("p",), ("rows", "p")])
def test_null_pointer_leaves_its_words_zero(synth, parts):
    host, dev = synth
    want = J.digests(*[host[n][:70] if n in parts else None for n in ("rows", "sel", "bits", "p")], 3, 6)
    got = _run(dev, 70, 3, 6, parts=parts)
    _same(got, want)
    assert bool(got[1][:, :130].any()) == ("rows" in parts) and bool(got[1][:, J.W_P].any()) == ("p" in parts)
    assert bool(got[1][:, J.W_SEL:J.W_BITS].any()) == ("sel" in parts) and bool(got[1][:, J.W_BITS].any()) == ("bits" in parts)


def test_extreme_words():
    """0xFFFFFFFF (+ 1 needs 33 bits; the LDS-poison pattern) and 0x80000000 in rows, selectors and p"""
    import torch
    T = 67
    rows = np.full((T, 2078), 0xFFFFFFFF, np.uint32)
    rows[::2] = 0x80000000
    rows[5, 2077] = 0
    sel = np.full((T, 47), 0xFFFFFFFF, np.uint32)
    p = np.full(T, 0xFFFFFFFF, np.uint32)
    bits = np.full(T, 255, np.uint8)
    dev = dict(rows=torch.from_numpy(rows.view(np.int32)).cuda().view(torch.float32), sel=torch.from_numpy(sel.view(np.int32)).cuda(),
               bits=torch.from_numpy(bits).cuda(), p=torch.from_numpy(p.view(np.int32)).cuda().view(torch.float32))
    want = J.digests(rows, sel, bits, p, 60, 6)
    _same(_run(dev, T, 60, 6), want)
    assert int(want[1][0, J.W_P]) == sum((1 << 32) * int(J.B(60 + i)) for i in range(4)) & M64   # (block 0 holds bits 60..63)


@pytest.mark.parametrize("col", [0, 2077])
def test_one_flipped_bit_moves_one_word(synth, col):
    """one bit flipped ON THE DEVICE, in the first column and in the last (the 14-column group 129): exactly one word changes, by delta * A[c] * B[t]"""
    host, dev = synth
    bit0, k, t, mask = (1 << 19) - 100, 6, 171, 1 << 23
    base = _run(dev, T_MAX, bit0, k)
    rows = dev["rows"].clone()
    word = rows.view(__import__("torch").int32)
    word[t, col] ^= mask
    got = _run(dict(dev, flipped=rows), T_MAX, bit0, k, rows="flipped")
    blk = ((bit0 + t) >> k) - (bit0 >> k)
    assert np.argwhere(got[1] != base[1]).tolist() == [[blk, col >> 4]]
    old = int(host["rows"].view(np.uint32)[t, col])
    delta = ((old ^ mask) - old) * int(J.A()[col]) * int(J.B(bit0 + t)) & M64
    assert (int(got[1][blk, col >> 4]) - int(base[1][blk, col >> 4])) & M64 == delta


def test_bad_arguments(synth):
    from cmix_amd import engine as E
    _, dev = synth
    for k in (5, 20):
        with pytest.raises(E.CmxError, match="6..19"):
            E.Journal(0, k)
    j = E.Journal(0, 8)
    with pytest.raises(E.CmxError, match="8-byte"):
        j.run(dev["rows"].view(-1)[1:1 + 2 * 2078].view(2, 2078), None, None, None, 0)   # rows at an odd float
    assert j.blocks() == 0
    j.close()


# ---- the whole pipeline ---------------------------------------------------------------------------------------------------------------------------

def _pipeline(g, chunks, k, journal=True):
    """fxcm and paq8 on the device: every one of the 2078 columns is the engine's. Returns (journal, p)."""
    import torch
    from cmix_amd import engine as E
    stream = np.ascontiguousarray(g["stream"])
    n = len(stream)
    edges = [0, n] if not chunks else sorted(set([0, n] + list(chunks)))
    pipe = E.Pipeline(g["vocab"], 0, max(b - a for a, b in zip(edges[:-1], edges[1:])))
    try:
        pipe.enable_fxcm(None)
        pipe.enable_paq8()
        if journal:
            pipe.set_journal(k)
        l0 = torch.full((8 * n, E.N_INPUTS), -1.0, dtype=torch.float32, device="cuda")
        p = torch.empty(8 * n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for a, b in zip(edges[:-1], edges[1:]):
            pipe.submit(stream[a:b], l0[8 * a:8 * b], p[8 * a:8 * b])
        pipe.sync()
        return (pipe.journal() if journal else None), p.cpu().numpy()
    finally:
        pipe.close()


def _slot_selectors(g):
    """What the slot holds of the reference's 47 selectors: their low 32 bits, except index 12 -- the auxiliary context, which the mixing network
    forms itself from three of the bit's inputs (as tests/test_gpu_late.py notes): the context stage writes 0 there (tests/test_gpu_ctxmodels.py), and
    reading the kernel shows it keeps that key in its own record, never in the slot. So word 12 is the model's on a column of zeros."""
    s = (g["sel"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    s[:, 12] = 0
    return s


@pytest.mark.parametrize("name,chunks", [("text_96", [1, 32]), ("binary_64", None)], ids=["text_96_chunks_1_31_64", "binary_64_in_one"])
def test_pipeline_journal_equals_reference(name, chunks):
    import make_golden as mg
    g = load_golden(name)
    k = 8
    (ends, words), p = _pipeline(g, chunks, k)
    assert bits_equal(p, g["p_final"]).all()
    want_e, want = J.digests(mg.unpack_probs(g), _slot_selectors(g), g["bits"], g["p_final"], 0, k)
    assert np.array_equal(ends, want_e)
    for lo, hi, what in ((0, 131, "the 130 column groups and p"), (J.W_BITS, J.WORDS, "bits"), (J.W_SEL, J.W_BITS, "selectors")):
        bad = np.argwhere(words[:, lo:hi] != want[:, lo:hi])
        assert len(bad) == 0, "%s: block %d, %s" % (what, bad[0][0], J.word_name(lo + int(bad[0][1])))
    with np.load(os.path.join(GOLDEN, "journal_ref_lines.npz")) as z:   # the line the reference's own tool printed for this stream
        line = z[name + "_words"]
    with np.errstate(over="ignore"):
        assert np.array_equal(words.sum(0, dtype=np.uint64)[:131], line)


def test_more_chunks_than_slots_and_p_unchanged():
    """2048 bytes in 100-byte chunks through EngineStream(journal=8): 21 chunks, the slots' partial records come round more than twice; the journal
    matches the fixture's p, selectors and bits (it has no rows), and p is bit-identical to a run with the journal off"""
    from cmix_amd import engine as E
    from cmix_amd.pipeline import EngineStream
    g = load_golden("text_2k_nofull")
    n, k = len(g["stream"]), 8
    assert -(-n // 100) > E.PIPELINE_SLOTS
    ps, jr = [], None
    for journal in (k, 0):
        eng = EngineStream(0, g["stream"], sub_chunk=100, vocab=g["vocab"], journal=journal)
        try:
            eng.feed(n)
            eng.finish()
            ps.append(eng.p_dev.cpu().numpy())
            if journal:
                jr = eng.journal()
            else:
                with pytest.raises(E.CmxError, match="journal is off"):
                    eng.journal()
        finally:
            eng.close()
    assert np.array_equal(ps[0].view(np.uint32), ps[1].view(np.uint32))
    assert bits_equal(ps[0], g["p_final"]).all()
    want_e, want = J.digests(None, _slot_selectors(g), g["bits"], g["p_final"], 0, k)
    assert np.array_equal(jr[0], want_e) and len(want_e) == n // 32
    for lo, hi in ((J.W_P, J.W_P + 1), (J.W_SEL, J.W_BITS), (J.W_BITS, J.WORDS)):
        assert np.array_equal(jr[1][:, lo:hi], want[:, lo:hi]), J.word_name(lo)
    assert jr[1][:, :130].all()   # (the column groups are digested too; the fixture holds no rows to compare them with)


def test_two_streams_differing_in_one_byte():
    g = load_golden("text_96")
    k, at = 8, 70   # blocks of 32 bytes: byte 70 lies in block 2
    other = dict(g, stream=g["stream"].copy())
    other["stream"][at] ^= 0x20
    a, _ = _pipeline(g, [40], k)
    b, _ = _pipeline(other, [40], k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][:2], b[1][:2])
    d = J.first_difference(a, b)
    assert (d["block"], d["byte0"], d["byte1"], d["kind"]) == (2, 64, 96, "bits")
    assert J.W_P in d["words"]


def _synthetic_pipeline(shadow, repair, journal):
    """as tests/test_gpu_shadow_repair.py: a bare Pipeline over 7 chunks of 256 synthetic text bytes, columns 3..2024 a seeded grid of the caller's"""
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    n_chunk, n_chunks = 256, 7
    data = np.frombuffer(S.enwik_like(n_chunks * n_chunk, 21), np.uint8)
    cols = (np.random.default_rng(8).integers(1, 4095, (8 * n_chunks * n_chunk, 2078)).astype(np.float32) * np.float32(1.0 / 4095)).astype(np.float32)
    layer0 = torch.from_numpy(cols).cuda()
    p = torch.full((8 * n_chunks * n_chunk,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=n_chunk)
    pipe.set_journal(journal)
    if shadow:
        pipe.set_shadow(shadow)
    if repair:
        pipe.set_shadow_repair(repair)

    def submit(i):
        a, b = i * n_chunk, (i + 1) * n_chunk
        pipe.submit(data[a:b].tobytes(), layer0[8 * a:8 * b], p[8 * a:8 * b])
    return pipe, p, submit


def test_a_repaired_chunks_journal_describes_the_p_that_is_coded():
    """The xor hook of test_gpu_shadow_repair.py in the stream's own network (instance 0) while chunks 3..5 are in flight: the repair replaces their p with
    the majority's AFTER the journal kernel ran behind the outvoted network. The journal must nevertheless equal, word for word, that of an unperturbed
    run (and p too): the repaired chunks' records are taken again before they are folded. Blocks of 2^9 bits: four per chunk."""
    from cmix_amd import engine as E
    k = 9
    pipe, p, submit = _synthetic_pipeline(0, 0, k)
    try:
        for i in range(7):
            submit(i)
        pipe.sync()
        want, want_p = pipe.journal(), p.cpu().numpy().copy()
    finally:
        pipe.close()
    pipe, p, submit = _synthetic_pipeline(2, 2, k)
    try:
        pipe.set_journal(0)      # off and on again before the first chunk, beside armed repair
        pipe.set_journal(k)
        with pytest.raises(E.CmxError, match="0 \\(off\\) or 6..19"):
            pipe.set_journal(5)
        for i in range(3):
            submit(i)
            pipe.wait(i)
        pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, 0x00400000)   # mixer 26's row 0 is used by every bit (test_gpu_shadow_repair.py)
        for i in (3, 4, 5):
            submit(i)
        for i in (3, 4, 5):
            pipe.wait(i)
        rep = pipe.shadow_repairs()
        assert rep["total"] == 1 and rep["log"][0]["odd"] == 0 and rep["log"][0]["chunk"] == 3
        submit(6)
        pipe.wait(6)
        pipe.sync()
        assert bits_equal(p.cpu().numpy(), want_p).all()
        got = pipe.journal()
        assert J.first_difference(want, got) is None, J.describe(J.first_difference(want, got))
    finally:
        pipe.close()
