"""CPU: the stream journal's numpy model (cmix_amd/journal.py) against the line the UNMODIFIED reference's trace tool printed for the trace fixtures
(tests/golden/journal_ref_lines.npz, written by tests/golden/make_journal_golden.py from oracle/_ref/ref_long_trace), its algebra (sub-blocks add up,
one changed word moves one digest by a predictable amount, a word of all ones counts as 2^32), its files (round trip, first_difference, and
scripts/gpu_stage_hashes.py --compare reading them), and the host-side fold cmx_journal_host_digest against the model. The GPU tests
(test_gpu_journal.py) then hold the kernel to this model."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from cmix_amd import journal as J

M64 = (1 << 64) - 1


def _fixture(name):
    import make_golden as mg
    g = load_golden(name)
    return g, mg.unpack_probs(g)


@pytest.fixture(scope="module")
def ref_lines():
    with np.load(os.path.join(GOLDEN, "journal_ref_lines.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["text_96", "binary_64"])
def test_model_equals_reference_line(name, ref_lines):
    g, rows = _fixture(name)
    ends, words = J.digests(rows, g["sel"], g["bits"], g["p_final"])
    assert len(ends) == 1 and int(ends[0]) == int(ref_lines[name + "_end"]) == len(g["stream"])
    assert np.array_equal(words[0, :131], ref_lines[name + "_words"])   # 130 column groups, then the final p


@pytest.mark.parametrize("name", ["text_96", "binary_64"])
def test_small_blocks_add_up_to_the_reference_line(name, ref_lines):
    g, rows = _fixture(name)
    ends, words = J.digests(rows, g["sel"], g["bits"], g["p_final"], 0, 8)
    n = len(g["stream"])
    assert [int(e) for e in ends] == [min(32 * (i + 1), n) for i in range(-(-n // 32))]
    with np.errstate(over="ignore"):
        total = words.sum(0, dtype=np.uint64)
    assert np.array_equal(total[:131], ref_lines[name + "_words"])
    whole = J.digests(rows, g["sel"], g["bits"], g["p_final"])[1][0]
    assert np.array_equal(total, whole)   # the selector and bits words too


def test_one_flipped_bit_moves_one_word_by_a_known_amount():
    g, rows = _fixture("text_96")
    bit0, k = (1 << 19) - 300, 8   # blocks of 256 bits, B's index wraps inside the piece
    base = J.digests(rows, g["sel"], g["bits"], g["p_final"], bit0, k)[1]
    A = J.A()
    for t, c, mask in ((0, 0, 1), (299, 15, 1 << 31), (300, 16, 1 << 7), (767, 2077, 1 << 22), (555, 2064, 3)):
        r2 = rows.copy()
        u = r2.view(np.uint32)
        old = int(u[t, c])
        u[t, c] ^= np.uint32(mask)
        got = J.digests(r2, g["sel"], g["bits"], g["p_final"], bit0, k)[1]
        blk = ((bit0 + t) >> k) - (bit0 >> k)
        diff = np.argwhere(got != base)
        assert diff.tolist() == [[blk, c >> 4]]
        delta = (int(u[t, c]) - old) * int(A[c]) * int(J.B(bit0 + t)) & M64
        assert (int(got[blk, c >> 4]) - int(base[blk, c >> 4])) & M64 == delta


def test_all_ones_word_counts_as_two_to_the_32():
    rows = np.zeros((1, 2078), np.uint32)
    rows[0, 5] = 0xFFFFFFFF
    sel = np.full((1, 47), 0xFFFFFFFF, np.uint64)
    p = np.array([0xFFFFFFFF], np.uint32)
    _, w = J.digests(rows, sel, np.array([1], np.uint8), p, 7, 6)
    A, b = J.A(), int(J.B(7))
    assert int(w[0, 0]) == ((1 << 32) * int(A[5]) + sum(int(A[c]) for c in range(16) if c != 5)) * b & M64
    assert int(w[0, J.W_P]) == (1 << 32) * b & M64
    assert int(w[0, J.W_SEL + 46]) == (1 << 32) * b & M64
    assert int(w[0, J.W_BITS]) == 2 * b & M64
    assert int(w[0, 129]) == sum(int(A[c]) for c in range(2064, 2078)) * b & M64   # the last group has 14 columns


def test_none_leaves_words_zero():
    g, rows = _fixture("binary_64")
    _, w = J.digests(None, g["sel"], None, g["p_final"])
    assert not w[:, :130].any() and not w[:, J.W_BITS].any() and w[:, J.W_P].all() and w[:, J.W_SEL:J.W_BITS].all()


def test_write_read_round_trip_and_first_difference(tmp_path):
    g, rows = _fixture("text_96")
    a = J.digests(rows, g["sel"], g["bits"], g["p_final"], 0, 8)
    path = str(tmp_path / "a.txt")
    J.write(path, *a)
    ends, words = J.read(path)
    assert np.array_equal(ends, a[0]) and np.array_equal(words, a[1])
    assert len(open(path).readline().split()) == 132 and len(open(path + ".inputs").readline().split()) == 49
    assert J.first_difference(a, (ends, words)) is None
    for word, kind in ((J.W_BITS, "bits"), (J.W_P, "p"), (J.W_SEL + 12, "selector 12"), (27, "column group 27: cols 432..447 (fxcm .. paq8[13])")):
        w2 = a[1].copy()
        w2[1, word] ^= np.uint64(1)
        w2[1, J.W_P] ^= np.uint64(2)   # another word of the same block differs too
        w2[2, 0] ^= np.uint64(1)       # and a later block
        d = J.first_difference(a, (a[0], w2))
        assert (d["block"], d["byte0"], d["byte1"], d["word"], d["kind"]) == (1, 32, 64, word, kind)
    w2 = a[1].copy()   # the word named is the first in causal order: bits, selectors, column groups, p
    w2[1, [0, J.W_P, J.W_SEL + 3, J.W_BITS]] ^= np.uint64(1)
    order = []
    while (d := J.first_difference(a, (a[0], w2))) is not None:
        order.append(d["kind"].split(":")[0])
        w2[1, d["word"]] = a[1][1, d["word"]]
    assert order == ["bits", "selector 3", "column group 0", "p"]
    short = (a[0][:2], a[1][:2])
    assert J.first_difference(a, short)["kind"] == "length" and J.first_difference(a, short)["block"] == 2
    # the command line
    w2 = a[1].copy()
    w2[1, J.W_P] += np.uint64(5)
    J.write(str(tmp_path / "b.txt"), a[0], w2)
    same = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "diff", path, path], cwd=ROOT, capture_output=True, text=True)
    assert same.returncode == 0 and "no difference" in same.stdout
    diff = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "diff", path, str(tmp_path / "b.txt")], cwd=ROOT, capture_output=True, text=True)
    assert diff.returncode == 1 and "block 1 (bytes 32..63): p:" in diff.stdout


def test_stage_hashes_compare_reads_a_written_journal(tmp_path, ref_lines):
    """scripts/gpu_stage_hashes.py --compare and ref_long_trace's fourth argument read `path`: one line per 64 KB block, 131 words."""
    g, rows = _fixture("text_96")
    a = J.digests(rows, g["sel"], g["bits"], g["p_final"])
    mine, ref = str(tmp_path / "mine.txt"), str(tmp_path / "ref.txt")
    J.write(mine, *a)
    with open(ref, "w") as f:   # the reference's line as the tool prints it
        f.write("%d %s\n" % (int(ref_lines["text_96_end"]), " ".join("%016x" % int(x) for x in ref_lines["text_96_words"])))
    script = os.path.join(ROOT, "scripts", "gpu_stage_hashes.py")
    ok = subprocess.run([sys.executable, script, "--compare", mine, ref], capture_output=True, text=True)
    assert ok.returncode == 0 and "compared 1 blocks, groups 0..130: all digests equal" in ok.stdout, ok.stdout + ok.stderr
    w2 = a[1].copy()
    w2[0, 129] ^= np.uint64(1 << 40)
    J.write(mine, a[0], w2)
    bad = subprocess.run([sys.executable, script, "--compare", mine, ref], capture_output=True, text=True)
    assert "FIRST DIFFERENCE in block 0" in bad.stdout and "cols 2064..2077" in bad.stdout, bad.stdout + bad.stderr
    both = subprocess.run([sys.executable, script, "--compare", mine + ".inputs", mine + ".inputs", "0", "47"], capture_output=True, text=True)
    assert "all digests equal" in both.stdout   # the existing .inputs form


@pytest.mark.parametrize("bit0,k,n", [(0, 19, 768), (0, 8, 768), ((1 << 19) - 3, 6, 7), ((1 << 32) - 100, 8, 300), (5, 6, 1)])
def test_host_digest_equals_model(bit0, k, n):
    from cmix_amd import engine as E
    g, _ = _fixture("text_96")
    p, bits = g["p_final"][:n].copy(), g["bits"][:n].copy()
    p.view(np.uint32)[0] = 0xFFFFFFFF
    ends, pw, bw = E.journal_host_digest(p, bits, bit0, k)
    want_e, want = J.digests(None, None, bits, p, bit0, k)
    assert np.array_equal(ends, want_e) and np.array_equal(pw, want[:, J.W_P]) and np.array_equal(bw, want[:, J.W_BITS])
    _, pw2, bw2 = E.journal_host_digest(p, None, bit0, k)
    assert np.array_equal(pw2, pw) and not bw2.any()
    # pieces fold to the same words: a decoder adds a bit at a time
    acc = {}
    for a in range(0, n, 5):
        e, x, y = E.journal_host_digest(p[a:a + 5], bits[a:a + 5], bit0 + a, k)
        for i in range(len(e)):
            blk = ((bit0 + a) >> k) + i
            px, by = acc.get(blk, (0, 0))
            acc[blk] = ((px + int(x[i])) & M64, (by + int(y[i])) & M64)
    assert [acc[b][0] for b in sorted(acc)] == [int(v) for v in pw] and [acc[b][1] for b in sorted(acc)] == [int(v) for v in bw]
