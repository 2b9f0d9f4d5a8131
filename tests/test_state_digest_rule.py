"""CPU: the state digest's rule (include/cmix_amd.h, "State digest"): cmx_state_digest_host through ctypes against the numpy restatement in
cmix_amd/journal.py, the algebra the GPU tests rely on (one changed word moves the digest by splitmix64(i, w') - splitmix64(i, w); position matters),
and the state journal's file: round trip, first_state_difference, the per-stage firsts, a truncated last line, a layout mismatch, and the state-diff
command line without torch in its process. No device is touched. The GPU tests (test_gpu_state_digest.py) then hold the kernel to this model."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from cmix_amd import journal as J

M64 = (1 << 64) - 1
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, (1 << 16) + 3]


def _mix(x):   # splitmix64 in Python integers: the formula restated once more, independent of numpy's wrapping
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _words(n, fill, seed=7):
    if fill == "random":
        return np.random.default_rng(seed + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.full(n, 0 if fill == "zero" else 0xFFFFFFFF, np.uint32)


@pytest.mark.parametrize("fill", ["random", "zero", "ones"])
@pytest.mark.parametrize("n", LENGTHS)
def test_host_form_equals_the_formula(n, fill):
    from cmix_amd import engine as E
    w = _words(n, fill)
    want = J.state_digest(w)
    assert E.state_digest_host(w) == want
    if n <= 257:   # and numpy's restatement equals plain integer arithmetic
        assert want == sum(_mix((i << 32) | int(x)) for i, x in enumerate(w)) & M64
    assert J.state_digest(w.view(np.float32)) == want   # (words are taken as they lie)


def test_term_is_the_formula():
    for i, w in ((0, 0), (1, 0xFFFFFFFF), ((1 << 32) - 1, 0x80000000), (12345, 678)):
        assert J.state_term(i, w) == _mix((i << 32) | w)


@pytest.mark.parametrize("n", [1, 5, 257, (1 << 16) + 3])
def test_one_changed_word_moves_the_digest_by_the_predicted_amount(n):
    from cmix_amd import engine as E
    w = _words(n, "random", 11)
    base = E.state_digest_host(w)
    for i in sorted({0, n // 2, n - 1}):
        for new in (0, 0xFFFFFFFF, int(w[i]) ^ 1, int(w[i]) ^ (1 << 31)):
            if new == int(w[i]):
                continue
            v = w.copy()
            v[i] = new
            got = E.state_digest_host(v)
            assert got != base   # splitmix64 is a bijection: a single changed word always shows
            assert (got - base) & M64 == (J.state_term(i, new) - J.state_term(i, int(w[i]))) & M64
            assert J.state_digest(v) == got


def test_swapping_two_unequal_words_changes_the_digest():
    from cmix_amd import engine as E
    for n, (a, b) in ((2, (0, 1)), (257, (3, 256)), ((1 << 16) + 3, (0, 1 << 16))):
        w = _words(n, "random", 3)
        w[b] = w[a] ^ np.uint32(1)
        v = w.copy()
        v[a], v[b] = w[b], w[a]
        assert E.state_digest_host(v) != E.state_digest_host(w) and J.state_digest(v) != J.state_digest(w)
    assert J.state_digest(np.array([1, 2], np.uint32)) != J.state_digest(np.array([2, 1], np.uint32))


# ---- the file ----
LAYOUT = np.array([[0, 0, 0, 100], [0, 10, 0, 148], [1, 4, 0, 64], [1, 4, 64, 64], [3, 9, 0, 7], [3, 9, 7, 3], [3, 11, 0, 40], [4, 1, 0, 1 << 20], [4, 9, 0, 999]], np.uint64)


def _records(n=8, seed=5):
    pos = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(4096)
    pos[-1] -= np.uint64(1000)   # a ragged last chunk
    words = np.random.default_rng(seed).integers(0, 1 << 63, (n, len(LAYOUT)), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    words[0, 0] = 0
    words[1, 1] = np.uint64(M64)
    return pos, words


def test_write_read_round_trip_and_equal_files(tmp_path):
    pos, words = _records()
    path = str(tmp_path / "a.state")
    J.write_state(path, LAYOUT, pos, words)
    lay, p2, w2 = J.read_state(path)
    assert np.array_equal(lay, LAYOUT) and np.array_equal(p2, pos) and np.array_equal(w2, words)
    lines = open(path).read().split("\n")
    assert lines[0] == J.STATE_MAGIC and lines[1] == "# columns %d" % len(LAYOUT) and lines[2] == "# col 0 0 0 0 100"
    assert len(lines[2 + len(LAYOUT)].split()) == 1 + len(LAYOUT)
    assert J.first_state_difference((lay, p2, w2), (LAYOUT, pos, words)) is None
    assert J.describe_state(None) == "no difference"
    empty = str(tmp_path / "e.state")   # a run killed before its first record leaves the header
    J.write_state(empty, LAYOUT, pos[:0], words[:0])
    lay, p0, w0 = J.read_state(empty)
    assert len(p0) == 0 and w0.shape == (0, len(LAYOUT)) and np.array_equal(lay, LAYOUT)


def test_a_difference_in_one_column_of_record_3():
    pos, words = _records()
    w2 = words.copy()
    w2[3, 5] ^= np.uint64(1 << 40)
    d = J.first_state_difference((LAYOUT, pos, words), (LAYOUT, pos, w2))
    assert (d["record"], d["kind"], d["byte0"], d["byte1"], d["columns"]) == (3, "state", 3 * 4096, 4 * 4096, [5])
    assert d["names"] == ["fxcm region 9 (wx) array 1 (words 7..9 of the region)"]
    assert (d["a"], d["b"]) == (int(words[3, 5]), int(w2[3, 5]))
    assert d["stages"] == [("fxcm", 3, 4 * 4096)]
    text = J.describe_state(d)
    assert "record 3" in text and "bytes 12288..16383" in text and "fxcm region 9 (wx) array 1" in text
    w2[0, 8] += np.uint64(2)   # the first record already: no equal record before it
    d = J.first_state_difference((LAYOUT, pos, words), (LAYOUT, pos, w2))
    assert (d["record"], d["byte0"], d["byte1"], d["columns"]) == (0, 0, 4096, [8])
    assert d["names"] == ["paq8 region 9 (role structs' scalars) array 0 (words 0..998 of the region)"]


def test_per_stage_firsts_follow_the_spread():
    pos, words = _records()
    w2 = words.copy()
    w2[2:, 4] ^= np.uint64(1)          # fxcm from record 2 on
    w2[2, 6] ^= np.uint64(7)           # (another fxcm column of record 2)
    w2[5:, 0] += np.uint64(1)          # mixnet from record 5 on
    w2[6, 7] ^= np.uint64(1 << 63)     # paq8 in record 6 only
    d = J.first_state_difference((LAYOUT, pos, words), (LAYOUT, pos, w2))
    assert (d["record"], d["columns"]) == (2, [4, 6])
    assert d["stages"] == [("fxcm", 2, int(pos[2])), ("mixnet", 5, int(pos[5])), ("paq8", 6, int(pos[6]))]
    text = J.describe_state(d)
    assert text.index("fxcm     record 2") < text.index("mixnet   record 5") < text.index("paq8     record 6")
    # the other way round it is the same finding
    d2 = J.first_state_difference((LAYOUT, pos, w2), (LAYOUT, pos, words))
    assert d2["stages"] == d["stages"] and (d2["a"], d2["b"]) == (d["b"], d["a"])


def test_length_and_position_differences():
    pos, words = _records()
    d = J.first_state_difference((LAYOUT, pos, words), (LAYOUT, pos[:5], words[:5]))
    assert (d["kind"], d["record"], d["a"], d["b"]) == ("length", 5, 8, 5)
    p2 = pos.copy()
    p2[4] += np.uint64(1)
    d = J.first_state_difference((LAYOUT, pos, words), (LAYOUT, p2, words))
    assert (d["kind"], d["record"]) == ("position", 4)


def test_a_truncated_last_line_is_ignored(tmp_path):
    pos, words = _records()
    path = str(tmp_path / "a.state")
    J.write_state(path, LAYOUT, pos, words)
    text = open(path).read()
    for cut in (5, 17 * 3, len(text.split("\n")[-2])):   # inside the last record: in its position, in a word, and all of it but the newline
        with open(path, "w") as f:
            f.write(text[:len(text) - 1 - len(text.split("\n")[-2]) + cut])
        lay, p2, w2 = J.read_state(path)
        assert np.array_equal(p2, pos[:-1]) and np.array_equal(w2, words[:-1])
    with open(path, "w") as f:   # a damaged line that is NOT the last is an error, not silence
        lines = text.split("\n")
        lines[len(LAYOUT) + 4] = lines[len(LAYOUT) + 4][:40]
        f.write("\n".join(lines))
    with pytest.raises(ValueError):
        J.read_state(path)
    with open(path, "w") as f:
        f.write("12 34\n")
    with pytest.raises(ValueError):
        J.read_state(path)


def test_layout_mismatch_is_refused(tmp_path):
    pos, words = _records()
    other = LAYOUT.copy()
    other[4, 3] += np.uint64(1)
    with pytest.raises(ValueError):
        J.first_state_difference((LAYOUT, pos, words), (other, pos, words))
    with pytest.raises(ValueError):
        J.first_state_difference((LAYOUT, pos, words), (LAYOUT[:-1], pos, words[:, :-1]))
    a, b = str(tmp_path / "a.state"), str(tmp_path / "b.state")
    J.write_state(a, LAYOUT, pos, words)
    J.write_state(b, other, pos, words)
    r = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "state-diff", a, b], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "different layouts" in r.stderr and "no difference" not in r.stdout


def test_state_diff_command_line_runs_without_torch(tmp_path):
    pos, words = _records()
    w2 = words.copy()
    w2[3:, 2] ^= np.uint64(1)
    w2[6, 8] ^= np.uint64(1)
    a, b = str(tmp_path / "a.state"), str(tmp_path / "b.state")
    J.write_state(a, LAYOUT, pos, words)
    J.write_state(b, LAYOUT, pos, w2)
    prog = ("import sys\nfrom cmix_amd import journal\nrc = journal.main(sys.argv[1:])\n"
            "assert 'torch' not in sys.modules, 'state-diff imported torch'\nsys.exit(rc)\n")
    same = subprocess.run([sys.executable, "-c", prog, "state-diff", a, a], cwd=ROOT, capture_output=True, text=True)
    assert same.returncode == 0 and "compared 8 record(s) of 9 column(s): no difference" in same.stdout, same.stdout + same.stderr
    diff = subprocess.run([sys.executable, "-c", prog, "state-diff", a, b], cwd=ROOT, capture_output=True, text=True)
    assert diff.returncode == 1, diff.stdout + diff.stderr
    assert "first difference in record 3" in diff.stdout and "bytes 12288..16383" in diff.stdout
    assert "context region 4 (pred) array 0 (words 0..63 of the region)" in diff.stdout
    assert diff.stdout.index("context  record 3") < diff.stdout.index("paq8     record 6")
    mod = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "state-diff", a, b], cwd=ROOT, capture_output=True, text=True)
    assert mod.returncode == 1 and mod.stdout == diff.stdout
    old = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "bogus"], cwd=ROOT, capture_output=True, text=True)
    assert old.returncode == 2 and "diff a b" in old.stderr
