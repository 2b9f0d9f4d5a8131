"""The fxcm stage without a GPU: the product's host text parser (cmix_amd/csrc/fxcm_parser_host.cpp) and the BODY of
cmx_fxcm_chunk_kernel (cmix_amd/csrc/fxcm_dev.h: five barrier-separated phases per bit) run through
tests/host/fxcm_emul.cpp -- a loop over thread ids per phase, in shuffled order -- against the oracle's monolithic
restatement of the model (oracle/fxcm_model.c, itself pinned against the reference's fxcmv1::Predictor) and against
layer-0 columns 3..433 of the golden traces recorded from the unmodified reference predictor. All 431 values per bit,
bit for bit. The same comparison runs on the device in tests/test_zgpu_stage_fxcm.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "host", "libfxcmemul.so")
SRC = [os.path.join(ROOT, "tests", "host", "fxcm_emul.cpp"), os.path.join(ROOT, "cmix_amd", "csrc", "fxcm_parser_host.cpp")]
DEPS = SRC + [os.path.join(ROOT, "cmix_amd", "csrc", f) for f in ("fxcm_dev.h", "fxcm_build.h", "fxcm_rec.h")]


def emul():
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", SO] + SRC)
    L = C.CDLL(SO)
    L.fxe_create.restype = C.c_void_p
    L.fxe_create.argtypes = [C.c_char_p, C.c_uint32]
    L.fxe_destroy.argtypes = [C.c_void_p]
    L.fxe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    return L


def oracle_rows(data, lstmpr, lstmex, dictionary=None, blpos=0):
    """rows[q] = FXCM::Predict() before bit q is coded (row 0 = the constructor's 0.5). blpos: start the model at that
    position in the block (orc_fx_model_set_blpos) to reach the thresholds that depend on it."""
    lib = O.lib()
    lib.orc_fx_model_new.restype = C.c_void_p
    lib.orc_fx_model_new_dict.restype = C.c_void_p
    lib.orc_fx_model_new_dict.argtypes = [C.c_char_p]
    lib.orc_fx_model_update.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    h, tag = O.new_owned(lib.orc_fx_model_new_dict, dictionary) if dictionary else O.new_owned(lib.orc_fx_model_new)
    if blpos:
        lib.orc_fx_model_set_blpos.argtypes = [C.c_void_p, C.c_int]
        lib.orc_fx_model_set_blpos(h, blpos)
    rows = np.full((8 * len(data), 431), 0.5, np.float32)
    out = np.zeros(431, np.float32)
    q = 0
    for b in data:
        for j in range(7, -1, -1):
            assert lib.orc_fx_model_update(h, (int(b) >> j) & 1, int(lstmpr[q]), int(lstmex[q]), out.ctypes.data) >= 0
            if q + 1 < len(rows):
                rows[q + 1] = out
            q += 1
    O.release(tag)   # (the model's tables: 4.4 GB of address space, freed here rather than at pytest's exit)
    return rows


def run_emul(L, data, lstmpr, lstmex, chunks, seed=12345, dictionary=None, blpos=0, serial_maps=False, stats=None, poison=None):
    h = L.fxe_create(dictionary, seed)
    if poison is not None:   # FxShared is refilled with this byte at the start of every fxe_run (tests/host/fxcm_emul.cpp, the audit at its top)
        L.fxe_set_poison.argtypes = [C.c_void_p, C.c_int]
        L.fxe_set_poison(h, poison)
    if serial_maps:
        L.fxe_set_serial_maps.argtypes = [C.c_void_p, C.c_int]
        L.fxe_set_serial_maps(h, 1)
    if blpos:
        L.fxe_set_blpos.argtypes = [C.c_void_p, C.c_int]
        L.fxe_set_blpos(h, blpos)
    data = np.ascontiguousarray(data, np.uint8)
    out = np.zeros((8 * len(data), 431), np.float32)
    pos = 0
    for n in chunks:
        n = min(n, len(data) - pos)
        if n <= 0:
            break
        pr = np.ascontiguousarray(lstmpr[8 * pos:8 * (pos + n)], np.int16)
        ex = np.ascontiguousarray(lstmex[8 * pos:8 * (pos + n)], np.uint8)
        o = out[8 * pos:8 * (pos + n)]
        assert L.fxe_run(h, data[pos:pos + n].ctypes.data, n, pr.ctypes.data, ex.ctypes.data, o.ctypes.data, 431) == 0
        pos += n
    if stats is not None:
        st = np.zeros(2, np.uint64)
        L.fxe_conflict_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.fxe_conflict_stats(h, st.ctypes.data)
        stats.extend(int(v) for v in st)
    L.fxe_destroy(h)
    return out[:8 * pos]


def hints(nbits, seed):
    r = np.random.default_rng(seed)
    return r.integers(1, 4096, nbits).astype(np.int16), r.integers(0, 256, nbits).astype(np.uint8)


def compare(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want[:len(got)].view(np.uint32))
    assert bad.size == 0, (what, "first mismatch (bit, column):", bad[0], got[tuple(bad[0])] * 4095, want[tuple(bad[0])] * 4095, "columns:", sorted(set(bad[:, 1]))[:12])


def test_text_vs_oracle_ragged_chunks():
    from cmix_amd import synth
    L = emul()
    data = np.frombuffer(synth.enwik_like(6000, 31), np.uint8)
    pr, ex = hints(8 * len(data), 7)
    want = oracle_rows(data, pr, ex)
    stats = []
    got = run_emul(L, data, pr, ex, [1, 1, 7, 100, 1000, 3, 2000, 4000], stats=stats)
    compare(got, want, "enwik-like text")
    # the slot-parallel path is the one exercised, and its serial fallback (two contexts of a map in one bucket) occurs
    assert 0 < stats[1] < stats[0] // 4, stats
    compare(run_emul(L, data[:2500], pr, ex, [2500], serial_maps=True), want, "one lane per map")


POISON = [0xFF, 0xA5, 0x00]   # what the LDS model holds when a run ("launch") begins: all bits set, a non-trivial byte, a fresh device's zeros
_poison_ref = {}


def _poison_case():
    """enwik-like text, LSTM hints and the oracle's rows: computed once for all poison bytes"""
    if not _poison_ref:
        from cmix_amd import synth
        data = np.frombuffer(synth.enwik_like(2500, 31), np.uint8)
        pr, ex = hints(8 * len(data), 7)
        _poison_ref["case"] = (data, pr, ex, oracle_rows(data, pr, ex))
    return _poison_ref["case"]


@pytest.mark.parametrize("poison", POISON)
def test_poisoned_lds_ragged_chunks_vs_oracle(poison):
    """Nothing the body reads from FxShared may be what the previous launch left there: with the whole struct refilled with a byte at the
    start of every run (on the device another kernel may have had the compute unit in between), ragged chunks still give the oracle's rows."""
    data, pr, ex, want = _poison_case()
    stats = []
    got = run_emul(emul(), data, pr, ex, [1, 1, 7, 100, 1000, 3, 2000], stats=stats, poison=poison)
    compare(got, want, "poison 0x%02X" % poison)
    assert 0 < stats[1] < stats[0], stats   # both the slot-parallel path and its serial fallback ran


@pytest.mark.parametrize("poison", POISON)
def test_poisoned_lds_one_lane_per_map_vs_oracle(poison):
    data, pr, ex, want = _poison_case()
    compare(run_emul(emul(), data[:1200], pr, ex, [1, 7, 500, 1000], serial_maps=True, poison=poison), want, "one lane per map, poison 0x%02X" % poison)


def other_data_case(flavour):
    """data and hints of test_other_data_vs_oracle (the device runs the markup flavour as well, tests/test_zgpu_stage_fxcm.py)"""
    r = np.random.default_rng(5)
    if flavour == "binary":
        data = r.integers(0, 256, 3000).astype(np.uint8)
    elif flavour == "runs":
        data = np.concatenate([np.full(int(n), int(v), np.uint8) for n, v in zip(r.integers(1, 40, 150), r.integers(0, 256, 150))])[:3000]
    else:   # cmix's WRT-swapped wiki markup: tables, links, headers, entities, escaped UTF-8, numbers
        parts = [b"PPQ class=wikitable\nQ-\nQ cell one QQ cell two\nQ-\nQ 12.5 QQ 1,000\nQR\n", b"NN Heading NN\n@the quick [[brown fox]] jumps over the (lazy) dog. ",
                 b"''italic'' and &Lref&N http://example.org/x J y\n", b"* item one\n* item two\n\n", b"\x0c\xc3\xa9t\x0c\xc3\xa9 1999 2001, 3.14 ", b"@she said 'hello' to him; it was theirs.\n"]
        data = np.frombuffer(b"".join(parts[int(i)] for i in r.integers(0, len(parts), 80)), np.uint8)[:3500]
    pr, ex = hints(8 * len(data), 11)
    return data, pr, ex


@pytest.mark.parametrize("flavour", ["binary", "runs", "markup"])
def test_other_data_vs_oracle(flavour):
    L = emul()
    data, pr, ex = other_data_case(flavour)
    want = oracle_rows(data, pr, ex)
    got = run_emul(L, data, pr, ex, [512] * 8, seed=99)
    compare(got, want, flavour)


def dictionary_case():
    """data, hints and the path of a stand-in dictionary (one word per line; the caller unlinks it) for the dictionary-mode tests, host and device"""
    import tempfile
    words = ["the", "of", "and", "text", "math", "page", "category", "image", "running", "houses", "quickly", "nowiki", "pre", "wikipedia"] + ["w%dx" % i for i in range(200)]
    with tempfile.NamedTemporaryFile("w", suffix=".dic", delete=False) as f:
        f.write("\n".join(words) + "\n")
        path = f.name.encode()
    r = np.random.default_rng(3)
    toks = []
    for _ in range(700):
        k = int(r.integers(0, 3))
        if k == 0:
            toks.append(bytes([128 + int(r.integers(0, 80))]))
        elif k == 1:
            toks.append(bytes([128 + 80 + int(r.integers(0, 2)), 128 + int(r.integers(0, 80))]))
        else:
            toks.append([b"the", b"Ltext N", b"J", b".", b",", b"dog", b"@"][int(r.integers(0, 7))])
        toks.append(b" " if r.random() < 0.8 else b"\n")
    data = np.frombuffer(b"".join(toks), np.uint8)[:2500]
    pr, ex = hints(8 * len(data), 13)
    return data, pr, ex, path


def test_dictionary_mode_vs_oracle():
    """WRT codewords (bytes >= 128) decoded through cmix's dictionary feed the stemmer; the dictionary travels with the
    fixtures as a small stand-in (one word per line)."""
    L = emul()
    data, pr, ex, path = dictionary_case()
    try:
        want = oracle_rows(data, pr, ex, dictionary=path)
        got = run_emul(L, data, pr, ex, [300] * 10, dictionary=path)
    finally:
        os.unlink(path.decode())
    compare(got, want, "dictionary mode")


@pytest.mark.parametrize("name", ["text_96"])
def test_golden_columns(name):
    """Columns 3..433 of a trace of the unmodified reference predictor, with the hints the reference's LSTM produced
    (recomputed by the LSTM restatement): fixtures only."""
    import make_golden as mg
    g = load_golden(name)
    probs, bits, stream = mg.unpack_probs(g), g["bits"], g["stream"]
    l = O.Lstm(g["vocab"])
    pr, ex = np.zeros(len(bits), np.int16), np.zeros(len(bits), np.uint8)
    t = 0
    for n in range(len(stream)):
        for j in range(7, -1, -1):
            l.bit_perceive((int(stream[n]) >> j) & 1)
            if j == 0:
                l.byte_update(g["ppmd_probs"][n + 1], stream[n])
            if t + 1 < len(bits):
                pr[t] = int(np.float32(1) + np.float32(4094) * np.float32(l.bit_predict()))
                ex[t] = int(l.ex())
            else:
                pr[t] = 2048
            t += 1
    got = run_emul(emul(), np.asarray(stream, np.uint8), pr, ex, [len(stream)])
    compare(got, np.ascontiguousarray(probs[:, 3:434]), name)


def pretraining_case():
    """a word list driven with the hints at 0 (as Predictor::Pretrain does), then text with seeded hints: data, hints, and the cuts (the first is the word list)"""
    from cmix_amd import synth
    data = np.frombuffer(b"aardvark\nabacus\nabandon\nability\nzebra\n" * 20 + synth.enwik_like(1500, 8), np.uint8)
    npre = 8 * 41 * 20
    pr, ex = hints(8 * len(data), 21)
    pr[:npre] = 0
    ex[:npre] = 0
    return data, pr, ex, [41 * 20, 700, 800]


def test_pretraining_then_data_vs_oracle():
    """Predictor::Pretrain drives fxcm over the dictionary with the hints at their start-up value 0 (predictor.cpp:359,
    471-476); the coded data follows in the same model."""
    L = emul()
    data, pr, ex, chunks = pretraining_case()
    compare(run_emul(L, data, pr, ex, chunks), oracle_rows(data, pr, ex), "pretraining + data")


@pytest.mark.parametrize("blpos", [14 * 256 * 1024 - 900, 28 * 512 * 1024 - 900, 448131719 - 700, 463139793 - 700])
def test_block_position_thresholds_vs_oracle(blpos):
    """The SSCM / APM rates change 3.67 MB and 14.7 MB into the block, two parser rules 448 MB and 463 MB in (update1
    :4772-4774, modelPrediction :3866, :3932): the stream starts just before each threshold. (This stream does not react to every
    threshold; test_block_position_thresholds_vs_oracle_cut_layouts runs all five on one that does.)"""
    from cmix_amd import synth
    L = emul()
    data = np.frombuffer(synth.enwik_like(1800, 4), np.uint8)
    pr, ex = hints(8 * len(data), 17)
    compare(run_emul(L, data, pr, ex, [600] * 3, blpos=blpos), oracle_rows(data, pr, ex, blpos=blpos), "blpos %d" % blpos)


# ---- every threshold on a stream that reacts to it, cut three ways -------------------------------------------------------------------------
# The five places fxcm reads its position in the block: the SSCM / APM rates (update1 :4772-4774) and three parser rules -- the codeword
# context (:3866 / :3932), the stemmer's auxiliary-verb list (:3198, fxcm_parser_host.cpp fx_stem) and the conjunction rule (:3965).
THRESHOLDS = [14 * 256 * 1024, 28 * 512 * 1024, 448131719, 451531986, 463139793]
THRESHOLD_BACK = 700    # the stream starts this many bytes below the threshold: the first update with blpos > T is the boundary bit of stream byte 700
# the crossing in mid-launch | stream byte 700 is a launch's last byte | byte 700 and byte 701 are each a launch of their own
THRESHOLD_CUTS = {"mid": [600, 600, 600], "last": [701, 1099], "alone": [700, 1, 1, 1098]}
_THRESHOLD_TEXT = (b"the cat sat and the dog ran but it was late; however he has been there, and she is going. they were happy or sad, yet we have seen it. "
                   b"it will be done because you can do it although I am not sure.\n")
_threshold_ref = {}


def threshold_stream(n=1800):
    """Text in which every rule that depends on the position has something to decide after the crossing: auxiliary verbs, conjunctions and
    conjunctive adverbs at word ends, words for the codeword context; with it the hints."""
    from cmix_amd import synth
    data = np.frombuffer((synth.enwik_like(600, 4) + _THRESHOLD_TEXT * 12)[:1800], np.uint8)[:n]
    pr, ex = hints(8 * 1800, 17)
    return data, pr[:8 * n], ex[:8 * n]


def threshold_case(threshold, back=THRESHOLD_BACK):
    """the stream, its hints and the oracle's rows for a start `back` bytes below the threshold: computed once for the cut layouts of a test, which
    run one after the other (only the last threshold's rows are kept, 25 MB: a set per threshold would stay for the rest of the process)"""
    key = (threshold, back)
    if key not in _threshold_ref:
        data, pr, ex = threshold_stream()
        _threshold_ref.clear()
        _threshold_ref[key] = (data, pr, ex, oracle_rows(data, pr, ex, blpos=threshold - back))
    return _threshold_ref[key]


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_the_thresholds_matter(threshold):
    """The threshold cases would be worthless on a stream that does not react: the oracle's rows for a start 700 bytes below the threshold must
    differ from those for a start 65 536 bytes lower (which crosses nothing) -- and not before bit 8 * 700, so the difference is the
    crossing's and not the start position's."""
    data, pr, ex, rows = threshold_case(threshold)
    low = oracle_rows(data, pr, ex, blpos=threshold - THRESHOLD_BACK - 65536)
    differs = np.nonzero((rows.view(np.uint32) != low.view(np.uint32)).any(axis=1))[0]
    print("threshold %d: first differing bit %s, %d differing rows" % (threshold, differs[:1], differs.size))
    assert differs.size > 0, "the stream does not react to the threshold at %d" % threshold
    assert differs[0] >= 8 * THRESHOLD_BACK, (threshold, "rows differ before the crossing, first at bit", int(differs[0]))


@pytest.mark.parametrize("cuts", sorted(THRESHOLD_CUTS))
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_block_position_thresholds_vs_oracle_cut_layouts(threshold, cuts):
    """All five thresholds on the stream of test_the_thresholds_matter, the crossing in mid-launch, as a launch's last byte and as a launch of its own."""
    data, pr, ex, want = threshold_case(threshold)
    compare(run_emul(emul(), data, pr, ex, THRESHOLD_CUTS[cuts], blpos=threshold - THRESHOLD_BACK), want, "threshold %d, cuts %s" % (threshold, cuts))


def _reference_fixture(name):
    """tests/golden/fxcm_cols_*.npz (tests/golden/make_fxcm_hashes.py): per-bit hashes of the 431 values the UNMODIFIED
    reference's fxcmv1::Predictor returned for a 16 KB stream, with the seeded hints it was driven with."""
    import make_fxcm_hashes as mk
    g = load_golden(name)
    data = g["stream"]
    pr, ex = mk.hints(8 * len(data), int(g["hint_seed"][0]))
    dic = None
    if "dictionary" in g:
        import tempfile
        with tempfile.NamedTemporaryFile("wb", suffix=".dic", delete=False) as f:
            f.write(g["dictionary"].tobytes())
            dic = f.name.encode()
    return data, pr, ex, dic, g["hash"], mk.row_hash


@pytest.mark.parametrize("name", ["fxcm_cols_wiki_16k", "fxcm_cols_dict_16k", "fxcm_cols_mixed_24k", "fxcm_cols_rich_16k"])
def test_reference_hashes_16k(name):
    """The product's text parser + the kernel body (host run) and the oracle against the reference itself on 16 KB of
    wiki markup and of dictionary-mode (WRT-coded) text: 131072 bits x 431 values each, compared through row hashes."""
    L = emul()
    data, pr, ex, dic, want, row_hash = _reference_fixture(name)
    try:
        got = row_hash(run_emul(L, data, pr, ex, [4096, 1, 4095, 8192, 8192], dictionary=dic))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, "kernel body: first differing bit", int(bad[0]))
        orc = row_hash(oracle_rows(data, pr, ex, dictionary=dic))
        bad = np.nonzero(orc != want)[0]
        assert bad.size == 0, (name, "oracle: first differing bit", int(bad[0]))
    finally:
        if dic:
            os.unlink(dic.decode())


def test_role_m_wavefront_layout():
    """Role M of the device stage runs as free-running wavefronts that own whole maps (fxcm_build.h): the groups must cover every
    slot and map exactly once, in order, cut at map boundaries, fit the 16 wavefronts and leave every wavefront a handful of lanes."""
    L = emul()
    h = L.fxe_create(None, 0)
    out = (C.c_int * (2 * 17 + 31))()
    L.fxe_wave_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.fxe_wave_layout(h, out)
    L.fxe_destroy(h)
    slots, maps, cs = list(out[0:17]), list(out[17:34]), list(out[34:65])
    assert sum(cs) == 81 and len(cs) == 31
    assert slots[0] == 0 and maps[0] == 0 and slots[16] == 81 and maps[16] == 31
    first_slot = [sum(cs[:k]) for k in range(32)]
    for w in range(16):
        assert maps[w] <= maps[w + 1] and slots[w] <= slots[w + 1]
        assert slots[w] == first_slot[maps[w]], "a wavefront starts at a map boundary"
        assert slots[w + 1] - slots[w] <= 12, "few lanes per wavefront"
    assert sum(1 for w in range(16) if slots[w + 1] > slots[w]) >= 12, "the maps are spread over the wavefronts"
