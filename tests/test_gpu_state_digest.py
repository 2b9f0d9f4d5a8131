"""GPU: the state digest (include/cmix_amd.h, "State digest"; cmix_amd/csrc/state_digest.hip) and the state journal on top of it.

The kernel against the numpy model (cmix_amd/journal.py state_digest, itself held to the formula by tests/test_state_digest_rule.py) on arrays of
0 .. 2^20 + 3 words and on a list that puts a one-word array between two large ones; per stage two fresh handles fed the same input agree in every
column and differ from a fresh handle in the learning tables' columns (fxcm and paq8: the second handle in two ragged launches); a flipped word of an
open region moves exactly its column by splitmix64(i, w') - splitmix64(i, w), the stage's state_diff names the same region, and flipping back restores
the digest; paq8 under poisoned LDS and with a picture in its stream; and the pipeline's journal: two streams write identical files, a record is the
digest taken by hand at its position, and one flipped wx word of fxcm is what state-diff names. Handles are shared by the module and closed at its end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, synth_mixnet_inputs
from cmix_amd import journal as J

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
N_TEXT = 2048
VOCAB = np.ones(256, np.uint8)


def _text(n=N_TEXT, seed=5):
    from cmix_amd import synth
    return np.frombuffer(synth.enwik_like(n, seed), np.uint8).copy()


# ---- the kernel ----
@pytest.fixture(scope="module")
def device_words():
    """(host, device) arrays of every size the kernel tests use, made once and never written"""
    import torch
    rng = np.random.default_rng(21)
    out = {}
    for n in (0, 1, 3, 4, 5, 255, 257, (1 << 20) + 3, (1 << 20) + 5):
        h = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if n >= 5:
            h[1], h[n - 1] = 0, 0xFFFFFFFF
        out[n] = (h, torch.from_numpy(h.view(np.int32)).cuda())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 257, (1 << 20) + 3])
def test_kernel_equals_the_model(device_words, n):
    from cmix_amd import engine as E
    h, d = device_words[n]
    got = E.state_digest_arrays([d])
    assert [int(x) for x in got] == [J.state_digest(h)]
    assert E.state_digest_host(h) == int(got[0])


def test_kernel_one_launch_over_a_mixed_list(device_words):
    """workgroups are dealt by size: a one-word array between two large ones, empty and tiny arrays, a single-word tail (n % 4 = 1, 3)"""
    from cmix_amd import engine as E
    order = [(1 << 20) + 3, 1, (1 << 20) + 5, 0, 255, 3, 257, 4, 5]
    got = E.state_digest_arrays([device_words[n][1] for n in order])
    assert [int(x) for x in got] == [J.state_digest(device_words[n][0]) for n in order]
    assert [int(x) for x in E.state_digest_arrays([device_words[n][1] for n in reversed(order)])] == [int(x) for x in got[::-1]]
    assert len(E.state_digest_arrays([])) == 0


# ---- the stages ----
def _mixnet_inputs():
    import torch
    probs, sel, bits = synth_mixnet_inputs(N_TEXT, seed=9, n_ctx_bits=2)
    return (torch.from_numpy(np.ascontiguousarray(probs)).cuda(), torch.from_numpy((sel & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(bits)).cuda())


class _Stage:
    """one stage: make() a fresh handle, run(handle, cuts) the module's input through it in launches of cuts bytes (mixnet: bits)"""

    def __init__(self, name):
        import torch
        self.name, self.torch = name, torch
        self.text = _text()
        if name == "mixnet":
            self.inp = _mixnet_inputs()
        elif name == "lstm":
            rng = np.random.default_rng(4)
            p = rng.dirichlet(np.full(256, 0.3), N_TEXT).astype(np.float32)
            self.inp = (torch.from_numpy(p).cuda(), torch.from_numpy(self.text).cuda())
        elif name == "ctxmodels":
            self.inp = torch.from_numpy(self.text).cuda()
        elif name == "fxcm":
            r = np.random.default_rng(7)
            self.inp = (r.integers(1, 4096, 8 * N_TEXT).astype(np.int16), r.integers(0, 256, 8 * N_TEXT).astype(np.uint8))
        self.keep = []

    def make(self):
        from cmix_amd import engine as E
        return {"mixnet": lambda: E.MixNet(0), "ctxmodels": lambda: E.CtxModels(VOCAB, 0), "lstm": lambda: E.Lstm(VOCAB, 0), "fxcm": lambda: E.Fxcm(None, 0),
                "p8stage": lambda: E.P8Stage(0)}[self.name]()

    def run(self, h, cuts, data=None):
        torch = self.torch
        pos = 0
        for n in cuts:
            a, b = pos, pos + n
            if self.name == "mixnet":
                probs, sel, bits = self.inp
                self.keep.append(h.run(probs[a:b], sel[a:b], bits[a:b]))
            elif self.name == "ctxmodels":
                self.keep.append(h.run(self.inp[a:b]))
            elif self.name == "lstm":
                self.keep.append(h.run(self.inp[0][a:b], self.inp[1][a:b]))
            elif self.name == "fxcm":
                pr, ex = self.inp
                self.keep.append(h.run(self.text[a:b], torch.from_numpy(pr[8 * a:8 * b].copy()).cuda(), torch.from_numpy(ex[8 * a:8 * b].copy()).cuda(),
                                       torch.full((8 * n, 434), -1.0, dtype=torch.float32, device="cuda")))
            else:
                self.keep.append(h.run(bytes((self.text if data is None else data)[a:b])))
            pos = b
        torch.cuda.synchronize()
        if hasattr(h, "sync"):
            h.sync()
        self.keep = []


STAGES = ["mixnet", "ctxmodels", "lstm", "fxcm", "p8stage"]
RAGGED = {"fxcm": [768, 1280], "p8stage": [768, 1280]}
# regions whose arrays learn from any input: at least one column of each must have left its initial digest
LEARNING = {"mixnet": [0, 1, 2, 10], "ctxmodels": [0, 1, 4], "lstm": [0, 2, 3, 8, 11], "fxcm": [1, 2, 9, 10, 11], "p8stage": [0, 1, 2, 4, 5, 9]}
_cache = {}


def _pair(name):
    """(stage, handle a, handle b, fresh digest, a's digest, b's digest, layout): a ran the input in one launch, b in one or (fxcm, paq8) two ragged ones"""
    if name not in _cache:
        st = _Stage(name)
        a, b = st.make(), st.make()
        fresh, fresh_b = a.state_digest(), b.state_digest()
        assert np.array_equal(fresh, fresh_b), "two fresh handles differ in columns %r" % np.flatnonzero(fresh != fresh_b).tolist()
        st.run(a, [N_TEXT])
        st.run(b, RAGGED.get(name, [N_TEXT]))
        _cache[name] = (st, a, b, fresh, a.state_digest(), b.state_digest(), a.state_digest_layout())
    return _cache[name]


def _release():
    """close the stages' handles: a process may hold 32 hardware queues, an engine takes 13 of them"""
    for st, a, b, *_ in _cache.values():
        a.close()
        b.close()
    _cache.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    _release()


@pytest.mark.parametrize("name", STAGES)
def test_two_handles_fed_the_same_input_agree_in_every_column(name):
    st, a, b, fresh, da, db, lay = _pair(name)
    assert len(da) == len(db) == len(fresh) == len(lay) > 0
    bad = np.flatnonzero(da != db)
    assert bad.size == 0, "%s: columns %r differ between two handles fed equal input (regions %r)" % (name, bad.tolist()[:12], sorted(set(int(lay[c, 0]) for c in bad)))
    assert np.array_equal(a.state_digest(), da)   # the digest reads the state and leaves it alone


@pytest.mark.parametrize("name", STAGES)
def test_learning_tables_leave_their_initial_digest(name):
    st, a, b, fresh, da, db, lay = _pair(name)
    moved = set(int(lay[c, 0]) for c in np.flatnonzero(da != fresh))
    assert set(LEARNING[name]) <= moved, "%s: regions %r learn from any input, but only %r moved" % (name, LEARNING[name], sorted(moved))
    if name == "fxcm":
        assert 0 not in moved   # constant tables
    # the layout: regions stand together and offsets run through a region (paq8 has models without a table of a kind: an empty array digests to 0)
    off = {}
    for c, (rg, o, n) in enumerate(lay.tolist()):
        assert o == off.get(rg, 0) and (n > 0 or (name == "p8stage" and int(da[c]) == 0))
        off[rg] = o + n
    assert [int(x) for x in lay[:, 0]] == sorted(int(x) for x in lay[:, 0])


def _flip_case(name):
    """(hook arguments, region, word index inside the region) of one word of a region the stage's hook leaves open: a value, never an address"""
    from cmix_amd import engine as E
    if name == "mixnet":
        return (0, 0, 0, 5), 0, 5                    # layer-0 weight 5 of mixer 0's row 0
    if name == "ctxmodels":
        at = int(E.ctx_layout()["br_probs"]) + 3
        return (0, None, at), 0, at                  # br_probs[3] of CtxPersist
    if name == "lstm":
        return (0, 7), 0, 7                          # W[0][0], word 7
    return (9, 3), 9, 3                              # fxcm: wx, word 3


@pytest.mark.parametrize("name", ["mixnet", "ctxmodels", "lstm", "fxcm"])
def test_one_flipped_word_moves_its_column_by_the_predicted_amount(name):
    st, a, b, fresh, da, db, lay = _pair(name)
    args, region, index = _flip_case(name)
    cols = [c for c in range(len(lay)) if int(lay[c, 0]) == region and int(lay[c, 1]) <= index < int(lay[c, 1]) + int(lay[c, 2])]
    assert len(cols) == 1
    col, i = cols[0], index - int(lay[cols[0], 1])
    for mask in (1 << 3, 0x80000001):
        a.debug_state_xor(*args, mask)
        try:
            got = a.state_digest()
            diff = a.state_diff(b)   # the stage's existing read path: the words of a (flipped) and of b (as a's was)
            first = diff["first"]
            new, old = int(first["a"]), int(first["b"])
            assert diff["words"] == 1 and int(first["region"]) == region and new == old ^ mask, (name, diff)
            assert np.flatnonzero(got != da).tolist() == [col], (name, np.flatnonzero(got != da).tolist(), col)
            assert (int(got[col]) - int(da[col])) & M64 == (J.state_term(i, new) - J.state_term(i, old)) & M64
        finally:
            a.debug_state_xor(*args, mask)
        assert np.array_equal(a.state_digest(), da), "%s: flipping back did not restore the digest" % name
        assert a.state_diff(b)["words"] == 0


# ---- paq8 ----
def _lds_fill(pattern):
    from cmix_amd import engine as E
    r = E.lds_fill(pattern)
    assert r["full"] and r["workgroups"] >= r["compute_units"] > 0, "LDS fill 0x%08X did not cover the device: %r" % (pattern, r)


def test_paq8_under_poisoned_lds_equals_the_clean_handle():
    st, a, b, fresh, da, db, lay = _pair("p8stage")
    _lds_fill(0xFFFFFFFF)   # (before the handle exists: creation launches init kernels)
    h = st.make()
    try:
        assert np.array_equal(h.state_digest(), fresh)
        pos = 0
        for n in (512, 1, 700, 835):
            _lds_fill(0xFFFFFFFF)
            st.keep.append(h.run(bytes(st.text[pos:pos + n])))
            pos += n
        assert pos == N_TEXT
        h.sync()
        got = h.state_digest()
    finally:
        st.keep = []
        h.close()
    bad = np.flatnonzero(got != da)
    assert bad.size == 0, "columns %r differ from the clean handle's (regions %r)" % (bad.tolist()[:12], sorted(set(int(lay[c, 0]) for c in bad)))


def test_paq8_picture_moves_the_image_models_columns():
    """text leaves the image models' tables (regions 6, 7) at their initial digest; the first 2 KB of the 24-bit BMP fixture (155 bytes of text, the
    header, then pixels) moves them"""
    st, a, b, fresh, da, db, lay = _pair("p8stage")
    image = [c for c in range(len(lay)) if int(lay[c, 0]) in (6, 7)]
    assert image and np.array_equal(da[image], fresh[image])
    with np.load(os.path.join(GOLDEN, "paq8_cols_bmp24_raw_9k.npz")) as z:
        stream = z["stream"][:N_TEXT].copy()
    assert bytes(stream).find(b"BM") == 155
    h = st.make()
    try:
        st.run(h, [N_TEXT], data=stream)
        got = h.state_digest()
    finally:
        h.close()
    assert np.flatnonzero(got[image] != fresh[image]).size > 0
    words = a.debug_state_words()
    assert len(words) == int(lay[-1, 2]) and J.state_digest(words) == int(da[-1])   # the last column is the digest of the role structs' scalar words


# ---- the pipeline and the engine ----
SUB, N_STREAM = 2048, 16384


@pytest.fixture(scope="module")
def stream_bytes():
    from cmix_amd import pipeline as P
    return P.text_file_stream(bytes(_text(N_STREAM - 6, 12)))


@pytest.fixture(scope="module")
def journalled(stream_bytes, tmp_path_factory):
    """one stream with state_journal=1: its file, its records, and the digest taken by hand after sub-chunk 3"""
    from cmix_amd import pipeline as P
    _release()
    s = P.EngineStream(0, stream_bytes, sub_chunk=SUB, state_journal=1)
    try:
        s.feed(3 * SUB)
        by_hand = s.pipe.state_digest()
        s.feed(N_STREAM)
        code = s.finish()
        lay, pos, words = s.state_journal()
    finally:
        s.close()
    path = str(tmp_path_factory.mktemp("sj") / "a.state")
    J.write_state(path, lay, pos, words)
    return dict(path=path, lay=lay, pos=pos, words=words, by_hand=by_hand, code=code)


def test_two_streams_write_identical_state_journals(journalled, stream_bytes, tmp_path):
    from cmix_amd import pipeline as P
    s = P.EngineStream(0, stream_bytes, sub_chunk=SUB, state_journal=1)
    try:
        s.feed(N_STREAM)
        code = s.finish()
        s.pipe.state_journal_write_file(str(tmp_path / "c.state"), final=True)   # the library's own writer
        lay, pos, words = s.state_journal()
    finally:
        s.close()
    assert code == journalled["code"]
    path = str(tmp_path / "b.state")
    J.write_state(path, lay, pos, words)
    assert open(path, "rb").read() == open(journalled["path"], "rb").read()
    assert open(str(tmp_path / "c.state"), "rb").read() == open(path, "rb").read()   # ... writes the same bytes as journal.write_state
    assert [int(x) for x in pos] == [SUB * (i + 1) for i in range(N_STREAM // SUB)]
    stages = sorted(set(int(x) for x in lay[:, 0]))
    assert stages == [0, 1, 2, 3, 4]
    assert all(np.any(words[k] != words[k - 1]) for k in range(1, len(pos)))
    r = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "state-diff", journalled["path"], path], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "compared 8 record(s)" in r.stdout and "no difference" in r.stdout, r.stdout + r.stderr


def test_a_record_is_the_digest_taken_by_hand(journalled):
    assert np.array_equal(journalled["words"][2], journalled["by_hand"])
    assert int(journalled["pos"][2]) == 3 * SUB


def test_a_period_takes_every_nth_record_and_the_last(journalled, stream_bytes):
    from cmix_amd import pipeline as P
    vocab = np.zeros(256, np.uint8)
    vocab[np.unique(np.frombuffer(stream_bytes, np.uint8))] = 1   # (the whole stream's, as the 16 KB runs have it: the LSTM's arrays are sized by it)
    s = P.EngineStream(0, stream_bytes[:5 * SUB + 100], sub_chunk=SUB, state_journal=4, vocab=vocab)
    try:
        s.feed(N_STREAM)
        s.finish()
        lay, pos, words = s.state_journal()
    finally:
        s.close()
    assert [int(x) for x in pos] == [4 * SUB, 5 * SUB + 100]
    assert np.array_equal(lay, journalled["lay"])
    assert np.array_equal(words[0], journalled["words"][3])   # the same bytes so far: the record every=4 takes after sub-chunk 4 is the one every=1 took there


def test_one_flipped_wx_word_is_what_state_diff_names(journalled, stream_bytes, tmp_path):
    """between sub-chunks 2 and 3 one wx word of the stream's own fxcm stage is flipped: record 1 (after sub-chunk 2) is still equal, record 2 names fxcm,
    region 9 (wx) and only that; later records show the same column again, or -- learning may have overwritten the word -- the difference has spread"""
    from cmix_amd import pipeline as P
    s = P.EngineStream(0, stream_bytes, sub_chunk=SUB, state_journal=1)
    try:
        s.feed(2 * SUB)
        s.pipe.sync()
        s.pipe.debug_fxcm_shadow_xor(0, 9, 3, 1 << 2)   # (instance 0: the stream's own stage)
        s.feed(N_STREAM)
        s.finish()
        lay, pos, words = s.state_journal()
    finally:
        s.close()
    path = str(tmp_path / "flipped.state")
    J.write_state(path, lay, pos, words)
    d = J.first_state_difference(J.read_state(journalled["path"]), J.read_state(path))
    assert d is not None and d["kind"] == "state" and d["record"] == 2 and (d["byte0"], d["byte1"]) == (2 * SUB, 3 * SUB)
    assert ("fxcm", 2, 3 * SUB) in d["stages"] and all(nm in ("fxcm", "mixnet") for nm, r, at in d["stages"] if r == 2), d["stages"]
    wx = [c for c in range(len(lay)) if int(lay[c, 0]) == 3 and int(lay[c, 1]) == 9]
    assert wx[0] in d["columns"] and all(int(lay[c, 0]) in (0, 3) for c in d["columns"]), d["names"]   # fxcm's own columns, and the network that read its output
    later = [k for k in range(3, len(pos)) if words[k, wx[0]] != journalled["words"][k, wx[0]]]
    spread = [k for k in range(3, len(pos)) if np.any(words[k] != journalled["words"][k])]
    print("the flipped wx column differs in later records %r; any column in %r" % (later, spread))
    assert later or spread, "a flipped weight left no trace in any later record"
    r = subprocess.run([sys.executable, "-m", "cmix_amd.journal", "state-diff", journalled["path"], path], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 1 and "first difference in record 2" in r.stdout and "fxcm region 9 (wx) array 0" in r.stdout, r.stdout + r.stderr
    assert "fxcm     record 2" in r.stdout


def test_a_decoding_handle_is_refused():
    from cmix_amd import engine as E
    _release()
    pipe = E.Pipeline(VOCAB, 0, 512)
    try:
        pipe.enable_fxcm(None)
        pipe.enable_paq8()
        pipe.set_state_journal(1)
        with pytest.raises(E.CmxError, match="does not cover a decoder"):
            pipe.late_start(0)
        pipe.set_state_journal(0)
        assert len(pipe.state_layout()) == pipe.state_digest().shape[0]
    finally:
        pipe.close()
