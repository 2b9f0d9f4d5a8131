"""The fxcm stage on the MI355X, through the C ABI (cmx_fxcm_create / _run): cmx_fxcm_chunk_kernel + the host text parser
against the oracle (oracle/fxcm_model.c) and against layer-0 columns 3..433 of the golden traces recorded from the
unmodified reference predictor -- all 431 values per bit, bit for bit. Same cases as tests/test_fxcm_stage_host.py, which
runs the kernel's body on the host (the data of the shared cases comes from that file's helpers), and what only the device
has: the position thresholds as the three roles restate them, lead and lag between the roles (CMX_FXCM_JITTER) under foreign
load, launches without a sync between them. (Named to sort after the other GPU tests: the stage was written after its
round's GPU budget was spent, so its first run on a device was the driver's.)"""
import numpy as np
import pytest

from conftest import load_golden
from test_fxcm_stage_host import (THRESHOLD_BACK, THRESHOLD_CUTS, THRESHOLDS, _poison_case, compare, dictionary_case, hints, oracle_rows, other_data_case,
                                  pretraining_case, threshold_case)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def run_device(data, lstmpr, lstmex, chunks, dictionary=None, blpos=0, sync_each=True, between=None, info=None):
    """One stream through a fresh handle, a launch per chunk. blpos: the handle starts there (cmx_fxcm_debug_set_blpos). sync_each=False: every
    tensor is made first, then all launches are issued on a stream of their own -- on torch's stream the copy of a chunk's bytes inside
    Fxcm.run would wait for the launch before it -- and the host syncs once at the end; cmx_fxcm_run still waits for the device itself
    whenever a launch is larger than every one before it (its row buffer regrows). between(): called after every launch is issued. info: a
    dict that receives the handle's jitter stall counts, ring waits and slot_parallel word. The fail flag (a bounded in-launch wait ran
    out) must stay clear."""
    import torch
    from cmix_amd import engine as E
    fx = E.Fxcm(dictionary, 0)
    try:
        if blpos:
            fx.debug_set_blpos(blpos)
        data = np.ascontiguousarray(data, np.uint8)
        cuts, pos = [], 0
        for n in chunks:
            n = min(n, len(data) - pos)
            if n <= 0:
                break
            cuts.append((pos, n))
            pos += n

        def tensors(pos, n):
            return (torch.from_numpy(np.ascontiguousarray(lstmpr[8 * pos:8 * (pos + n)], np.int16)).cuda(),
                    torch.from_numpy(np.ascontiguousarray(lstmex[8 * pos:8 * (pos + n)], np.uint8)).cuda(),
                    torch.full((8 * n, 434), -1.0, dtype=torch.float32, device="cuda"))

        held = []
        if sync_each:
            for pos, n in cuts:
                pr, ex, probs = tensors(pos, n)
                fx.run(data[pos:pos + n], pr, ex, probs)
                held.append((pr, ex, probs))
                if between:
                    between()
                fx.sync()
                assert not fx.failed(), "a bounded wait of the roles kernel ran out in the launch at byte %d" % pos
        else:
            held = [tensors(pos, n) for pos, n in cuts]
            torch.cuda.synchronize()   # the inputs were made on torch's stream
            side = torch.cuda.Stream()
            for (pos, n), (pr, ex, probs) in zip(cuts, held):
                fx.run(data[pos:pos + n], pr, ex, probs, stream=side.cuda_stream)
                if between:
                    between()
        fx.sync()
        torch.cuda.synchronize()
        assert not fx.failed(), "a bounded wait of the roles kernel ran out"
        outs = []
        for _, _, probs in held:
            got = probs.cpu().numpy()
            assert (got[:, :3] == -1.0).all()          # columns outside 3..433 are not the stage's
            outs.append(got[:, 3:434])
        if info is not None:
            info.update(jitter_counts=fx.debug_jitter_counts(), ring_waits=fx.debug_ring_waits(), slot_parallel=fx.debug_slot_parallel())
            try:   # the position hook is for a fresh handle only
                fx.debug_set_blpos(1)
                info["blpos_refused"] = False
            except E.CmxError:
                info["blpos_refused"] = True
    finally:
        fx.close()
    return np.ascontiguousarray(np.concatenate(outs))


def test_text_vs_oracle_ragged_chunks():
    from cmix_amd import synth
    data = np.frombuffer(synth.enwik_like(6000, 31), np.uint8)
    pr, ex = hints(8 * len(data), 7)
    compare(run_device(data, pr, ex, [1, 1, 7, 100, 1000, 3, 2000, 4000]), oracle_rows(data, pr, ex), "enwik-like text")


def test_binary_and_runs_vs_oracle():
    r = np.random.default_rng(5)
    runs = np.concatenate([np.full(int(n), int(v), np.uint8) for n, v in zip(r.integers(1, 40, 150), r.integers(0, 256, 150))])[:2000]
    data = np.concatenate([r.integers(0, 256, 2000).astype(np.uint8), runs])
    pr, ex = hints(8 * len(data), 11)
    compare(run_device(data, pr, ex, [512] * 8), oracle_rows(data, pr, ex), "binary + runs")


def test_golden_columns():
    import make_golden as mg
    from oracle import oracle as O
    g = load_golden("text_96")
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
    compare(run_device(np.asarray(stream, np.uint8), pr, ex, [len(stream)]), np.ascontiguousarray(probs[:, 3:434]), "text_96")


def test_long_text_properties():
    """64 KB of text at full table sizes: every value is on the k / 4095 grid the model exports, the final probability
    column tracks the data (coding cost well under 8 bits per byte), and two runs of the same stream are identical."""
    from cmix_amd import synth
    data = np.frombuffer(synth.enwik_like(65536, 77), np.uint8)
    pr, ex = hints(8 * len(data), 3)
    a = run_device(data, pr, ex, [4096] * 16)
    b = run_device(data, pr, ex, [65536])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    k = a[8:, :429] * np.float32(4095)                   # rows 0..7: the first byte's layout, 0.5 where no map has a context yet
    assert np.abs(k - np.round(k)).max() < 1e-3 and k.min() >= 0 and k.max() <= 4095.001 and (a[:, 429:] == 0.5).all()
    bits = np.unpackbits(data)
    p1 = np.clip(a[:, 428].astype(np.float64), 1 / 4096, 1 - 1 / 4096)   # the model's own final probability (last AddPrediction); an APM may return 0
    cost = -np.log2(np.where(bits == 1, p1, 1 - p1)).sum() / len(data)
    assert cost < 4.0, cost


# ---- what the host twin cannot run: fx_bit_dev and role M's copy of it, role X's APM update from the LDS row, the speculated APM contexts and
# next-update errors, the hand-offs between the workgroups ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", sorted(THRESHOLD_CUTS))
@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_block_position_thresholds_vs_oracle(threshold, cuts):
    """The five places fxcm reads its position in the block, on the stream that reacts to each (test_the_thresholds_matter), started 700 bytes
    below. The rates are restated three times on the device (fx_bit_dev, role M, role X's own APM update); the first update with
    blpos > threshold is the boundary bit of stream byte 700. "mid": the crossing inside a launch. "last": that update is its launch's last, so
    the look-aheads for the next update's APM contexts and mixer errors are skipped. "alone": byte 700 and byte 701 are launches of their own,
    the next launch starts without the APM rows in LDS and takes fxd_apm_update at the new rate; FxDev::blpos carries the position across."""
    data, pr, ex, want = threshold_case(threshold)
    got = run_device(data, pr, ex, THRESHOLD_CUTS[cuts], blpos=threshold - THRESHOLD_BACK)
    compare(got, want, "threshold %d, cuts %s" % (threshold, cuts))


_text3000 = {}


def _text3000_case():
    """3000 bytes of text, hints and the oracle's rows: once for the tests below"""
    if not _text3000:
        from cmix_amd import synth
        data = np.frombuffer(synth.enwik_like(3000, 31), np.uint8)
        pr, ex = hints(8 * len(data), 7)
        _text3000["case"] = (data, pr, ex, oracle_rows(data, pr, ex))
    return _text3000["case"]


def test_roles_bit_exact_under_jitter_and_foreign_load(monkeypatch):
    """Role X polls 17 counters and then reads row words that role M's 16 free-running wavefronts and role U stored just before moving their
    counter. On a quiet device M and U run far ahead; CMX_FXCM_JITTER makes every role stall at pseudo-random bits (up to ~100 us, far below
    the bound of any wait), so that X also arrives first and reads a row the moment its counter moves, and a step of foreign work
    (scripts/gpu_foreign_load.py, torch's stream) is issued behind every launch and shares the device with it. The stage's own launches do
    not overlap one another here (most of these chunks regrow the row buffer, for which cmx_fxcm_run waits for the device). Nothing of it
    may change a word: the clean run equals the oracle, every disturbed
    run the clean one, no wait runs out, and each of the 18 stall sites was live."""
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    from gpu_foreign_load import Foreign
    data, pr, ex, want = _poison_case()
    chunks = [1, 1, 7, 100, 1000, 3, 2000]

    def run(load, jitter):
        if jitter:
            monkeypatch.setenv("CMX_FXCM_JITTER", str(jitter))
        else:
            monkeypatch.delenv("CMX_FXCM_JITTER", raising=False)
        F = Foreign(load, torch.device("cuda", 0)) if load else None
        info = {}
        got = run_device(data, pr, ex, chunks, sync_each=False, between=F.step if F else None, info=info)
        print("load %s, jitter %s: stall counts %s, ring waits %d" % (load, jitter, info["jitter_counts"], info["ring_waits"]))
        return got, info["jitter_counts"]

    clean, counts = run(None, 0)
    compare(clean, want, "clean run")
    assert counts == [0] * 18, counts   # the product kernel has no stall sites
    for load, jitter in ((None, 3), (None, 9), ("all", 0), ("all", 12)):
        got, counts = run(load, jitter)
        compare(got, clean, "load %s, jitter %d" % (load, jitter))
        if jitter:
            assert len(counts) == 18 and min(counts) > 0, ("a stall site was never live", jitter, counts)


def test_one_lane_per_map_vs_oracle(monkeypatch):
    """CMX_FXCM_SERIAL_MAPS=1, the A/B fallback of the slot-parallel maps, on the device (the host twin runs it in test_text_vs_oracle_ragged_chunks)"""
    data, pr, ex, want = _text3000_case()
    info = {}
    run_device(data[:8], pr, ex, [8], info=info)
    assert info["slot_parallel"] == 1, info   # the product's path is the other one
    monkeypatch.setenv("CMX_FXCM_SERIAL_MAPS", "1")
    compare(run_device(data[:2500], pr, ex, [1, 7, 500, 1000, 2000], info=info), want, "one lane per map")
    assert info["slot_parallel"] == 0, ("the switch did not reach the model the kernels read", info)


def test_markup_vs_oracle():
    data, pr, ex = other_data_case("markup")
    compare(run_device(data, pr, ex, [512] * 8), oracle_rows(data, pr, ex), "markup")


def test_dictionary_mode_vs_oracle():
    import os
    data, pr, ex, path = dictionary_case()
    try:
        want = oracle_rows(data, pr, ex, dictionary=path)
        got = run_device(data, pr, ex, [300] * 10, dictionary=path)
    finally:
        os.unlink(path.decode())
    compare(got, want, "dictionary mode")


def test_pretraining_then_data_vs_oracle():
    data, pr, ex, chunks = pretraining_case()
    compare(run_device(data, pr, ex, chunks), oracle_rows(data, pr, ex), "pretraining + data")


def test_back_to_back_launches_without_sync():
    """Ten launches without a host sync between them, of growing sizes around role M's 64-byte window of the chunk's bytes (63, 64, 65): the
    growth paths. The row buffer regrows at launches 2, 3, 5 and 7, for which cmx_fxcm_run waits for the device itself, and launches 9 and 10
    take slots 0 and 1 of the staging ring again with larger chunks, so their record buffers regrow. No ring wait meets a launch in flight
    here (the two slots' first launches drained at those device waits): that is test_staging_ring_waits_for_launches_in_flight."""
    data, pr, ex, want = _text3000_case()
    chunks = [63, 64, 65, 1, 512, 2, 1024, 3, 700, 566]
    assert sum(chunks) == len(data)
    compare(run_device(data, pr, ex, chunks, sync_each=False), want, "back-to-back launches")


def test_staging_ring_waits_for_launches_in_flight():
    """The staging ring itself (used[b] / done[b], 8 slots taken in turn): one launch of 1000 bytes, after which nothing regrows, then sixteen
    of 125 bytes, all issued at once on one stream. Launches 9 to 17 take a slot whose previous launch is still queued behind the first
    (~50 ms of device time against the milliseconds it takes to issue them) and must wait for it before the slot's records are overwritten:
    without that wait the queued launch would read the later chunk's records. The handle counts the waits that met a launch in flight."""
    data, pr, ex, want = _text3000_case()
    chunks = [1000] + [125] * 16
    assert sum(chunks) == len(data)
    info = {}
    compare(run_device(data, pr, ex, chunks, sync_each=False, info=info), want, "seventeen launches on eight staging slots")
    print("ring waits that met a launch in flight: %d of 9 reuses" % info["ring_waits"])
    assert info["ring_waits"] > 0, ("no launch met its slot's previous launch in flight", info)
    assert info["blpos_refused"], "cmx_fxcm_debug_set_blpos accepted a stream that had begun"


# ---- the stage inside the chunk pipeline: cmx_pipeline_enable_fxcm --------------------------------------------------
# oracle/_ref/cmix_lookahead with CMX_FXCM_DEVICE=1: the reference's preprocessor and paq8 objects on the host, fxcm as a
# device stage fed by the LSTM stage's hints on the device (pretraining over the dictionary included). The files must
# equal the reference binary's byte for byte (tests/golden/dropin_vectors.npz).

def _lookahead(mode, files, timeout=900):
    import os
    import subprocess
    import tempfile
    from test_gpu_dropin import LOOKAHEAD
    if not os.path.exists(LOOKAHEAD):
        pytest.skip("oracle/_ref/cmix_lookahead not built (make -C oracle lookahead)")
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for name, data in files:
            p = os.path.join(d, name)
            with open(p, "wb") as f:
                f.write(data)
            paths.append(p)
        out = os.path.join(d, "out")
        r = subprocess.run([LOOKAHEAD, mode] + paths + [out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout,
                           env=dict(os.environ, CMX_FXCM_DEVICE="1"))
        assert r.returncode == 0, f"cmix_lookahead {mode} (fxcm on the device) failed: {r.stderr.decode(errors='replace')[-400:]}"
        with open(out, "rb") as f:
            return f.read()


def test_pipeline_with_device_fxcm_files_are_byte_identical():
    from test_gpu_dropin import _lookahead_vectors
    v = _lookahead_vectors()
    assert _lookahead("-n", [("in", v["raw_n_payload"])]) == v["raw_n_file"]
    assert _lookahead("-c", [("in", v["text_c_payload"])]) == v["text_c_file"]
    assert _lookahead("-c", [("in", v["text12k_c_payload"])]) == v["text12k_c_file"]


def test_pipeline_with_device_fxcm_dictionary_pretraining():
    from test_gpu_dropin import _lookahead_vectors
    v = _lookahead_vectors()
    assert _lookahead("-c", [("dict", v["dict_payload"]), ("in", v["dict_c_payload"])]) == v["dict_c_file"]


@pytest.mark.parametrize("name", ["fxcm_cols_wiki_16k", "fxcm_cols_dict_16k", "fxcm_cols_mixed_24k", "fxcm_cols_rich_16k"])
def test_reference_hashes_16k(name):
    """The device stage against the reference itself (not against its twin, the oracle): 16 KB of wiki markup and of
    dictionary-mode text, per-bit hashes of all 431 values recorded from the unmodified fxcmv1::Predictor
    (tests/golden/make_fxcm_hashes.py)."""
    import os
    from test_fxcm_stage_host import _reference_fixture
    data, pr, ex, dic, want, row_hash = _reference_fixture(name)
    try:
        got = row_hash(run_device(data, pr, ex, [4096, 1, 4095, 8192, 8192], dictionary=dic))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, "first differing bit", int(bad[0]))
    finally:
        if dic:
            os.unlink(dic.decode())
