"""GPU: the resolve paths of cmx_mixnet_spec_kernel's speculative chain, pinned one by one against the CPU model (tests/spec_model.py).

tests/test_gpu_mixnet.py sees end results only; a resolve that always re-runs, a candidate window off by one, or a resolve that is wrong only
for an edge lane, across a binade or across zero would pass it. Here the device's own counters (MixNet.spec_stats(): segments, hits, re-runs
of segment 1, 2, 3) must EQUAL the model's on a 512-bit stream that takes every path (tests/test_spec_model.py asserts that it does), in
every run-time form of the kernel; and crafted rows, built by weight injection on both sides (MixNet.debug_state_xor on the device,
orc_mixnet_set_weight in the oracle), put one named path at a time through the kernel: the mixer's output bit for bit and the exact counter
increments of that bit."""
import numpy as np
import pytest

import spec_model as S

pytestmark = pytest.mark.gpu


def _device_inputs(d):
    import torch
    return (torch.from_numpy(np.array(d["probs"])).cuda(),
            torch.from_numpy((d["sel"] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.array(d["bits"])).cuda())


def _run_synthetic(cuts=(), verify=False, tolerance=False):
    """the shared 512-bit stream on a fresh handle -> p, mix, [(bits done, spec_stats) after every launch], verify report"""
    import torch
    from cmix_amd import engine as E
    d = S.synthetic()
    T = S.SYNTH_T
    d_probs, d_sel, d_bits = _device_inputs(d)
    net = E.MixNet(0)
    try:
        if verify:
            net.set_verify(True)
        if tolerance:
            net.set_tolerance(True)
        p = torch.empty(T, dtype=torch.float32, device="cuda")
        mix = torch.empty((T, S.N_MIX), dtype=torch.float32, device="cuda")
        edges = sorted(set([0, T] + list(cuts)))
        stats = []
        for a, b in zip(edges[:-1], edges[1:]):
            net.run(d_probs[a:b], d_sel[a:b], d_bits[a:b], p[a:b], mix[a:b])
            stats.append((b, S.stats_of(net.spec_stats())))   # (synchronises the device)
        assert net.bits_done() == T
        report = net.verify_report() if verify else None
        return p.cpu().numpy(), mix.cpu().numpy(), stats, report
    finally:
        net.close()


def _check_outputs(p, mix, d, what):
    bad = np.argwhere(mix.view(np.uint32) != d["mix"].view(np.uint32))
    assert bad.size == 0, "%s: first differing (bit, mixer) %s" % (what, bad[0])
    bad = np.nonzero(p.view(np.uint32) != d["p"].view(np.uint32))[0]
    assert bad.size == 0, "%s: final p differs first at bit %d" % (what, bad[0])


def _check_stats(stats, what):
    recs = S.synthetic()["recs"]
    for done, got in stats:
        want = S.counts(recs[:done])
        print("%-28s after %3d bits  model %s  device %s" % (what, done, want, got))
        assert got == want, "%s, after %d bits: device %s, model %s" % (what, done, got, want)


def test_synthetic_outputs_and_counters_equal_the_model():
    """One launch of 512 bits: p and all 47 mixer outputs are the oracle's, and segments == 3 * 26 * 512, hits and the three re-run counts are
    the model's -- equalities: the estimate is a deterministic function of the products."""
    p, mix, stats, _ = _run_synthetic()
    _check_outputs(p, mix, S.synthetic(), "one launch")
    assert stats[-1][1]["segments"] == 3 * 26 * 512
    _check_stats(stats, "one launch")


def test_counters_accumulate_over_ragged_cuts():
    """The counters are cumulative per handle: after every one of the ragged launches they equal the model's over the bits done so far."""
    p, mix, stats, _ = _run_synthetic(cuts=[1, 2, 9, 64, 65, 300, 511])
    _check_outputs(p, mix, S.synthetic(), "ragged cuts")
    assert [b for b, _ in stats] == [1, 2, 9, 64, 65, 300, 511, 512]
    _check_stats(stats, "ragged cuts")


@pytest.mark.parametrize("switch", ["CMX_MIXNET_JITTER=5", "CMX_MIXNET_XCD=2"])
def test_counters_under_kernel_switches(monkeypatch, switch):
    """The jitter form (pseudo-random stalls in every role) and the one-XCD placement resolve every segment the same way."""
    name, val = switch.split("=")
    monkeypatch.setenv(name, val)
    p, mix, stats, _ = _run_synthetic()
    _check_outputs(p, mix, S.synthetic(), switch)
    _check_stats(stats, switch)


def test_counters_in_verify_form():
    p, mix, stats, report = _run_synthetic(verify=True)
    _check_outputs(p, mix, S.synthetic(), "verify form")
    _check_stats(stats, "verify form")
    assert report["mismatches"] == 0 and report["bits"] == S.SYNTH_T, report


def test_tolerance_mode_does_not_speculate():
    """Tolerance mode sums every segment as a tree: no candidates, no resolve, every counter stays 0."""
    _, _, stats, _ = _run_synthetic(tolerance=True)
    print("tolerance mode: device", stats[-1][1])
    assert stats[-1][1] == {"segments": 0, "hits": 0, "reruns": [0, 0, 0]}


# ---------------------------------------------------------------------------------------------------------------- crafted rows
@pytest.fixture(scope="module")
def crafted_device():
    """The crafted stream on one handle: every case's weights injected into the row its bit will select (a mixer's rows are numbered in order of
    first touch: bit c's key c is row c), then one launch per bit with the counters read after each."""
    import torch
    from cmix_amd import engine as E
    d = S.crafted()
    T = len(d["cases"])
    d_probs, d_sel, d_bits = _device_inputs(d)
    net = E.MixNet(0)
    try:
        for c in d["cases"]:
            assert c.mixer != S.AUX_MIXER
            for i, w in sorted(c.weights.items()):
                net.debug_state_xor("rows0", c.mixer, c.bit, i, int(np.float32(w).view(np.uint32)))   # the row is zero memory: XOR sets the pattern
        p = torch.empty(T, dtype=torch.float32, device="cuda")
        mix = torch.empty((T, S.N_MIX), dtype=torch.float32, device="cuda")
        stats = [S.stats_of(net.spec_stats())]
        for t in range(T):
            net.run(d_probs[t:t + 1], d_sel[t:t + 1], d_bits[t:t + 1], p[t:t + 1], mix[t:t + 1])
            stats.append(S.stats_of(net.spec_stats()))
        assert net.bits_done() == T
        return {"p": p.cpu().numpy(), "mix": mix.cpu().numpy(), "stats": stats}
    finally:
        net.close()


def _delta(a, b):
    return {"segments": b["segments"] - a["segments"], "hits": b["hits"] - a["hits"], "reruns": [y - x for x, y in zip(a["reruns"], b["reruns"])]}


@pytest.mark.parametrize("index", range(S.N_CRAFTED))
def test_crafted_row(crafted_device, index):
    """One crafted case: the mixer's output (the ordered sum of its 2078 products) and every other output of the bit are the oracle's bit for
    bit, and the counters moved by exactly what the model says for this bit's 78 speculative segments."""
    d = S.crafted()
    c = d["cases"][index]
    got = crafted_device["mix"][c.bit].view(np.uint32)
    want = d["mix"][c.bit].view(np.uint32)
    r = d["recs"][c.bit, c.mixer]
    delta = _delta(crafted_device["stats"][c.bit], crafted_device["stats"][c.bit + 1])
    model = S.counts(d["recs"][c.bit])
    print("%-62s mixer %2d offsets %-16s sum model %08x device %08x  counters model %s device %s"
          % (c.name, c.mixer, list(map(int, r["offset"])), int(r["sum"]), int(got[c.mixer]), model, delta))
    assert int(got[c.mixer]) == int(want[c.mixer]) == int(r["sum"]), c
    assert np.array_equal(got, want), (c, np.nonzero(got != want)[0])
    assert int(crafted_device["p"][c.bit].view(np.uint32)) == int(d["p"][c.bit].view(np.uint32)), c
    assert delta == model, (c, delta, model)
