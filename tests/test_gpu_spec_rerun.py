"""GPU: the split re-run of cmx_mixnet_spec_kernel's speculative chain against its numpy model (tests/spec_rerun_model.py).

A missed segment is re-run as two speculative halves inside its wave (helper_role's miss branch): lane 0 the first 256 terms from the true
start, lanes 1..63 the rest from 63 candidate mid-points; it resolves at the mid-point or runs the second half serially. Either way the sum
must be the oracle's bit for bit, the old counters (MixNet.spec_stats()) must move as spec_model.counts says, and the two new ones
(MixNet.spec_rerun_stats(): mid hits, serial halves) exactly as the numpy model says -- on crafted rows that put one path at a time
through the kernel (one-bit launches, weight injection on both sides), and on the shared 512-bit stream in the plain, jitter and verify
forms, in one launch and in ragged cuts.

The window of the mid-point is -31..+31 (lane j = 1..63 starts from centre + j - 32; lane 0 runs the first half), so the edge cases are
-31 / +31 (and +30) inside, -32 / -33 / +32 outside."""
import numpy as np
import pytest

import spec_model as S
import spec_rerun_model as R

pytestmark = pytest.mark.gpu


def _device_inputs(d):
    import torch
    return (torch.from_numpy(np.array(d["probs"])).cuda(),
            torch.from_numpy((d["sel"] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.array(d["bits"])).cuda())


def _both(net):
    return S.stats_of(net.spec_stats()), net.spec_rerun_stats()


# ---------------------------------------------------------------------------------------------------------------- crafted rows
@pytest.fixture(scope="module")
def crafted_device():
    """The crafted stream on one handle: every case's weights injected into the row its bit will select, then one launch per bit with
    both sets of counters read after each."""
    import torch
    from cmix_amd import engine as E
    d = R.crafted()
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
        stats = [_both(net)]
        for t in range(T):
            net.run(d_probs[t:t + 1], d_sel[t:t + 1], d_bits[t:t + 1], p[t:t + 1], mix[t:t + 1])
            stats.append(_both(net))
        assert net.bits_done() == T
        return {"p": p.cpu().numpy(), "mix": mix.cpu().numpy(), "stats": stats}
    finally:
        net.close()


def _delta(a, b):
    return ({"segments": b[0]["segments"] - a[0]["segments"], "hits": b[0]["hits"] - a[0]["hits"], "reruns": [y - x for x, y in zip(a[0]["reruns"], b[0]["reruns"])]},
            {k: b[1][k] - a[1][k] for k in ("mid_hits", "serial_halves")})


@pytest.mark.parametrize("index", range(R.N_CRAFTED))
def test_crafted_row(crafted_device, index):
    """One crafted case: the mixer's output (the ordered sum of its 2078 products) and every other output of the bit are the oracle's bit for
    bit; the old counters moved by what spec_model.counts says for the bit's 78 segments, the new ones by what the numpy model says."""
    d = R.crafted()
    c = d["cases"][index]
    got = crafted_device["mix"][c.bit].view(np.uint32)
    want = d["mix"][c.bit].view(np.uint32)
    r, rr = d["recs"][c.bit, c.mixer], d["rr"][c.bit, c.mixer]
    old, new = _delta(crafted_device["stats"][c.bit], crafted_device["stats"][c.bit + 1])
    m_old, m_new = S.counts(d["recs"][c.bit]), R.counts(d["rr"][c.bit])
    print("%-74s mixer %2d start %-16s mid %-14s sum model %08x device %08x  counters model %s %s device %s %s"
          % (c.name, c.mixer, list(map(int, r["offset"])), list(map(int, rr["mid_offset"])), int(r["sum"]), int(got[c.mixer]), m_old, m_new, old, new))
    assert int(got[c.mixer]) == int(want[c.mixer]) == int(r["sum"]), c
    assert np.array_equal(got, want), (c, np.nonzero(got != want)[0])
    assert int(crafted_device["p"][c.bit].view(np.uint32)) == int(d["p"][c.bit].view(np.uint32)), c
    assert old == m_old, (c, old, m_old)
    assert new == m_new, (c, new, m_new)


# ---------------------------------------------------------------------------------------------------------------- the synthetic stream
def _run_synthetic(cuts=(), verify=False):
    import torch
    from cmix_amd import engine as E
    d = S.synthetic()
    T = S.SYNTH_T
    d_probs, d_sel, d_bits = _device_inputs(d)
    net = E.MixNet(0)
    try:
        if verify:
            net.set_verify(True)
        p = torch.empty(T, dtype=torch.float32, device="cuda")
        mix = torch.empty((T, S.N_MIX), dtype=torch.float32, device="cuda")
        edges = sorted(set([0, T] + list(cuts)))
        stats = []
        for a, b in zip(edges[:-1], edges[1:]):
            net.run(d_probs[a:b], d_sel[a:b], d_bits[a:b], p[a:b], mix[a:b])
            stats.append((b,) + _both(net))
        assert net.bits_done() == T
        report = net.verify_report() if verify else None
        return p.cpu().numpy(), mix.cpu().numpy(), stats, report
    finally:
        net.close()


def _check(p, mix, stats, what):
    d, r = S.synthetic(), R.synthetic()
    bad = np.argwhere(mix.view(np.uint32) != d["mix"].view(np.uint32))
    assert bad.size == 0, "%s: first differing (bit, mixer) %s" % (what, bad[0])
    assert np.array_equal(p.view(np.uint32), d["p"].view(np.uint32)), what
    for done, old, new in stats:
        m_old, m_new = S.counts(d["recs"][:done]), R.counts(r["rr"][:done])
        print("%-22s after %3d bits  model %s %s  device %s %s" % (what, done, m_old, m_new, old, new))
        assert old == m_old, (what, done, old, m_old)
        assert new["mid_hits"] + new["serial_halves"] == sum(old["reruns"]), (what, done, new, old)
        assert new == m_new, (what, done, new, m_new)


CUTS = [1, 2, 9, 64, 65, 300, 511]


@pytest.mark.parametrize("form", ["plain", "jitter", "verify"])
@pytest.mark.parametrize("cuts", [(), tuple(CUTS)], ids=["one launch", "ragged cuts"])
def test_synthetic_stream(monkeypatch, form, cuts):
    if form == "jitter":
        monkeypatch.setenv("CMX_MIXNET_JITTER", "5")
    p, mix, stats, report = _run_synthetic(cuts=cuts, verify=form == "verify")
    assert [b for b, _, _ in stats] == sorted(set(list(cuts) + [S.SYNTH_T]))
    _check(p, mix, stats, "%s, %s" % (form, "ragged cuts" if cuts else "one launch"))
    if form == "verify":
        assert report["mismatches"] == 0 and report["bits"] == S.SYNTH_T, report
