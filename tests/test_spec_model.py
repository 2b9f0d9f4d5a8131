"""The CPU model of the speculative chain (tests/spec_model.py, oracle/spec_probe.c) against the oracle, and the conditions under which the GPU
tests of tests/test_gpu_spec_chain.py mean something: the streams they run must take every resolve path, often enough, and every crafted
row must be of the class it claims. Nothing here needs a GPU."""
import numpy as np
import pytest

import spec_model as S


def test_model_chain_equals_the_oracle():
    """Mixer 0 has no extra inputs: the model's ordered sum of its 2078 products is Mixer::p_ itself, bit for bit. For every mixer, a segment
    resolved from the hit lane's candidate -- ord2f(f2ord((float)est) + lane - 32), run through the segment -- equals the serial run from the true start."""
    d = S.synthetic()
    r = d["recs"]
    assert r.shape == (S.SYNTH_T, S.N_MIX0)
    assert np.array_equal(r["sum"][:, 0], d["mix"][:, 0].view(np.uint32))
    assert np.array_equal(r["resolved"], r["serial"])
    assert np.array_equal(r["serial"][:, :, 2], r["sum"])
    # a hit's candidate IS the true start: the ordered-integer arithmetic of the model's offsets and the kernel's candidates agree
    hit = S.is_hit(r)
    assert np.array_equal((S.f2ord(r["centre"]) + r["offset"])[hit], S.f2ord(r["start"])[hit])
    # what the write-up calls unreachable: a true start of -0.0, a non-finite centre
    assert not (r["start"] == 0x80000000).any()
    assert (S.exponent(r["centre"]) != 0xff).all()


def test_model_against_a_plain_numpy_restatement():
    """The C model's true starts and whole sums from float32 cumulative sums of the same products, for products drawn at random and for
    the subnormal range (numpy adds float32 in order, one rounding per add)."""
    rng = np.random.default_rng(3)
    for scale in (1.0, 1e-3, 2.0 ** -140):
        prod = (rng.standard_normal(S.N_IN0) * scale).astype(np.float32)
        rec = S.from_products(prod)
        run = np.cumsum(prod, dtype=np.float32)
        assert [int(v) for v in rec["start"]] == [int(run[k - 1].view(np.uint32)) for k in (512, 1024, 1536)]
        assert int(rec["sum"]) == int(run[-1].view(np.uint32))
        for q in range(3):
            est = np.float32(prod[:512 * (q + 1)].astype(np.float64).sum())   # any order: the terms are few enough to add exactly here
            if scale == 2.0 ** -140:
                assert int(rec["centre"][q]) == int(est.view(np.uint32))       # exact sums of subnormals: centre == true start
                assert int(rec["offset"][q]) == 0


def test_synthetic_stream_takes_every_resolve_path():
    """Coverage CONDITIONS of the 512-bit stream that tests/test_gpu_spec_chain.py runs: without them its equalities could hold vacuously.
    The model's figures on synth_mixnet_inputs(512, seed=11): 39 936 speculative segments, re-runs 474 / 537 / 853."""
    r = S.synthetic()["recs"]
    c = S.counts(r)
    print("model, synthetic %d bits seed %d: %s" % (S.SYNTH_T, S.SYNTH_SEED, c))
    assert c["segments"] == 3 * S.N_MIX0 * S.SYNTH_T and c["hits"] + sum(c["reruns"]) == c["segments"]
    off, hit = r["offset"], S.is_hit(r)
    for q in range(3):
        for o in (-33, -32, 31, 32):       # the last hit and the first miss on either side of the window
            assert int((off[:, :, q] == o).sum()) >= 5, (q + 1, o)
        assert int((np.abs(off[:, :, q]) > 1000).sum()) >= 5, q + 1
    assert sorted(set((off[hit] + 32).tolist())) == list(range(64)), "a candidate lane never resolves"
    assert int((~hit).all(axis=2).sum()) >= 5, "triple misses"
    assert (~hit).any(axis=0).all(), "a (mixer, segment) never re-runs"
    assert hit.any(axis=0).all()


def _rec(case, d):
    return d["recs"][case.bit, case.mixer]


@pytest.mark.parametrize("kind", ["binade", "edge", "zero", "seam", "tail"])
def test_crafted_rows_are_what_they_claim(kind):
    d = S.crafted()
    cases = [c for c in d["cases"] if c.claim[0] == kind]
    assert cases
    for c in cases:
        r = _rec(c, d)
        q = None if c.segment is None else c.segment - 1
        # the crafted mixer's row is fresh (extra weights zero): its output is the model's ordered sum, and the resolve is exact
        assert int(r["sum"]) == int(d["mix"][c.bit, c.mixer].view(np.uint32)), c
        assert np.array_equal(r["resolved"], r["serial"]), c
        if kind == "binade":
            _, what, below = c.claim
            one = 0x3f800000
            s, ce, off = int(r["start"][q]), int(r["centre"][q]), int(r["offset"][q])
            assert S.exponent(s) != S.exponent(ce), c
            assert (s < one <= ce) if below else (ce < one <= s), c
            assert abs(s - one) <= 3, c                                 # "just" below / at the power of two
            if what == "hit":
                assert -32 <= off <= 31 and off != 0, c                  # through a lane other than 32
            else:
                assert not (-32 <= off <= 31), c
            assert (r["offset"][:q] == 0).all(), c                       # the segments before it: plain hits through lane 32
        elif kind == "edge":
            assert int(r["offset"][q]) == c.claim[1], c
            assert (r["offset"][:q] == 0).all(), c
        elif kind == "zero":
            _, true_units, centre_units = c.claim
            sub = lambda u: (abs(u) | (0x80000000 if u < 0 else 0))
            assert int(r["start"][q]) == sub(true_units) and int(r["centre"][q]) == sub(centre_units), c
            # ordered integers across zero: -k units -> -k - 1, +k units -> k (so -0.0 and +0.0 are two candidates)
            o = lambda u: u if u >= 0 else u - 1
            assert int(r["offset"][q]) == o(true_units) - o(centre_units) and -32 <= int(r["offset"][q]) <= 31, c
            assert int(r["sum"]) == sub(true_units), c                   # the chain keeps f32 subnormals
        elif kind == "seam":
            s = c.claim[1]
            x = np.float32(0.25) * _x()
            assert int(r["sum"]) == int(x.view(np.uint32)), c            # (big + -big) + small
            assert (r["offset"] == 0).all(), c
            if s < 2048:
                assert S.exponent(int(r["start"][s // 512 - 1])) == 127 + 24, c   # the seam's wave starts from `big`
        else:
            assert (r["start"] == 0).all() and (r["offset"] == 0).all(), c        # nothing before element 2048
            assert len(c.weights) == c.claim[1] and min(c.weights) >= 2048 and int(r["sum"]) != 0, c
    # every other layer-0 mixer of a crafted bit but the auxiliary-context one runs on an all-zero row: 0.0 from lane 32
    for c in d["cases"]:
        others = [m for m in range(S.N_MIX0) if m not in (c.mixer, S.AUX_MIXER)]
        assert (d["recs"]["offset"][c.bit, others] == 0).all() and (d["recs"]["sum"][c.bit, others] == 0).all()


def _x():
    from oracle import oracle as O
    return O.stretch(S.CRAFT_P)


def test_tail_terms_each_move_the_sum():
    """The tail case is only a test of the last wave's 30 extra terms if dropping any one of them, or the zero pad behind them turning up
    as a term, changes the sum."""
    case = [c for c in S.crafted_cases() if c.claim == ("tail", 30)][0]
    prod = np.zeros(S.N_IN0, np.float32)
    for i, w in case.weights.items():
        prod[i] = _x() * w
    full = int(S.from_products(prod)["sum"])
    for i in case.weights:
        p = prod.copy()
        p[i] = 0
        assert int(S.from_products(p)["sum"]) != full, i
    swapped = prod.copy()
    swapped[[2049, 2050]] = swapped[[2050, 2049]]
    assert int(S.from_products(swapped)["sum"]) != full


def test_set_weight_twin():
    """orc_mixnet_set_weight: the value lands in the row the key selects (created if new), bit for bit, subnormals included."""
    from oracle import oracle as O
    probs = np.full(S.N_IN0, S.CRAFT_P, np.float32)
    sel = np.full(S.N_MIX, 7, np.uint64)
    for w in (np.float32(0.5), np.float32(-2.0 ** -140), np.array([0x80000000], np.uint32).view(np.float32)[0]):
        net = O.MixNet()
        net.set_weight(3, 7, 100, w)
        _, mix = net.step(probs, sel, 0, want_mix=True)
        assert int(mix[3].view(np.uint32)) == int((np.float32(_x() * w) + np.float32(0)).view(np.uint32))
        assert mix[2] == 0 and mix[4] == 0
        with pytest.raises(ValueError):
            net.set_weight(3, 7, S.N_IN0, w)
        with pytest.raises(ValueError):
            net.set_weight(47, 7, 0, w)
        net.close()
