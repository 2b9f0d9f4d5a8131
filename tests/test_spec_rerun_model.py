"""CPU: the numpy model of the split re-run (tests/spec_rerun_model.py) against spec_model's C model where they overlap, and the coverage that
tests/test_gpu_spec_rerun.py relies on: the shared synthetic stream and the crafted rows together take BOTH mid-point paths in every segment."""
import numpy as np

import spec_model as S
import spec_rerun_model as R


def test_wave_sum_is_the_c_models_tree():
    """on one-hot and random vectors the numpy tree equals the sum (exactly representable inputs: any order gives the same value) and, for products
    of a real mix, the start offsets formed with it equal the C model's (below)"""
    rng = np.random.default_rng(3)
    v = rng.integers(-2 ** 20, 2 ** 20, 64).astype(np.float64)
    assert R.wave_sum(v) == v.sum()
    for i in (0, 1, 15, 16, 63):
        e = np.zeros(64); e[i] = 1.5
        assert R.wave_sum(e) == 1.5


def test_start_offsets_agree_with_spec_model_on_the_synthetic_stream():
    d, r = S.synthetic(), R.synthetic()
    assert np.array_equal(r["recs"]["offset"], d["recs"]["offset"])
    assert np.array_equal(r["rr"]["start_offset"], d["recs"]["offset"])
    assert np.array_equal(r["rr"]["miss"], ~S.is_hit(d["recs"]))
    c = R.counts(r["rr"])
    print("synthetic stream: re-runs %s, per segment (mid hits, serial halves) %s" % (S.counts(d["recs"])["reruns"], R.paths(r["rr"])))
    assert c["mid_hits"] + c["serial_halves"] == sum(S.counts(d["recs"])["reruns"])


def test_crafted_rows_take_the_path_they_are_built_for():
    d = R.crafted()
    for c in d["cases"]:
        rr, rec = d["rr"][c.bit, c.mixer], d["recs"][c.bit, c.mixer]
        print("%-72s mixer %2d start %-18s mid %-14s hit %s" % (c.name, c.mixer, list(map(int, rr["start_offset"])), list(map(int, rr["mid_offset"])), list(map(bool, rr["mid_hit"]))))
        assert np.array_equal(rr["start_offset"], rec["offset"]), c
        for q, claim in c.claim.items():
            assert rr["miss"][q - 1], (c, q)
            if claim is None:
                continue
            path, off = claim
            assert bool(rr["mid_hit"][q - 1]) == (path == "mid"), (c, q, int(rr["mid_offset"][q - 1]))
            if off is not None:
                assert int(rr["mid_offset"][q - 1]) == off, (c, q, int(rr["mid_offset"][q - 1]))
        others = np.delete(np.arange(R.N_MIX0), [c.mixer, S.AUX_MIXER])
        assert not d["rr"]["miss"][c.bit, others].any(), c     # every other mixer of the bit (but the auxiliary-context one, which learns): all-zero rows, every segment a hit


def test_both_paths_are_taken_in_every_segment():
    syn, cr = R.paths(R.synthetic()["rr"]), R.paths(R.crafted()["rr"])
    print("per segment (mid hits, serial halves): synthetic %s, crafted %s" % (syn, cr))
    for q in range(3):
        assert syn[q][0] + cr[q][0] > 0 and syn[q][1] + cr[q][1] > 0, (q + 1, syn, cr)
