"""CPU: the four votes' rule modules (cmix_amd/vote.py, ctxvote.py, lstmvote.py, fxcmvote.py) are fronts of ONE rule (cmix_amd/votecore.py): fed their
stage's own array forms of the same stack w [n, 9, COLS], each returns exactly what votecore.vote_rule and chunk_rule return on w. The stacks, their
perturbations and the stage forms are shared with tests/test_gpu_vote_core.py, which runs the device's core (cmix_amd/csrc/cmx_vote_core.h) on them."""
import functools

import numpy as np
import pytest

from cmix_amd import ctxvote, fxcmvote, lstmvote, vote
from cmix_amd.votecore import NONE, VoteTwin, chunk_rule, vote_rule

ROWS = 9   # three workgroups of four one-row waves, the last one partial
COLS = {"mixnet": vote.COLS, "ctx": ctxvote.COLS, "lstm": lstmvote.COLS, "fxcm": fxcmvote.COLS}
CASES = ("clean", "one", "three", "same_odd")


@functools.lru_cache(maxsize=None)
def _base(cols, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (ROWS, cols), dtype=np.uint64).astype(np.uint32)


def stack(stage, n, case, seed=7):
    """w [n, 9, COLS]: n copies of one random chunk, then the case's differences.
    one: row 4, a middle column, the last instance. three: row 8 column 0 (instance 1), row 0 last column (instance 2; n = 2: instance 1), row 4 column
    0 (all three differ; n = 2: differ). same_odd: rows 0 and 8, both with instance 1 odd."""
    cols = COLS[stage]
    w = np.stack([_base(cols, seed)] * n).copy()
    if case == "one":
        w[n - 1, 4, cols // 2] ^= np.uint32(1)
    elif case == "three":
        w[1, 8, 0] ^= np.uint32(0x80000000)
        w[n - 1, 0, cols - 1] ^= np.uint32(1)
        w[1, 4, 0] ^= np.uint32(2)
        if n == 3:
            w[2, 4, 0] ^= np.uint32(4)
    elif case == "same_odd":
        w[1, 0, 1] ^= np.uint32(8)
        w[1, 8, cols - 2] ^= np.uint32(16)
    else:
        assert case == "clean"
    return w


def _inside(words, width, at, seed):
    """words [T, k] inside a [T, width] matrix of other words, at columns `at`"""
    m = np.random.default_rng(seed).integers(0, 1 << 32, (words.shape[0], width), dtype=np.uint64).astype(np.uint32)
    m[:, at] = words
    return m


def arrays(stage, w):
    """the stack in the stage's own array forms, as they lie in device memory: a dict of lists, one entry per instance. Instance 0 has the in-place
    form of the pipeline's main instance: layer-0 rows of 2078 words for ctx, lstm and fxcm."""
    n = w.shape[0]
    if stage == "mixnet":
        return {"ps": [w[i, :, 47].copy() for i in range(n)], "mixes": [w[i, :, :47].copy() for i in range(n)]}
    if stage == "ctx":
        probs = [_inside(w[i, :, :54], 2078, ctxvote.LAYER0_COLS, 30) if i == 0 else _inside(w[i, :, :54], 64, slice(0, 54), 31 + i) for i in range(n)]
        return {"probs": probs, "compact": [i != 0 for i in range(n)], "sels": [w[i, :, 54:].copy() for i in range(n)]}
    if stage == "lstm":
        bit_ps = [_inside(w[i, :, 256:264].reshape(-1, 1), 2078, slice(2077, 2078), 40) if i == 0 else w[i, :, 256:264].reshape(-1).copy() for i in range(n)]
        return {"dists": [w[i, :, :256].copy() for i in range(n)], "bit_ps": bit_ps, "exs": [w[i, :, 264:].copy() for i in range(n)]}
    assert stage == "fxcm"
    return {"rows": [_inside(w[i], 2078 if i == 0 else 434, slice(3, 434), 50 + i) for i in range(n)]}


def reference(stage, a, unit0):
    """(record, words, chunk result) by the stage's own module"""
    if stage == "mixnet":
        args = (a["ps"], a["mixes"])
        return vote.vote_reference(*args, unit0) + (vote.chunk_result(*args, unit0),)
    if stage == "ctx":
        args = ([ctxvote.model_outputs(p, c) for p, c in zip(a["probs"], a["compact"])], a["sels"])
        return ctxvote.ctx_vote_reference(*args, unit0) + (ctxvote.chunk_result(*args, unit0),)
    if stage == "lstm":
        args = (a["dists"], a["bit_ps"], a["exs"])
        return lstmvote.lstm_vote_reference(*args, unit0) + (lstmvote.chunk_result(*args, unit0),)
    return fxcmvote.fxcm_vote_reference(a["rows"], unit0) + (fxcmvote.chunk_result(a["rows"], unit0),)


def brute_force(w, unit0):
    """the rule element by element in plain Python, written from its statement (no numpy comparison): (record, chunk result)"""
    n, rows, cols = w.shape
    first, count, odds = None, 0, set()
    for t in range(rows):
        for c in range(cols):
            v = [int(w[i, t, c]) for i in range(n)]
            if len(set(v)) == 1:
                continue
            odd = NONE   # two instances that differ, or three different values
            if n == 3 and len(set(v)) == 2:
                odd = [i for i in range(3) if v.count(v[i]) == 1][0]
            count += 1
            odds.add(odd)
            if first is None:
                first = [unit0 + t, c, odd]
    if first is None:
        return [1, rows, n, 0, 0, 0, 0, 0], [0, 0, 0, 0]
    return [1, rows, n, 1] + first + [count], [count, first[0], first[1], odds.pop() if len(odds) == 1 else NONE]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [2, 3])
def test_the_one_rule_is_the_rule_element_by_element(n, case):
    for stage in ("mixnet", "ctx"):
        w = stack(stage, n, case)
        assert (vote_rule(w, 77)[0], chunk_rule(w, 77)) == brute_force(w, 77)
    rng = np.random.default_rng(n)   # and on small values, where every kind of element occurs many times
    w = rng.integers(0, 2, (n, 5, 7), dtype=np.uint64).astype(np.uint32)
    assert (vote_rule(w, 3)[0], chunk_rule(w, 3)) == brute_force(w, 3)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("stage", sorted(COLS))
def test_every_front_is_the_one_rule(stage, n, case):
    w = stack(stage, n, case)
    rec, words, chunk = reference(stage, arrays(stage, w), 1000)
    want_rec, want_words = vote_rule(w, 1000)
    assert rec == want_rec and chunk == chunk_rule(w, 1000)
    assert (words is None and want_words is None) or (words.dtype == np.uint32 and np.array_equal(words, want_words))
    # and the rule says what the cases were built to show
    last = COLS[stage] - 1
    if case == "clean":
        assert rec == [1, ROWS, n, 0, 0, 0, 0, 0] and words is None and chunk == [0, 0, 0, 0]
    elif case == "one":
        assert rec == [1, ROWS, n, 1, 1004, COLS[stage] // 2, n - 1 if n == 3 else NONE, 1] and chunk == [1, 1004, COLS[stage] // 2, rec[6]]
    elif case == "three":
        assert rec == [1, ROWS, n, 1, 1000, last, 2 if n == 3 else NONE, 3] and chunk == [3, 1000, last, NONE]
        assert np.array_equal(words, w[:, 0, :])
    else:
        assert rec == [1, ROWS, n, 1, 1000, 1, 1 if n == 3 else NONE, 2] and chunk == [2, 1000, 1, rec[6]]


@pytest.mark.parametrize("n", [2, 3])
def test_the_twin_keeps_the_first_event_over_chunks(n):
    tw = VoteTwin(n)
    assert tw.run(stack("ctx", n, "three"), 1000) == [3, 1000, 100, NONE]
    first = list(tw.record)
    assert tw.run(stack("ctx", n, "same_odd", 8), 1009) == [2, 1009, 1, 1 if n == 3 else NONE]
    assert tw.run(stack("ctx", n, "clean", 9), 1018) == [0, 0, 0, 0]
    assert tw.record == [3, 3 * ROWS, n, 2] + first[4:] and np.array_equal(tw.words, stack("ctx", n, "three")[:, 0, :])
    with pytest.raises(ValueError, match="%d instances" % n):
        tw.run(stack("ctx", 5 - n, "clean"), 0)
