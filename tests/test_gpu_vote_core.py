"""GPU: what the four votes share on the device (cmix_amd/csrc/cmx_vote_core.h) with MORE THAN ONE non-agreeing element in a chunk, in different
waves and workgroups: the cross-wave atomicMin / atomicAdd / atomicOr of the accumulator's flush and the fold's decision about last[3]. Nine rows are
three workgroups of four one-row waves, the last one partial; for the mixing network's vote 423 mixer words (105 quads + 3) and 9 p words (2 quads + 1).
Instance 0 has each stage's in-place form (tests/test_vote_core_rule.py: arrays); the mixing network's arrays start one row into their allocation,
so the single-word path runs, and once aligned, so the 16-byte path does. Expected values are the numpy twin's (cmix_amd/votecore.py)."""
import numpy as np
import pytest

from test_vote_core_rule import COLS, ROWS, arrays, stack

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NONE = (1 << 64) - 1
UNIT0 = 1000


def _dev(a, lead=0):
    """a numpy array of words on the device, `lead` rows into its allocation"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32))
    buf = torch.zeros((t.shape[0] + lead,) + tuple(t.shape[1:]), dtype=torch.int32, device="cuda")[lead:]
    buf.copy_(t)
    return buf


class _Run:
    """one vote handle of a stage; run(w, unit0) votes the stack in the stage's array forms and returns the extras its capture should hold"""

    def __init__(self, stage, n, lead):
        import torch
        from cmix_amd import engine as E
        self.stage, self.lead = stage, lead
        self.v = {"mixnet": E.Vote, "ctx": E.CtxVote, "lstm": E.LstmVote, "fxcm": E.FxcmVote}[stage](n)
        self.sel = torch.arange(ROWS * 47, dtype=torch.int32, device="cuda") * 2654435 % 1000003
        self.bytes = (torch.arange(ROWS, device="cuda") * 37 % 251 + 1).to(torch.uint8)

    def run(self, w, unit0, row):
        a = {k: [_dev(x, self.lead) if not isinstance(x, bool) else x for x in xs] for k, xs in arrays(self.stage, w).items()}
        by = [int(x) for x in self.bytes.cpu()]
        if self.stage == "mixnet":
            self.v.run(a["ps"], a["mixes"], unit0, self.sel, self.bytes)
            return {"bit": by[row], "sel": self.sel.cpu().numpy().view(np.uint32)[47 * row:47 * row + 47]}
        if self.stage == "ctx":
            self.v.run(a["probs"], a["compact"], a["sels"], unit0, self.bytes)
            return {"bit": by[row]}
        if self.stage == "lstm":
            self.v.run(a["dists"], a["bit_ps"], a["exs"], unit0, self.bytes)
            return {"byte": by[row]}
        self.v.run(a["rows"], unit0, self.bytes)
        return {"byte": by[row >> 3], "bit": (by[row >> 3] >> (7 - (row & 7))) & 1}


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("stage,lead", [("mixnet", 1), ("mixnet", 0), ("ctx", 0), ("lstm", 0), ("fxcm", 0)])
def test_several_elements_in_several_workgroups(stage, lead, n):
    from cmix_amd.votecore import VoteTwin
    last_col = COLS[stage] - 1
    tw, r = VoteTwin(n), _Run(stage, n, lead)
    try:
        # (a) row 8 column 0 (instance 1), row 0 last column (instance 2), row 4 column 0 (all differ): three elements, no ONE odd instance
        w = stack(stage, n, "three")
        tw.run(w, UNIT0)
        assert tw.record == [1, ROWS, n, 1, UNIT0, last_col, 2 if n == 3 else NONE, 3] and tw.last == [3, UNIT0, last_col, NONE]
        extras = r.run(w, UNIT0, 0)
        rep, val = r.v.report()["raw"], r.v.values()
        assert rep == tw.record and rep[7] == 3, (rep, tw.record)
        assert r.v.last()["raw"] == tw.last
        assert np.array_equal(val["words"], tw.words)
        for k, x in extras.items():
            assert np.array_equal(val[k], x), (k, val[k], x)
        # (b) two elements, rows 0 and 8, both with instance 1 odd: the chunk has ONE odd instance
        w = stack(stage, n, "same_odd", 8)
        tw.run(w, UNIT0 + ROWS)
        assert tw.last == [2, UNIT0 + ROWS, 1, 1 if n == 3 else NONE]
        r.run(w, UNIT0 + ROWS, 0)
        assert r.v.last()["raw"] == tw.last and r.v.report()["raw"] == tw.record == [2, 2 * ROWS, n, 2] + rep[4:]
        # (c) a clean chunk: last is zero, the sticky fields stay
        w = stack(stage, n, "clean", 9)
        tw.run(w, UNIT0 + 2 * ROWS)
        r.run(w, UNIT0 + 2 * ROWS, 0)
        assert r.v.last()["raw"] == tw.last == [0, 0, 0, 0]
        assert r.v.report()["raw"] == tw.record == [3, 3 * ROWS, n, 2] + rep[4:]
        val = r.v.values()
        assert np.array_equal(val["words"], tw.words)
        for k, x in extras.items():
            assert np.array_equal(val[k], x), (k, val[k], x)
    finally:
        r.v.close()
