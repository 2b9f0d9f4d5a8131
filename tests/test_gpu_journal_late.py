"""GPU: a DECODER's stream journal. The late-bit pipeline runs in a process of its own (as in test_gpu_late.py: it needs every stage kernel of the stream
running at once). The child replays the bits of text_96 through cmx_predict / cmx_perceive with the journal on at blocks of 2^8 bits; the host-side fold
(no decoder kernel knows of it) must give the reference's p and bits words -- the model on the fixture's p_final and bits --, and a handle held to that journal with one p word
changed (cmx_set_journal_check) must stop at that block. (A decode held to an unchanged journal running through: test_gpu_journal_dropin.py.)"""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu

_CHILD = r'''
import sys, os, tempfile
import numpy as np
sys.path.insert(0, {root!r})
from cmix_amd import engine as E, journal as J
with np.load(os.path.join({golden!r}, "text_96.npz")) as z:
    g = {{k: z[k] for k in z.files}}
bits = np.ascontiguousarray(g["bits"], np.uint8)
want_e, want = J.digests(None, None, bits, g["p_final"], 0, 8)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "dec.txt")

def replay(setup):
    P = E.Predictor(g["vocab"], 0)
    try:
        setup(P)
        for t in range(len(bits)):
            p = P.Predict()
            assert np.float32(p).view(np.uint32) == g["p_final"][t].view(np.uint32), "p differs at bit %d" % t
            P.Perceive(int(bits[t]))
            if t == 300:
                P.journal_write_files(path)   # mid-run: the complete blocks so far
                assert len(open(path).readlines()) == 1
        P.journal_write_files(path)
        P.journal_close_files()
    finally:
        P.close()

if {mode!r} == "journal":
    replay(lambda P: P.set_journal(8))
    ends, words = J.read(path)
    assert np.array_equal(ends, want_e), (ends, want_e)
    assert np.array_equal(words[:, J.W_P], want[:, J.W_P]), "the decoder's p words != the reference's"
    assert np.array_equal(words[:, J.W_BITS], want[:, J.W_BITS]), "the decoder's bits words != the reference's"
    assert not words[:, :130].any() and not words[:, J.W_SEL:J.W_BITS].any()
else:   # held to the reference's journal with one p word of block 1 changed: stops there, and says so
    ref = os.path.join(tmp, "ref.txt")
    bad = want.copy()
    bad[1, J.W_P] ^= np.uint64(1)
    J.write(ref, want_e, bad)
    try:
        replay(lambda P: P.set_journal_check(ref))
    except E.CmxError as e:
        assert "block 1 (bytes 32..63)" in str(e) and "the p word differs" in str(e), str(e)
        print("stopped:", e)
    else:
        raise SystemExit("a changed p word of block 1 went unnoticed")
print("OK")
'''


def _child(mode):
    load_golden("text_96")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, golden=GOLDEN, mode=mode)], capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-2000:] + "\n" + r.stderr[-3000:]


def test_decoder_journal_equals_reference():
    _child("journal")


def test_decoder_held_to_a_changed_journal_stops_at_the_block():
    _child("check")
