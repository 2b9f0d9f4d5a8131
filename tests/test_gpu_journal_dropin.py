"""GPU: the stream journal through the command-line program (oracle/_ref/cmix_dropin: the reference's runner, coder and preprocessor over
integration/predictor_dropin.h and libcmixamd.so; the same skip rule as test_gpu_dropin.py where it is not built). The 12 KB text vector with blocks
of 2^13 bits (1 KB): `-c` with CMIX_JOURNAL still writes the reference binary's file, and leaves the two journal files; `-d` with CMIX_JOURNAL_CHECK
round-trips, and its own journal (CMIX_JOURNAL on -d) has the compressor's p and bits words; with one p word of block 3 changed in the journal file `-d`
stops with a non-zero exit and names block 3."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from cmix_amd import journal as J

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")
K = 13


def _missing(what):
    import torch
    if torch.cuda.is_available():
        pytest.fail(what + " (build oracle/_ref with `make -C oracle` before taking the snapshot to the GPU box)")
    pytest.skip(what)


def _dropin(mode, src, dst, env):
    return subprocess.run([DROPIN, mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, **env))


def test_compress_journal_then_checked_decodes(tmp_path):
    if not os.path.exists(DROPIN):
        _missing("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    with np.load(os.path.join(GOLDEN, "dropin_vectors.npz")) as z:
        payload, want_file = z["text12k_c_payload"].tobytes(), z["text12k_c_file"].tobytes()
    src, packed, jr = str(tmp_path / "in"), str(tmp_path / "packed"), str(tmp_path / "journal.txt")
    with open(src, "wb") as f:
        f.write(payload)
    # -c: the file is the reference binary's, and the journal is there
    r = _dropin("-c", src, packed, {"CMIX_JOURNAL": jr, "CMIX_JOURNAL_LOG2": str(K)})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-600:]
    assert open(packed, "rb").read() == want_file
    ends, words = J.read(jr)
    nblk = len(ends)
    assert nblk >= 12 and [int(e) for e in ends[:-1]] == [1024 * (i + 1) for i in range(nblk - 1)] and 1024 * (nblk - 1) < int(ends[-1]) <= 1024 * nblk
    assert int(ends[-1]) >= len(payload)   # the preprocessed stream: the payload behind its block header
    assert words.all()   # every one of the 179 words of every block was digested (selector 12 is a column of zeros: (0 + 1) * B)
    # -d held to that journal round-trips; its own journal has the compressor's p and bits words
    back, dj = str(tmp_path / "back"), str(tmp_path / "dec.txt")
    r = _dropin("-d", packed, back, {"CMIX_JOURNAL_CHECK": jr, "CMIX_JOURNAL": dj})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-600:]
    assert open(back, "rb").read() == payload
    dends, dwords = J.read(dj)
    assert np.array_equal(dends, ends) and np.array_equal(dwords[:, J.W_P], words[:, J.W_P]) and np.array_equal(dwords[:, J.W_BITS], words[:, J.W_BITS])
    d = J.first_difference((ends, words), (dends, dwords))
    assert d["block"] == 0 and d["kind"] == "selector 0"   # (a decoder's journal has no selector and no column words)
    # one p word of block 3 changed in the journal file: the decode stops there
    bad = words.copy()
    bad[3, J.W_P] ^= np.uint64(1 << 17)
    J.write(jr, ends, bad)
    back2 = str(tmp_path / "back2")
    r = _dropin("-d", packed, back2, {"CMIX_JOURNAL_CHECK": jr})
    err = r.stderr.decode(errors="replace")
    assert r.returncode != 0, "a changed p word went unnoticed"
    assert "block 3 (bytes 3072..4095)" in err and "the p word differs" in err, err[-600:]
