"""GPU: the state journal through the command-line program (oracle/_ref/cmix_dropin, as tests/test_gpu_journal_dropin.py runs it; the same skip rule
where it is not built). The 12 KB text vector: `-c` with CMIX_STATE_JOURNAL still writes the reference binary's file and leaves the journal -- the
header with the layout, one record per chunk of 4096 bytes (CMIX_STATE_JOURNAL_EVERY=1) and one after the last --, a second run writes the same bytes,
and `-d` with the switch set says that the decoder is not covered and decodes as before."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from cmix_amd import journal as J

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(ROOT, "oracle", "_ref", "cmix_dropin")


def _missing(what):
    import torch
    if torch.cuda.is_available():
        pytest.fail(what + " (build oracle/_ref with `make -C oracle` before taking the snapshot to the GPU box)")
    pytest.skip(what)


def _dropin(mode, src, dst, env):
    return subprocess.run([DROPIN, mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, **env))


def test_compress_with_state_journal_then_decode(tmp_path):
    if not os.path.exists(DROPIN):
        _missing("oracle/_ref/cmix_dropin not built (make -C oracle dropin_engine)")
    with np.load(os.path.join(GOLDEN, "dropin_vectors.npz")) as z:
        payload, want_file = z["text12k_c_payload"].tobytes(), z["text12k_c_file"].tobytes()
    src, packed, sj = str(tmp_path / "in"), str(tmp_path / "packed"), str(tmp_path / "run.state")
    with open(src, "wb") as f:
        f.write(payload)
    # -c: the file is the reference binary's, and the state journal is there: a record after every chunk of 4096 bytes and one after the ragged last
    r = _dropin("-c", src, packed, {"CMIX_STATE_JOURNAL": sj, "CMIX_STATE_JOURNAL_EVERY": "1"})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-600:]
    assert open(packed, "rb").read() == want_file
    lay, pos, words = J.read_state(sj)
    n = int(pos[-1])   # the preprocessed stream: the payload behind its block header
    assert len(payload) <= n < len(payload) + 64
    assert [int(x) for x in pos] == [min(4096 * (i + 1), n) for i in range(-(-n // 4096))]
    assert sorted(set(int(x) for x in lay[:, 0])) == [0, 1, 2, 3, 4] and words.shape == (len(pos), len(lay))
    assert all(np.any(words[k] != words[k - 1]) for k in range(1, len(pos)))
    assert not os.path.exists(sj + ".inputs")   # a file of its own: nothing of the stream journal's pair
    # a second run writes the same journal, byte for byte
    packed2, sj2 = str(tmp_path / "packed2"), str(tmp_path / "run2.state")
    r = _dropin("-c", src, packed2, {"CMIX_STATE_JOURNAL": sj2, "CMIX_STATE_JOURNAL_EVERY": "1"})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-600:]
    assert open(packed2, "rb").read() == want_file
    assert open(sj2, "rb").read() == open(sj, "rb").read()
    assert J.first_state_difference(J.read_state(sj), J.read_state(sj2)) is None
    # -d with the switch set: not covered, said so, decoded as before; no file
    back, sj3 = str(tmp_path / "back"), str(tmp_path / "dec.state")
    r = _dropin("-d", packed, back, {"CMIX_STATE_JOURNAL": sj3})
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-600:]
    assert "does not cover a decoder" in err
    assert open(back, "rb").read() == payload
    assert not os.path.exists(sj3)
