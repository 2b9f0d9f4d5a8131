"""Every stage stream of an engine on a hardware queue of its own, whatever GPU_MAX_HW_QUEUES says (include/cmix_amd.h, section 3).

HIP multiplexes plain streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and kernels of streams that share a queue run
one after the other. The library creates every stream with a compute-unit mask (cmx_make_stream), which HIP never pools, and checks
with the overlap probe that the stage streams really run at once. Each case runs in a fresh process started with
GPU_MAX_HW_QUEUES=4 (the suite's conftest raises the variable for its own process, so the children set it back).
"""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_HEAD = r'''
import hashlib, os, sys
import numpy as np
sys.path.insert(0, {root!r})
import torch
assert torch.cuda.is_available()   # HIP starts here, with the child's GPU_MAX_HW_QUEUES
assert os.environ["GPU_MAX_HW_QUEUES"] == "4"
from cmix_amd import engine as E, synth
from cmix_amd.pipeline import EngineStream, text_file_stream
'''


def _run_child(body, timeout=900, **fmt):
    code = _HEAD.format(root=ROOT) + body.format(**fmt)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    sys.stdout.write(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:] + "\n" + r.stderr[-3000:])
    return r.stdout


_CODE_128K = r'''
with np.load({fixture!r}) as z:
    want_sha, want_size, (n, seed) = z["sha256"].tobytes(), int(z["size"][0]), z["seed"]
eng = EngineStream(0, text_file_stream(synth.enwik_like(int(n), int(seed), rich=True)), 4096)
assert eng.pipe.stage_overlap(), "the overlap probe saw stage streams that share a hardware queue"
assert E.hw_queues(0) == 13, E.hw_queues(0)
eng.feed(1 << 30)
blob = eng.finish()
eng.close()
assert E.hw_queues(0) == 0, E.hw_queues(0)
assert len(blob) == want_size and hashlib.sha256(blob).digest() == want_sha, "the 128 KB file differs from the reference binary's"
print("OK 128 KB:", len(blob), "bytes, every stage stream concurrent")
'''


def test_probe_and_128k_file_at_4_queues():
    """the probe reports every stage stream concurrent, and the 128 KB file is the reference binary's (tests/golden/dropin_rich_128k_s1001.npz)"""
    _run_child(_CODE_128K, fixture=os.path.join(GOLDEN, "dropin_rich_128k_s1001.npz"))


_DECODE_50K = r'''
stream = bytes(text_file_stream(synth.enwik_like(50000, 1000, rich=True)))
eng = EngineStream(0, stream, 4096)
eng.feed(len(stream))
blob = eng.finish()
eng.close()
length, dic, vocab, hl = E.header_read(blob)
p = E.Predictor(vocab, 0)
out = p.decode_stream(blob[hl:], length)
p.close()
assert out == stream, "the decoded bytes differ"
print("OK 50 KB round trip:", length, "bytes")
'''


def test_decode_round_trip_50k_at_4_queues():
    """the decoder needs all 14 stage kernels of a chunk running at once: with 4 pooled queues it would time out inside its launches"""
    _run_child(_DECODE_50K)


_TWO_ENGINES = r'''
a = EngineStream(0, text_file_stream(synth.enwik_like(8192, 1000, rich=True)), 4096)
b = EngineStream(0, text_file_stream(synth.enwik_like(8192, 1001, rich=True)), 4096)
assert a.pipe.stage_overlap() and b.pipe.stage_overlap(), "an engine's stage streams share a hardware queue"
assert E.hw_queues(0) == 26, E.hw_queues(0)
for e in (a, b):
    e.feed(1 << 30)
    e.finish()
    e.close()
assert E.hw_queues(0) == 0, E.hw_queues(0)
print("OK two engines, 26 queues")
'''


def test_two_engines_in_one_process_at_4_queues():
    _run_child(_TWO_ENGINES)
