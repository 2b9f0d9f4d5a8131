"""Shadow mixing networks 0 / 1 / 2 through the whole engine (EngineStream) on a shard prefix in one process: wall time, B/s, the mixing network's
HIP-event time per chunk, SHA-256, the vote's report; then the vote kernels' time per chunk and one state_diff call, timed with HIP events on standalone
handles (profiles/r08_shadow_vote.txt). Usage: gpu_shadow_measure.py SIZE MODES [OUT.json], e.g. 1048576 0,1,2."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cmix_amd import engine as E  # noqa: E402
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402


def one(n, rich, shadow):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=rich))
    eng = EngineStream(0, stream, 4096, shadow=shadow)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        rep = eng.pipe.shadow_report()["raw"]
    finally:
        eng.close()
    bits = 8 * len(stream)
    return {"bytes": len(stream), "shadow": shadow, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "us_per_bit_stream": round(wall * 1e6 / bits, 4),
            "mixnet_ms_per_chunk": round(st["mixnet"], 3), "chunks": st["chunks"], "size": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "vote": rep}


def kernels():
    """the vote on a full 32 768-bit chunk (n = 2, 3; mean of 20 calls after 3) and one state_diff of two fresh handles, in ms"""
    import torch
    T = 32768
    out = {}
    for n in (2, 3):
        p = [torch.rand(T, device="cuda") for _ in range(n)]          # independent arrays: every element differs, every wave takes its atomics
        m = [torch.rand((T, 47), device="cuda") for _ in range(n)]    # (the worst case for the kernel)
        v = E.Vote(n)
        for _ in range(3):
            v.run(p, m, 0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            v.run(p, m, 0)
        b.record()
        torch.cuda.synchronize()
        out["vote_ms_per_chunk_n%d" % n] = round(a.elapsed_time(b) / 20, 4)
        v.close()
    x, y = E.MixNet(0), E.MixNet(0)
    x.state_diff(y)
    t0 = time.perf_counter()
    d = x.state_diff(y)
    out["state_diff_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["state_diff_words"] = d["words"]
    x.close()
    y.close()
    return out


if __name__ == "__main__":
    n = int(sys.argv[1])
    modes = [int(m) for m in sys.argv[2].split(",")]
    out = []
    for k in modes:
        r = one(n, n >= (1 << 20), k)
        print(json.dumps(r), flush=True)
        out.append(r)
    r = kernels()
    print(json.dumps(r), flush=True)
    out.append(r)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)
