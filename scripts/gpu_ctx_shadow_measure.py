"""Shadow context stages 0 / 1 / 2 through the whole engine (EngineStream) on a shard prefix in one process, RUNS runs each: wall time, B/s, the context
stage's and the mixing network's HIP-event time per chunk, SHA-256, the context vote's report; then the vote kernels' time per 32 768-bit chunk and the
device memory one shadow adds (profiles/r13_ctx_shadow.txt). A tree without the feature (the parent commit) runs mode 0 only.
Usage: gpu_ctx_shadow_measure.py SIZE MODES RUNS [OUT.json], e.g. 1048576 0,1,2 3."""
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


def one(n, rich, k):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=rich))
    eng = EngineStream(0, stream, 4096, ctx_shadow=k) if k else EngineStream(0, stream, 4096)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        rep = eng.pipe.ctx_shadow_report()["raw"] if k else [0] * 8
    finally:
        eng.close()
    bits = 8 * len(stream)
    return {"bytes": len(stream), "ctx_shadow": k, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "us_per_bit_stream": round(wall * 1e6 / bits, 4),
            "ctx_ms_per_chunk": round(st["ctxmodels"], 3), "mixnet_ms_per_chunk": round(st["mixnet"], 3), "chunks": st["chunks"], "size": len(blob),
            "sha256": hashlib.sha256(blob).hexdigest(), "vote": rep}


def kernels():
    """the context vote on a full 32 768-bit chunk (n = 2, 3; agreeing instances = every chunk of a healthy stream, and independent random arrays = every
    element differs and every wave takes its atomics; mean of 20 calls after 3), and the device memory one compact handle takes, in MB"""
    import torch
    T = 32768
    out = {}
    for n in (2, 3):
        for name, same in (("agree", True), ("all_differ", False)):
            full = torch.rand((T, E.N_INPUTS), device="cuda")
            sel = torch.randint(0, 1 << 31, (T, 47), dtype=torch.int32, device="cuda")
            probs, sels = [full], [sel]
            for _ in range(1, n):
                c = torch.rand((T, 64), device="cuda")
                if same:
                    c[:, :3] = full[:, :3]
                    c[:, 3:54] = full[:, 2025:2076]
                probs.append(c)
                sels.append(sel.clone() if same else torch.randint(0, 1 << 31, (T, 47), dtype=torch.int32, device="cuda"))
            compact = [False] + [True] * (n - 1)
            v = E.CtxVote(n)
            for _ in range(3):
                v.run(probs, compact, sels, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                v.run(probs, compact, sels, 0)
            b.record()
            torch.cuda.synchronize()
            out["ctxvote_ms_per_chunk_n%d_%s" % (n, name)] = round(a.elapsed_time(b) / 20, 4)
            assert (v.report()["events"] == 0) == same
            v.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]   # hipMemGetInfo
    h = E.CtxModels(np.ones(256, np.uint8), 0, compact=True)
    free1 = torch.cuda.mem_get_info()[0]
    out["compact_handle_MB"] = round((free0 - free1) / 1e6, 1)
    out["per_slot_buffers_MB_4096B_chunk"] = round(E.PIPELINE_SLOTS * 32768 * (64 + 47) * 4 / 1e6, 1)
    g = E.CtxModels(np.ones(256, np.uint8), 0)
    h.state_diff(g)
    t0 = time.perf_counter()
    d = h.state_diff(g)
    out["state_diff_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["state_diff_words"] = d["words"]
    h.close()
    g.close()
    return out


if __name__ == "__main__":
    n = int(sys.argv[1])
    modes = [int(m) for m in sys.argv[2].split(",")]
    runs = int(sys.argv[3])
    out = []
    for _ in range(runs):   # (the modes interleaved: a drift of the box over the session spreads over all of them)
        for k in modes:
            r = one(n, n >= (1 << 20), k)
            print(json.dumps(r), flush=True)
            out.append(r)
    if hasattr(E, "CtxVote"):
        r = kernels()
        print(json.dumps(r), flush=True)
        out.append(r)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)
