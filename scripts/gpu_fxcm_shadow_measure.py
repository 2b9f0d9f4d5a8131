"""Shadow fxcm stages 0 / 1 / 2 through the whole engine (EngineStream) on a shard prefix in one process, RUNS runs each: wall time, B/s, the fxcm
stage's, the LSTM stage's and the mixing network's HIP-event time per chunk, SHA-256, the fxcm vote's report; then (with a fifth argument "kernels")
the vote kernels' time per 32768-bit chunk with the bandwidth it implies, the construction time and device memory of one shadow, the state diff's
time (profiles/r19_fxcm_shadow.txt). A tree without the feature (the parent commit) runs mode 0 only.
Usage: gpu_fxcm_shadow_measure.py SIZE MODES RUNS [OUT.json [kernels]], e.g. 1048576 0,1,2 3."""
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
    eng = EngineStream(0, stream, 4096, fxcm_shadow=k) if k else EngineStream(0, stream, 4096)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        fx_ms = eng.pipe.fxcm_total_ms() / max(st["chunks"], 1)
        rep = eng.pipe.fxcm_shadow_report()["raw"] if k else [0] * 8
    finally:
        eng.close()
    bits = 8 * len(stream)
    return {"bytes": len(stream), "fxcm_shadow": k, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "us_per_bit_stream": round(wall * 1e6 / bits, 4),
            "fxcm_ms_per_chunk": round(fx_ms, 3), "fxcm_us_per_bit": round(fx_ms * 1e3 / 32768, 4), "lstm_ms_per_chunk": round(st["lstm"], 3),
            "mixnet_ms_per_chunk": round(st["mixnet"], 3), "chunks": st["chunks"], "size": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "vote": rep}


def kernels():
    """the fxcm vote on a full 4096-byte chunk = 32768 rows (n = 2, 3; agreeing instances = every chunk of a healthy stream, and independent random
    rows = every element differs and every wave takes its atomics; mean of 20 calls after 3; instance 0 in place in layer-0 rows), the bytes it reads
    and the bandwidth that implies; the construction time of one shadow, the device memory it takes, the state diff's time"""
    import torch
    T = 8 * 4096
    out = {}
    for n in (2, 3):
        for name, same in (("agree", True), ("all_differ", False)):
            layer0 = torch.rand((T, E.N_INPUTS), device="cuda")
            rows = [layer0]
            for _ in range(1, n):
                r = torch.rand((T, 434), device="cuda")
                if same:
                    r[:, 3:434] = layer0[:, 3:434]
                rows.append(r)
            v = E.FxcmVote(n)
            for _ in range(3):
                v.run(rows, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                v.run(rows, 0)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 20
            out["fxcmvote_ms_per_chunk_n%d_%s" % (n, name)] = round(ms, 4)
            out["fxcmvote_GBps_n%d_%s" % (n, name)] = round(n * T * 431 * 4 / ms / 1e6, 1)
            assert (v.report()["events"] == 0) == same
            v.close()
    out["fxcmvote_MB_read_n3"] = round(3 * T * 431 * 4 / 1e6, 1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]   # hipMemGetInfo
    t0 = time.perf_counter()
    h = E.Fxcm(device=0, shadow=True)
    out["shadow_construction_s"] = round(time.perf_counter() - t0, 3)
    free1 = torch.cuda.mem_get_info()[0]
    out["shadow_handle_MB"] = round((free0 - free1) / 1e6, 1)
    out["state_words"] = sum(a["words"] for a in E.fxcm_layout(h))
    out["per_slot_row_buffers_MB_4096B_chunk_per_shadow"] = round(E.PIPELINE_SLOTS * 8 * 4096 * 434 * 4 / 1e6, 1)
    g = E.Fxcm(device=0, shadow=True)
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
    if len(sys.argv) > 5 and sys.argv[5] == "kernels" and hasattr(E, "FxcmVote"):
        r = kernels()
        print(json.dumps(r), flush=True)
        out.append(r)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)
