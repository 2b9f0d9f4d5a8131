"""Shadow LSTM stages 0 / 1 / 2 through the whole engine (EngineStream) on a shard prefix in one process, RUNS runs each: wall time, B/s, the LSTM
stage's and the mixing network's HIP-event time per chunk, SHA-256, the LSTM vote's report; then (with a fifth argument "kernels") the vote kernels'
time per 4096-byte chunk and the device memory one shadow adds (profiles/r17_lstm_shadow.txt). A tree without the feature (the parent commit) runs
mode 0 only.
Usage: gpu_lstm_shadow_measure.py SIZE MODES RUNS [OUT.json [kernels]], e.g. 1048576 0,1,2 3."""
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
    eng = EngineStream(0, stream, 4096, lstm_shadow=k) if k else EngineStream(0, stream, 4096)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        rep = eng.pipe.lstm_shadow_report()["raw"] if k else [0] * 8
    finally:
        eng.close()
    bits = 8 * len(stream)
    return {"bytes": len(stream), "lstm_shadow": k, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "us_per_bit_stream": round(wall * 1e6 / bits, 4),
            "lstm_ms_per_chunk": round(st["lstm"], 3), "mixnet_ms_per_chunk": round(st["mixnet"], 3), "chunks": st["chunks"], "size": len(blob),
            "sha256": hashlib.sha256(blob).hexdigest(), "vote": rep}


def kernels():
    """the LSTM vote on a full 4096-byte chunk (n = 2, 3; agreeing instances = every chunk of a healthy stream, and independent random arrays = every
    element differs and every wave takes its atomics; mean of 20 calls after 3), and the device memory one LSTM handle takes, in MB"""
    import torch
    N = 4096
    out = {}
    for n in (2, 3):
        for name, same in (("agree", True), ("all_differ", False)):
            layer0 = torch.rand((8 * N, E.N_INPUTS), device="cuda")
            dist = torch.rand((N, 256), device="cuda")
            ex = torch.randint(0, 256, (N, 8), dtype=torch.int32, device="cuda")
            dists, ps, exs = [dist], [layer0], [ex]
            for _ in range(1, n):
                dists.append(dist.clone() if same else torch.rand((N, 256), device="cuda"))
                ps.append(layer0[:, E.N_INPUTS - 1].reshape(N, 8).contiguous() if same else torch.rand((N, 8), device="cuda"))
                exs.append(ex.clone() if same else torch.randint(256, 512, (N, 8), dtype=torch.int32, device="cuda"))
            v = E.LstmVote(n)
            for _ in range(3):
                v.run(dists, ps, exs, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                v.run(dists, ps, exs, 0)
            b.record()
            torch.cuda.synchronize()
            out["lstmvote_ms_per_chunk_n%d_%s" % (n, name)] = round(a.elapsed_time(b) / 20, 4)
            assert (v.report()["events"] == 0) == same
            v.close()
    torch.cuda.synchronize()
    vocab = np.ones(256, np.uint8)
    free0 = torch.cuda.mem_get_info()[0]   # hipMemGetInfo
    h = E.Lstm(vocab, 0)
    free1 = torch.cuda.mem_get_info()[0]
    out["lstm_handle_MB_V256"] = round((free0 - free1) / 1e6, 1)
    out["state_words_V256"] = sum(a["words"] for a in E.lstm_layout(h))
    out["per_slot_buffers_MB_4096B_chunk"] = round(E.PIPELINE_SLOTS * 4096 * (256 + 8 + 8) * 4 / 1e6, 1)
    g = E.Lstm(vocab, 0)
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
    if len(sys.argv) > 5 and sys.argv[5] == "kernels" and hasattr(E, "LstmVote"):
        r = kernels()
        print(json.dumps(r), flush=True)
        out.append(r)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)
