"""The stream journal off / on through the whole engine (EngineStream) on a shard prefix in one process, RUNS runs each, interleaved: wall time, B/s, the
mixing network's HIP-event time per chunk, the file's SHA-256 (must not change) and a SHA-256 over the journal's words (must not change from run to
run); then the journal kernel alone on a full 32 768-bit chunk (profiles/r16_journal.txt).
Usage: gpu_journal_measure.py SIZE LOG2S RUNS [OUT.json], e.g. 1048576 0,19 3     (LOG2S: 0 = journal off)
       gpu_journal_measure.py kernel [CALLS]     only the kernel on random rows: the target of a `rocprofv3 --kernel-trace --stats` run of its own"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cmix_amd import engine as E  # noqa: E402
from cmix_amd import journal as J  # noqa: E402
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402


def one(n, rich, k, out_dir=None, tag=""):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=rich))
    eng = EngineStream(0, stream, 4096, journal=k) if k else EngineStream(0, stream, 4096)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        jr = eng.journal() if k else None
    finally:
        eng.close()
    r = {"bytes": len(stream), "journal_log2": k, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "mixnet_ms_per_chunk": round(st["mixnet"], 3),
         "ctx_ms_per_chunk": round(st["ctxmodels"], 3), "chunks": st["chunks"], "size": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}
    if jr is not None:
        r["journal_blocks"] = len(jr[0])
        r["journal_sha256"] = hashlib.sha256(np.ascontiguousarray(jr[0]).tobytes() + np.ascontiguousarray(jr[1]).tobytes()).hexdigest()
        if out_dir:
            J.write(os.path.join(out_dir, "journal_%d%s.txt" % (n, tag)), *jr)
    return r


def kernel(calls=20):
    """cmx_journal_run on a full chunk of random words, all four arrays: HIP-event time around `calls` calls (each call also waits for its copy and folds on
    the host, so this is an upper bound of the kernel's time; the kernel's own duration is what rocprofv3 reports for cmx_journal_kernel)"""
    import torch
    T = 32768
    rows = torch.rand((T, E.N_INPUTS), device="cuda")
    sel = torch.randint(0, 1 << 31, (T, 47), dtype=torch.int32, device="cuda")
    bits = torch.randint(0, 2, (T,), dtype=torch.uint8, device="cuda")
    p = torch.rand(T, device="cuda")
    j = E.Journal(0, 19)
    t = 0
    for _ in range(3):
        j.run(rows, sel, bits, p, t)
        t += T
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        j.run(rows, sel, bits, p, t)
        t += T
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / calls
    j.close()
    nbytes = T * (E.N_INPUTS * 4 + 47 * 4 + 1 + 4)
    return {"journal_call_ms_per_chunk": round(ms, 4), "chunk_bytes_read": nbytes, "GB_per_s_per_call": round(nbytes / ms / 1e6, 1)}


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        print(json.dumps(kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 20)), flush=True)
        sys.exit(0)
    n = int(sys.argv[1])
    modes = [int(m) for m in sys.argv[2].split(",")]
    runs = int(sys.argv[3])
    out_dir = os.path.dirname(os.path.abspath(sys.argv[4])) if len(sys.argv) > 4 else None
    out = []
    for i in range(runs):   # (the modes interleaved: a drift of the box over the session spreads over both)
        for k in modes:
            r = one(n, n >= (1 << 20), k, out_dir, "_run%d" % i)
            print(json.dumps(r), flush=True)
            out.append(r)
    r = kernel()
    print(json.dumps(r), flush=True)
    out.append(r)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(out, f, indent=1)
