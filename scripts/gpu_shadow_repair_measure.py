"""Repair on the majority, measured (profiles/r09_shadow_repair.txt). Two parts, each a JSON line per result:

  kernels            cmx_mixnet_state_repair next to cmx_mixnet_state_diff on the same two handles (nothing differs, then a few thousand words differ):
                     HIP-event time around each call, mean and spread of REPS calls, and the GB/s that the 5.6 GB read implies
  engine SIZE MODES  the whole engine (EngineStream) on a shard prefix, one run per mode, in one process: off (no shadows), shadow2 (two shadows, no
                     repair), armed (two shadows, repair armed, no event), event (armed, one word of the stream's own network changed after chunk 20):
                     wall time, B/s, SHA-256, the vote's report, the repair log and, for `event`, the wall time of the wait that made the repair

Usage: gpu_shadow_repair_measure.py [--root DIR] kernels | engine SIZE off,shadow2,armed,event [REPEATS]
--root DIR imports cmix_amd from another checkout (the parent commit's, for the A/B of `off` and `shadow2`: it has no repair argument)."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 2 and sys.argv[1] == "--root":
    ROOT = os.path.abspath(sys.argv[2])
    del sys.argv[1:3]
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402,F401
from cmix_amd import engine as E  # noqa: E402
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402

REPS = 10
STATE_BYTES = 2 * 4 * (26 * 10001 * 2112 + 20 * 10001 * 64 + 10001 * 64 + 47 * 10001 * 2 + 2 * 47 * 32768 + (3 * 128 * 256 * 256 + 3 * 32 * 256 * 255) * 4
                       + 4 * 256 * 8 * 79 + 3 * 2 * 256 * 256)   # both handles' ten regions


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, r


def _stats(name, ev, wall, words):
    ev, wall = np.array(ev), np.array(wall)
    return {"call": name, "reps": len(ev), "event_ms_mean": round(float(ev.mean()), 3), "event_ms_min": round(float(ev.min()), 3), "event_ms_max": round(float(ev.max()), 3),
            "wall_ms_mean": round(float(wall.mean()), 3), "GBps_of_event_mean": round(STATE_BYTES / 1e6 / float(ev.mean()), 1), "words": words}


def kernels():
    import torch
    torch.zeros(1, device="cuda")
    x, y = E.MixNet(0), E.MixNet(0)
    try:
        x.state_diff(y)
        x.state_repair(y)
        for name, fn in (("state_diff, nothing differs", lambda: x.state_diff(y)), ("state_repair, nothing differs", lambda: x.state_repair(y))):
            ev, wall = [], []
            for _ in range(REPS):
                e, w, d = _timed(fn)
                ev.append(e)
                wall.append(w)
            print(json.dumps(_stats(name, ev, wall, d["words"])), flush=True)
        ev, wall, evd, walld = [], [], [], []
        for _ in range(REPS):   # 32 words of one layer-0 row differ
            for i in range(0, 2048, 64):
                x.debug_state_xor("rows0", 3, 7, i, 0x00400000)
            e, w, d0 = _timed(lambda: x.state_diff(y))
            evd.append(e)
            walld.append(w)
            e, w, d = _timed(lambda: x.state_repair(y))
            ev.append(e)
            wall.append(w)
            assert d["raw"] == d0["raw"] and x.state_diff(y)["words"] == 0
        print(json.dumps(_stats("state_diff, 32 words differ", evd, walld, d0["words"])), flush=True)
        print(json.dumps(_stats("state_repair, 32 words differ", ev, wall, d["words"])), flush=True)
    finally:
        x.close()
        y.close()


def one(n, mode):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=n >= (1 << 20)))
    kw = {"shadow": 0 if mode == "off" else 2}
    if mode in ("armed", "event"):
        kw["repair"] = 8
    eng = EngineStream(0, stream, 4096, **kw)
    stall = {}
    try:
        if mode == "event":
            wait = eng.pipe.wait

            def timed_wait(i):
                t0 = time.perf_counter()
                wait(i)
                dt = time.perf_counter() - t0
                if "ms" not in stall and eng.pipe.shadow_repairs()["total"]:
                    stall["ms"], stall["at_chunk"] = round(dt * 1e3, 2), i
                stall.setdefault("waits", []).append(round(dt * 1e3, 2))
            eng.pipe.wait = timed_wait
        t0 = time.perf_counter()
        if mode == "event":
            eng.feed(21 * 4096)
            eng.pipe.debug_shadow_xor(0, "rows1", 26, 0, 28, 0x00400000)
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        rep = eng.pipe.shadow_report()["raw"]
        log = eng.pipe.shadow_repairs() if "repair" in kw else None
    finally:
        eng.close()
    out = {"mode": mode, "bytes": len(stream), "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "size": len(blob),
           "sha256": hashlib.sha256(blob).hexdigest(), "vote": rep}
    if log is not None:
        out["repairs"] = log["total"]
        out["log"] = [e["text"] for e in log["log"]]
    if stall:
        w = sorted(stall.pop("waits"))
        out["repair_wait_ms"] = stall
        out["median_wait_ms"] = w[len(w) // 2]
    return out


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels()
    else:
        n = int(sys.argv[2])
        reps = int(sys.argv[4]) if len(sys.argv) > 4 else 1
        for _ in range(reps):
            for mode in sys.argv[3].split(","):
                print(json.dumps(one(n, mode)), flush=True)
