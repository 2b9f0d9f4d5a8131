"""Verify mode on / off through the whole engine (EngineStream) on shard prefixes: wall time, the mixing network's HIP-event time per chunk, SHA-256
(profiles/r07_verify_mode.txt). Usage: gpu_verify_measure.py SIZES MODES [OUT.json], e.g. 262144,1048576 0,1 -- every size with every mode, in order."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402


def one(n, rich, verify):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=rich))
    eng = EngineStream(0, stream, 4096, verify=verify)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
        rep = eng.pipe.verify_report()
    finally:
        eng.close()
    bits = 8 * len(stream)
    return {"bytes": len(stream), "rich": rich, "verify": verify, "wall_s": round(wall, 3), "us_per_bit_stream": round(wall * 1e6 / bits, 4),
            "mixnet_ms_per_chunk": round(st["mixnet"], 3), "mixnet_us_per_bit": round(st["mixnet"] * 1e3 * st["chunks"] / bits, 4), "chunks": st["chunks"],
            "size": len(blob), "sha256": hashlib.sha256(blob).hexdigest(), "report": rep}


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1].split(",")]
    modes = [m == "1" for m in sys.argv[2].split(",")]
    out = []
    for n in sizes:
        for v in modes:
            r = one(n, n >= (1 << 20), v)
            print(json.dumps(r), flush=True)
            out.append(r)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)
