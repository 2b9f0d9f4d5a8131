"""One whole-engine stream (EngineStream) over a prefix of the bench shard with one kind of shadow stage at k = 1, or none, run against the tree
ROOT (this one, or a checkout of another commit with its own library: a process per run, so that two builds can be interleaved on one box): wall time,
B/s, the stages' HIP-event ms per chunk, the submitting thread's ms, SHA-256, the kind's vote report, as one JSON line (profiles/r21_pipeline_shadow_kinds.txt).
Usage: gpu_shadow_kinds_measure.py ROOT SIZE KIND, KIND = none | shadow | ctx_shadow | lstm_shadow | fxcm_shadow; e.g. . 1048576 lstm_shadow"""
import hashlib
import json
import sys
import time

root, size, kind = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path.insert(0, root)
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402

stream = text_file_stream(synth.enwik_like(size, 1000, rich=True))
kw = {} if kind == "none" else {kind: 1}
eng = EngineStream(0, stream, 4096, **kw)
try:
    eng.pipe.stage_totals(reset=True)
    t0 = time.perf_counter()
    eng.feed(len(stream))
    blob = eng.finish()
    wall = time.perf_counter() - t0
    st = eng.pipe.stage_totals()
    host = eng.pipe.host_ms()
    fx = eng.pipe.fxcm_total_ms() / max(st["chunks"], 1)
    rep = getattr(eng.pipe, kind + "_report")()["raw"] if kw else None
finally:
    eng.close()
print(json.dumps({"root": root, "kind": kind, "bytes": len(stream), "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1),
                  "mixnet_ms": round(st["mixnet"], 3), "lstm_ms": round(st["lstm"], 3), "ctx_ms": round(st["ctxmodels"], 3), "fxcm_ms": round(fx, 3),
                  "chunks": st["chunks"], "host_ms": {k: round(v, 2) for k, v in host.items()} if isinstance(host, dict) else [round(v, 2) for v in host],
                  "sha256": hashlib.sha256(blob).hexdigest()[:16], "vote": rep}))
