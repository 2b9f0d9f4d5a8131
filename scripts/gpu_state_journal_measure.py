"""The state journal off / on through the whole engine (EngineStream) on a shard prefix, one run per call so that a shell loop can interleave the
settings with the parent commit's tree (which runs scripts/gpu_journal_measure.py SIZE 0 1: the same stream with no switch): wall time, B/s, the
stages' HIP-event time per chunk, the file's SHA-256 (must not change), the number of records and a SHA-256 over the state journal's words (must not
change from run to run) (profiles/r21_state_journal.txt).
Usage: gpu_state_journal_measure.py SIZE EVERY [OUT.state]     EVERY: chunks of 4096 bytes per record, 0 = the switch off"""
import hashlib
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cmix_amd import journal as J  # noqa: E402
from cmix_amd import synth  # noqa: E402
from cmix_amd.pipeline import EngineStream, text_file_stream  # noqa: E402


def one(n, every, out=None):
    stream = text_file_stream(synth.enwik_like(n, 1000, rich=True))
    eng = EngineStream(0, stream, 4096, state_journal=every) if every else EngineStream(0, stream, 4096)
    try:
        eng.pipe.stage_totals(reset=True)
        t0 = time.perf_counter()
        eng.feed(len(stream))
        blob = eng.finish()
        sj = eng.state_journal() if every else None
        wall = time.perf_counter() - t0
        st = eng.pipe.stage_totals()
    finally:
        eng.close()
    r = {"bytes": len(stream), "state_journal_every": every, "wall_s": round(wall, 3), "bytes_per_s": round(len(stream) / wall, 1), "mixnet_ms_per_chunk": round(st["mixnet"], 3),
         "chunks": st["chunks"], "size": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}
    if sj is not None:
        lay, pos, words = sj
        r["records"], r["columns"] = len(pos), len(lay)
        r["columns_per_stage"] = {J.STATE_STAGES[i]: int((lay[:, 0] == i).sum()) for i in range(len(J.STATE_STAGES))}
        r["state_mb"] = round(4 * int(lay[:, 3].sum()) / 1e6, 1)
        r["state_journal_sha256"] = hashlib.sha256(np.ascontiguousarray(pos).tobytes() + np.ascontiguousarray(words).tobytes()).hexdigest()
        if out:
            J.write_state(out, lay, pos, words)
    return r


if __name__ == "__main__":
    print(json.dumps(one(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)), flush=True)
