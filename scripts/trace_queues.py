#!/usr/bin/env python3
"""Which hardware queue each stage kernel ran on, and whether the stages overlapped, from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python bench.py --steps 4
    python scripts/trace_queues.py DIR/t_kernel_trace.csv

Per stage kernel: launches, the Queue_Id values it ran on, total time. Overall: the distinct queues of the stage kernels, and over the span
from the first to the last stage kernel the mean number of stage kernels running at once (sum of durations / span) and the maximum."""
import csv
import sys
from collections import defaultdict

STAGES = ("cmx_mixnet_spec", "cmx_fxcm_roles", "cmx_p8s_", "cmx_lstm_", "cmx_ctxmodels_kernel", "cmx_bytemodel")


def main(path):
    per = defaultdict(lambda: [0, set(), 0])   # name -> launches, queue ids, ns
    iv = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            if not name.startswith(STAGES):
                continue
            t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            e = per[name]
            e[0] += 1
            e[1].add(int(r["Queue_Id"]))
            e[2] += t1 - t0
            iv.append((t0, t1))
    print(f"{'kernel':28s} {'launches':>8s} {'ms':>9s}  queue ids")
    for name, (n, qs, ns) in sorted(per.items(), key=lambda kv: -kv[1][2]):
        print(f"{name:28s} {n:8d} {ns / 1e6:9.1f}  {sorted(qs)}")
    queues = set().union(*(e[1] for e in per.values())) if per else set()
    print(f"distinct queues of the stage kernels: {len(queues)} {sorted(queues)}")
    if iv:
        span = max(t for _, t in iv) - min(t for t, _ in iv)
        ev = sorted([(t0, 1) for t0, _ in iv] + [(t1, -1) for _, t1 in iv])
        run = peak = 0
        for _, d in ev:
            run += d
            peak = max(peak, run)
        print(f"stage kernels running at once over {span / 1e9:.2f} s: mean {sum(t1 - t0 for t0, t1 in iv) / span:.2f}, max {peak}")


if __name__ == "__main__":
    main(sys.argv[1])
