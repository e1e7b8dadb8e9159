#!/usr/bin/env python
"""Record-shaped count-window throughput on one GPU: countWindow(250, 150) sum(LONG) and minBy(LONG)
on the FW_WIN_COUNT_RECORD kind, device-resident pushes.

The streams of tools/count_window_bench.py: --rows rows per push (default 2^22) over 10^6 uniform keys,
Zipf(1.1) over 10^6 keys, and one hot key.  Each push is one step, timed with events around it on the
pushing stream, which the handle's stream is ordered with; the results are dropped and the retain /
release events read after the step's closing event, outside the timed region (a shim reads both after
every push -- the event buffer holds one push).  Prints one JSON line per aggregate and stream.

    python tools/count_record_bench.py [--rows N] [--warmup 5] [--steps 20] [--streams uniform,zipf,hot] [--aggs sum,minBy]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(agg, kind, rows, warmup, steps, n_keys=10**6):
    import torch
    from count_window_bench import _keys

    from flink_amd.datastream import RecordCountWindowOperator
    dev = torch.device("cuda", 0)
    if kind == "hot":  # a step of the hot key takes far longer than the others: fewer of them
        warmup, steps = min(warmup, 1), min(steps, 3)
    op = RecordCountWindowOperator(250, 150, (agg, "LONG"), field=1, state_capacity=1 << 20, max_batch_rows=rows,
                                   output_capacity=1 << 20).open()
    try:
        keys = _keys(kind, n_keys, rows, min(warmup + steps, 8), dev)
        vals = torch.randint(1, 10**6, (rows,), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        n_events = 0
        for s in range(warmup + steps):
            t = s - warmup
            if t >= 0:
                ev[t][0].record()
            op.handle.push_device(keys[s % len(keys)], None, [vals])
            if t >= 0:
                ev[t][1].record()
            op.handle.reset_results()  # the rows count as consumed (stream-ordered)
            retain, release = op.handle.first_element_events()
            n_events += len(retain) + len(release)
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        st = op.handle.stats()
        return {"tool": "count_record_bench", "stream": kind, "window": f"countWindow(250,150).{agg} LONG, records", "rows_per_push": rows,
                "keys": 1 if kind == "hot" else n_keys, "warmup": warmup, "steps": steps,
                "ms_per_push_median": round(float(np.median(ms)), 4), "ms_per_push_min": round(float(ms.min()), 4),
                "events_per_s": round(rows / (float(np.median(ms)) * 1e-3)), "fired_windows": st["num_fired_windows"],
                "retain_release_events": n_events, "live_keys": st["live_state_entries"], "superbuckets": st["num_superbuckets"],
                "error_flags": st["error_flags"]}
    finally:
        op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--streams", default="uniform,zipf,hot")
    ap.add_argument("--aggs", default="sum,minBy")
    a = ap.parse_args()
    for agg in a.aggs.split(","):
        for kind in a.streams.split(","):
            print(json.dumps(run(agg, kind, a.rows, a.warmup, a.steps)), flush=True)


if __name__ == "__main__":
    main()
