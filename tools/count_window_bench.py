#!/usr/bin/env python
"""Count-window throughput on one GPU: countWindow(250, 150).sum(LONG), device-resident pushes.

Three streams of --rows rows per push (default 2^22): 10^6 uniform keys, Zipf(1.1) over 10^6 keys,
and one hot key (the path's known worst case: a key's rows are folded by one workgroup).  Each push
is one step; the steps are timed with events around them on the pushing stream, which the handle's
stream is ordered with.  Prints one JSON line per stream.

    python tools/count_window_bench.py [--rows N] [--warmup 5] [--steps 20] [--streams uniform,zipf,hot]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _keys(kind, n_keys, rows, pushes, device):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(1234)
    if kind == "hot":
        return [torch.full((rows,), 42, dtype=torch.int64, device=device)] * pushes
    if kind == "uniform":
        return [torch.randint(0, n_keys, (rows,), generator=g, device=device, dtype=torch.int64) for _ in range(pushes)]
    w = torch.arange(1, n_keys + 1, device=device, dtype=torch.float64).pow(-1.1)
    cdf = torch.cumsum(w / w.sum(), 0)
    return [torch.searchsorted(cdf, torch.rand(rows, generator=g, device=device, dtype=torch.float64)).clamp_(max=n_keys - 1)
            for _ in range(pushes)]


def run(kind, rows, warmup, steps, n_keys=10**6):
    import torch
    from flink_amd.datastream import CountWindowOperator
    dev = torch.device("cuda", 0)
    if kind == "hot":  # a step of the hot key takes far longer than the others: fewer of them
        warmup, steps = min(warmup, 1), min(steps, 3)
    op = CountWindowOperator(250, 150, ("sum", "LONG"), state_capacity=1 << 20, max_batch_rows=rows,
                             output_capacity=1 << 20).open()
    try:
        keys = _keys(kind, n_keys, rows, min(warmup + steps, 8), dev)
        vals = torch.randint(1, 10**6, (rows,), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for s in range(warmup + steps):
            t = s - warmup
            if t >= 0:
                ev[t][0].record()
            op.process_batch_device(keys[s % len(keys)], vals)
            op.handle.reset_results()  # the rows count as consumed (stream-ordered)
            if t >= 0:
                ev[t][1].record()
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        st = op.handle.stats()
        return {"tool": "count_window_bench", "stream": kind, "window": "countWindow(250,150).sum LONG", "rows_per_push": rows,
                "keys": 1 if kind == "hot" else n_keys, "warmup": warmup, "steps": steps,
                "ms_per_push_median": round(float(np.median(ms)), 4), "ms_per_push_min": round(float(ms.min()), 4),
                "events_per_s": round(rows / (float(np.median(ms)) * 1e-3)), "fired_windows": st["num_fired_windows"],
                "live_keys": st["live_state_entries"], "superbuckets": st["num_superbuckets"], "error_flags": st["error_flags"]}
    finally:
        op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--streams", default="uniform,zipf,hot")
    a = ap.parse_args()
    for kind in a.streams.split(","):
        print(json.dumps(run(kind, a.rows, a.warmup, a.steps)), flush=True)


if __name__ == "__main__":
    main()
