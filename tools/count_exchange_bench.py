#!/usr/bin/env python
"""The count-window push behind the N > 1 keyBy exchange on one GPU, beside the direct push of the
same rows on the same build: countWindow(250, 150).sum(LONG) (BASELINE's CFG1 window), the settings
of tools/count_window_bench.py (10^6 uniform keys, and Zipf(1.1) over 10^6 keys; device-resident rows).

The handle is subtask 0 of parallelism 2 and the streams hold only keys of its key groups.  A step
is --rows live rows (default 2^22) in --segs segments (default 8) of the exchange's segment capacity
(KeyByExchange.segment_capacity: the even share plus 25 % headroom), the padding behind each
segment's live rows filled with keys of the other subtask.

    segments   fw_push_device_count_packed_segments over the padded packed buffer (24 B per row)
    direct     fw_push_device over the same live rows in the same order, compacted beforehand into
               columns (16 B per row): the reference

Both run in one process on two handles, alternating step by step; each step is timed with events
around it on the pushing stream, which the handle's stream is ordered with.  Prints one JSON line
per stream.  --only segments|direct runs one of them alone: under a kernel trace that run splits a
step into the partition (the k_fd_* kernels) and the fold (k_cw_fold).  Recorded, not gated.

    python tools/count_exchange_bench.py [--rows N] [--segs 8] [--warmup 5] [--steps 20]
                                         [--streams uniform,zipf] [--only segments|direct]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_P = 128
ROW_WORDS = 3


def _split_keys(n_keys):
    """(keys of subtask 0's key groups, keys of subtask 1's) out of [0, n_keys), ascending"""
    from flink_amd import _native, abi
    k = np.arange(n_keys, dtype=np.int64)
    dest = np.empty(n_keys, dtype=np.int32)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, n_keys, abi.KEYHASH_LONG, MAX_P, 2, None,
                                                          dest.ctypes.data))
    return k[dest == 0], k[dest == 1]


def _live_keys(kind, pool, rows, pushes, device):
    """per push: rows keys drawn from the pool (the owned keys, ascending: rank r of the Zipf law is pool[r])"""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(1234)
    n = pool.numel()
    if kind == "uniform":
        return [pool[torch.randint(0, n, (rows,), generator=g, device=device)] for _ in range(pushes)]
    w = torch.arange(1, n + 1, device=device, dtype=torch.float64).pow(-1.1)
    cdf = torch.cumsum(w / w.sum(), 0)
    return [pool[torch.searchsorted(cdf, torch.rand(rows, generator=g, device=device, dtype=torch.float64)).clamp_(max=n - 1)]
            for _ in range(pushes)]


def run(kind, rows, n_segs, warmup, steps, only, n_keys=10**6):
    import torch
    from flink_amd.datastream import CountWindowOperator
    from flink_amd.runtime.exchange import KeyByExchange
    dev = torch.device("cuda", 0)
    per = rows // n_segs
    rows = per * n_segs
    seg_len = KeyByExchange.segment_capacity(rows, n_segs)
    modes = [m for m in ("direct", "segments") if only in (None, m)]
    ops = {m: CountWindowOperator(250, 150, ("sum", "LONG"), max_parallelism=MAX_P, parallelism=2, subtask_index=0,
                                  state_capacity=1 << 20, max_batch_rows=n_segs * seg_len, output_capacity=1 << 20).open()
           for m in modes}
    try:
        own, foreign = (torch.from_numpy(x).to(dev) for x in _split_keys(n_keys))
        n_bufs = min(warmup + steps, 4)
        live = _live_keys(kind, own, rows, n_bufs, dev)
        vals = torch.randint(1, 10**6, (rows,), device=dev, dtype=torch.int64)
        counts = torch.full((n_segs,), per, dtype=torch.int64, device=dev)
        padded = []
        if "segments" in modes:
            for k in live:  # segment s: its share of the live rows in order, then padding of foreign keys
                buf = torch.empty((n_segs, seg_len, ROW_WORDS), dtype=torch.int64, device=dev)
                buf[:, :, 0] = foreign[torch.randint(0, foreign.numel(), (n_segs, seg_len), device=dev)]
                buf[:, :, 1] = 0
                buf[:, :, 2] = 7
                buf[:, :per, 0] = k.view(n_segs, per)
                buf[:, :per, 2] = vals.view(n_segs, per)
                padded.append(buf.reshape(-1))
        torch.cuda.synchronize()
        ev = {m: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for m in modes}
        for s in range(warmup + steps):
            t = s - warmup
            for m in modes:
                op = ops[m]
                if t >= 0:
                    ev[m][t][0].record()
                if m == "direct":
                    op.process_batch_device(live[s % n_bufs], vals)
                else:
                    op.process_packed_segments_device(counts, padded[s % n_bufs], ROW_WORDS)
                op.handle.reset_results()  # the rows count as consumed (stream-ordered)
                if t >= 0:
                    ev[m][t][1].record()
        torch.cuda.synchronize()
        out = {"tool": "count_exchange_bench", "stream": kind, "window": "countWindow(250,150).sum LONG", "live_rows_per_step": rows,
               "segments": n_segs, "segment_rows": seg_len, "buffer_rows": n_segs * seg_len, "keys": int(own.numel()),
               "warmup": warmup, "steps": steps}
        for m in modes:
            ms = np.array([a.elapsed_time(b) for a, b in ev[m]])
            st = ops[m].handle.stats()
            out[m] = {"ms_per_step_median": round(float(np.median(ms)), 4), "ms_per_step_min": round(float(ms.min()), 4),
                      "ms_per_step_max": round(float(ms.max()), 4), "events_per_s": round(rows / (float(np.median(ms)) * 1e-3)),
                      "fired_windows": st["num_fired_windows"], "live_keys": st["live_state_entries"],
                      "error_flags": st["error_flags"]}
        if len(modes) == 2:
            out["same_fires"] = out["direct"]["fired_windows"] == out["segments"]["fired_windows"]
            out["segments_over_direct"] = round(out["segments"]["ms_per_step_median"] / out["direct"]["ms_per_step_median"], 4)
        return out
    finally:
        for op in ops.values():
            op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--segs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--streams", default="uniform,zipf")
    ap.add_argument("--only", choices=("segments", "direct"), default=None)
    a = ap.parse_args()
    for kind in a.streams.split(","):
        print(json.dumps(run(kind, a.rows, a.segs, a.warmup, a.steps, a.only)), flush=True)


if __name__ == "__main__":
    main()
