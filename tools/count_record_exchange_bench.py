#!/usr/bin/env python
"""The record count-window push behind the N > 1 keyBy exchange on one GPU, beside the direct record push
of the same rows on the same build: countWindow(250, 150).sum on a LONG field of four-field records
(key, field, LONG, DOUBLE), 10^6 uniform keys and Zipf(1.1) over 10^6 keys, device-resident rows.

The handle is subtask 0 of parallelism 2 and the streams hold only keys of its key groups.  A step is
--rows live rows (default 2^20) in --segs segments (default 8) of the exchange's segment capacity, the
padding behind each segment's live rows filled with keys of the other subtask.

    segments   fw_push_device_count_record_packed_segments over the padded packed buffer (48 B per row),
               then fw_count_record_rows (the gather kernel, the one host wait, the events and the
               gathered words to the host) and fw_results
    direct     fw_push_device over the same live rows in the same order, compacted beforehand into
               columns (16 B per row), then fw_results and fw_first_element_events: what the direct shim
               reads per push, without its Python record handling

Both run in one process on two handles, alternating step by step.  A step ends with a host wait on both
sides, so it is timed on the host (perf_counter, the device idle at its start); the push alone is also
timed with events.  --only segments|direct runs one of them alone: under a kernel trace that run gives
k_cw_gather_rec's share of a step.  Prints one JSON line per stream.  Recorded, not gated.

    python tools/count_record_exchange_bench.py [--rows N] [--segs 8] [--warmup 3] [--steps 10]
                                                [--streams uniform,zipf] [--only segments|direct]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAX_P = 128
TYPES = ["LONG", "LONG", "LONG", "DOUBLE"]
ROW_WORDS = 2 + len(TYPES)


def run(kind, rows, n_segs, warmup, steps, only, n_keys=10**6):
    import torch
    from count_exchange_bench import _live_keys, _split_keys

    from flink_amd.datastream import RecordCountWindowOperator
    from flink_amd.runtime.exchange import KeyByExchange
    dev = torch.device("cuda", 0)
    per = rows // n_segs
    rows = per * n_segs
    seg_len = KeyByExchange.segment_capacity(rows, n_segs)
    modes = [m for m in ("direct", "segments") if only in (None, m)]
    ops = {m: RecordCountWindowOperator(250, 150, ("sum", "LONG"), field=1, record_types=TYPES if m == "segments" else None,
                                        max_parallelism=MAX_P, parallelism=2, subtask_index=0, state_capacity=1 << 20,
                                        max_batch_rows=n_segs * seg_len, output_capacity=1 << 20).open() for m in modes}
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
                buf[:, :, 1:] = 7
                buf[:, :per, 0] = k.view(n_segs, per)
                buf[:, :per, 2] = k.view(n_segs, per)
                buf[:, :per, 3] = vals.view(n_segs, per)
                buf[:, :per, 4] = torch.arange(rows, device=dev).view(n_segs, per)
                padded.append(buf.reshape(-1))
        torch.cuda.synchronize()
        ev = {m: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for m in modes}
        wall = {m: [] for m in modes}
        n_ev = {m: 0 for m in modes}
        n_words = 0
        for s in range(warmup + steps):
            t = s - warmup
            for m in modes:
                h = ops[m].handle
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if t >= 0:
                    ev[m][t][0].record()
                if m == "direct":
                    h.push_device(live[s % n_bufs], None, [vals])
                else:
                    h.push_device_count_record_packed_segments(counts, padded[s % n_bufs], ROW_WORDS)
                if t >= 0:
                    ev[m][t][1].record()
                if m == "direct":
                    h.results(reset=True)
                    retain, release = h.first_element_events()
                    n = len(retain) + len(release)
                else:
                    g = h.count_record_rows(padded[s % n_bufs], ROW_WORDS)
                    h.results(reset=True)
                    n = len(g["ev_ord"])
                    if t >= 0:
                        n_words += int(g["ev_is_retain"].sum() + g["res_from_push"].sum()) * len(TYPES)
                if t >= 0:
                    wall[m].append((time.perf_counter() - t0) * 1e3)
                    n_ev[m] += n
        torch.cuda.synchronize()
        out = {"tool": "count_record_exchange_bench", "stream": kind, "window": "countWindow(250,150).sum LONG, 4-field records",
               "live_rows_per_step": rows, "segments": n_segs, "segment_rows": seg_len, "buffer_rows": n_segs * seg_len,
               "keys": int(own.numel()), "warmup": warmup, "steps": steps}
        for m in modes:
            push = np.array([a.elapsed_time(b) for a, b in ev[m]])
            w = np.array(wall[m])
            st = ops[m].handle.stats()
            out[m] = {"ms_per_step_median": round(float(np.median(w)), 4), "ms_per_step_min": round(float(w.min()), 4),
                      "ms_per_step_max": round(float(w.max()), 4), "push_ms_median": round(float(np.median(push)), 4),
                      "events_per_s": round(rows / (float(np.median(w)) * 1e-3)), "retain_release_events_per_step": n_ev[m] // steps,
                      "fired_windows": st["num_fired_windows"], "live_keys": st["live_state_entries"], "error_flags": st["error_flags"]}
        if "segments" in modes:
            out["segments"]["gathered_bytes_per_step"] = n_words * 8 // steps
        if len(modes) == 2:
            out["same_fires"] = out["direct"]["fired_windows"] == out["segments"]["fired_windows"]
            out["segments_over_direct"] = round(out["segments"]["ms_per_step_median"] / out["direct"]["ms_per_step_median"], 4)
        return out
    finally:
        for op in ops.values():
            op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--segs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--streams", default="uniform,zipf")
    ap.add_argument("--only", choices=("segments", "direct"), default=None)
    a = ap.parse_args()
    for kind in a.streams.split(","):
        print(json.dumps(run(kind, a.rows, a.segs, a.warmup, a.steps, a.only)), flush=True)


if __name__ == "__main__":
    main()
