#!/usr/bin/env python
"""The session step behind the N > 1 keyBy exchange on one GPU, beside the direct step of the same
build on the same stream: EventTimeSessionWindows.withGap(3 s).sum(LONG), the settings of
tools/session_window_bench.py (uniform keys out of 10^6, event times of push s in
[10 s * s, 10 s * (s + 1)), the watermark 10 s * (s + 1) - 1 behind it, device-resident rows).

The handle is subtask 0 of parallelism 2 and the stream holds only keys of its key groups.

    --mode direct     push_device + advance, the step session_window_bench times
    --mode exchange   one rank over the nccl backend (RCCL) with force_collectives: the packed
                      partition, the all-to-all, fw_push_device_packed_segments, the device valve's
                      all-reduce and fw_advance_device (SessionExchangeStep.step_device_valve, rows
                      not collected)

A step is timed on the host around a handle sync.  Prints one JSON line.  Recorded, not gated.
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAP_MS = 3000
SPAN_MS = 10_000
MAX_P = 128


def _own_keys(n_keys):
    from flink_amd import _native, abi
    k = np.arange(n_keys, dtype=np.int64)
    dest = np.empty(n_keys, dtype=np.int32)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, n_keys, abi.KEYHASH_LONG, MAX_P, 2, None,
                                                          dest.ctypes.data))
    return k[dest == 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("direct", "exchange"), default="exchange")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from flink_amd import abi
    from flink_amd.datastream import SessionWindowOperator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = a.rows
    op = SessionWindowOperator(GAP_MS, ("sum", "LONG"), max_parallelism=MAX_P, parallelism=2, subtask_index=0,
                               state_capacity=1 << 21, max_batch_rows=2 * rows, output_capacity=1 << 22).open()
    drv = None
    if a.mode == "exchange":
        import torch.distributed as dist
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        from flink_amd.datastream import SessionExchangeStep
        from flink_amd.runtime.exchange import KeyByExchange
        drv = SessionExchangeStep(op, KeyByExchange(abi.KEYHASH_LONG, MAX_P, force_collectives=True), dev)
    try:
        pool = torch.from_numpy(_own_keys(10**6)).to(dev)
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        keys = [pool[torch.randint(0, pool.numel(), (rows,), generator=g, device=dev)] for _ in range(8)]
        vals = torch.randint(1, 10**6, (rows,), generator=g, device=dev, dtype=torch.int64)
        offs = torch.randint(0, SPAN_MS, (rows,), generator=g, device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        ms = []
        for s in range(a.warmup + a.steps):
            ts = offs + s * SPAN_MS
            wm = (s + 1) * SPAN_MS - 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if drv is None:
                op.process_batch_device(keys[s % 8], ts, vals)
                op.handle.advance(wm)
            else:
                drv.step_device_valve(keys[s % 8], ts, [vals], wm, collect=False)
            op.handle.reset_results()  # the rows count as consumed (stream-ordered)
            op.handle.sync()
            if s >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        if drv is not None:
            drv.settle(collect=False)
        ms = np.array(ms)
        st = op.handle.stats()
        out = {"tool": "session_exchange_bench", "mode": a.mode, "window": "EventTimeSessionWindows.withGap(3s).sum LONG",
               "rows_per_step": rows, "keys": int(pool.numel()), "warmup": a.warmup, "steps": a.steps,
               "ms_per_step_median": round(float(np.median(ms)), 4), "ms_per_step_min": round(float(ms.min()), 4),
               "events_per_s": round(rows / (float(np.median(ms)) * 1e-3)), "fired_windows": st["num_fired_windows"],
               "live_sessions": st["live_state_entries"], "late_dropped": st["num_late_records_dropped"],
               "current_watermark": st["current_watermark"], "error_flags": st["error_flags"]}
        if drv is not None:
            out["spill_rounds"] = drv.exchange.spill_rounds
        print(json.dumps(out), flush=True)
    finally:
        op.close()
        if a.mode == "exchange":
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
