#!/usr/bin/env python
"""Session-window throughput on one GPU: EventTimeSessionWindows.withGap(3 s).sum(LONG),
device-resident pushes, a watermark after every push.

Three streams of --rows rows per push (default 2^22): 10^6 uniform keys, Zipf(1.1) over 10^6 keys,
and one hot key (the path's known worst case: a key's rows are folded by one workgroup, tile after
tile).  Push s carries event times in [10 s * s, 10 s * (s + 1)) and is followed by the watermark
10 s * (s + 1) - 1, so no element is late and sessions of earlier pushes fire.  A step is the push,
the advance and the (stream-ordered) result reset; it is timed on the host around a handle sync.
Prints one JSON line per stream.

    python tools/session_window_bench.py [--rows N] [--warmup 5] [--steps 20] [--streams uniform,zipf,hot]
                                         [--sql AGGS | --dynamic-gap | --lateness MS [--late-share F] |
                                          --dynamic-gap --lateness MS [--late-share F]]

--sql AGGS runs the same streams through a SQL session handle (the SESSION window TVF aggregate,
BINROW_BIGINT keys) instead: AGGS is a comma-separated aggregate list over two value columns, a
NOT NULL BIGINT ``a`` and a NULL-able DOUBLE ``b`` (a tenth of its rows are NULL), out of
COUNT(*), COUNT(b), SUM(a), MIN(a), MAX(a), AVG(a), SUM(b), AVG(b); the line then also reports the
accumulator words of the plan.  SUM(a) plans one word, SUM(a),COUNT(*) two,
SUM(a),COUNT(*),MIN(a),MAX(a) four and SUM(a),MIN(a),MAX(a),COUNT(*),AVG(b),SUM(b),COUNT(b) six,
which the eight-word kernels carry.

--dynamic-gap runs every stream three times in turn, twice over: through the static handle, through
a dynamic-gap handle (EventTimeSessionWindows.withDynamicGap, max gap 3 s) whose gap column is the
constant 3 s, and through one whose gaps are drawn from 0.5 / 1 / 2 / 3 s.  The dynamic fold reads
8 B more per event (the gap column); the lines carry "gaps": "static" / "constant" / "mixed".

--lateness MS runs the streams through a handle with that allowed lateness (FW_WIN_SESSION_LATENESS;
0 is allowed) and makes a share --late-share (default 1/6) of every push's rows late candidates:
their event times lie 3 to 8 s behind the push's span, behind the watermark of the push before.  A
candidate's key run leaves the parallel path for the arrival-order walk of one lane; with a lateness
that reaches back (10 s: every candidate is kept) most of them fire a retained session again, with
0 the ones that touch no open session are dropped.  The lines carry "lateness_ms", "late_share" and
the rows dropped.

--dynamic-gap --lateness MS runs the constant-gap and the mixed-gap dynamic handles with that allowed
lateness (FW_WIN_SESSION_DYNAMIC_LATENESS) and the same late candidates, once each.  A candidate is
placed by the 3 s gap; a mixed-gap row with a shorter gap that lies behind the watermark by its own
gap is a candidate too.  The lines carry "kind", "gaps", "lateness_ms", "late_share" and the rows
dropped.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAP_MS = 3000
SPAN_MS = 10_000
MIXED_GAPS_MS = (500, 1000, 2000, 3000)


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


_SQL_AGGS = {"COUNT(*)": ("COUNT_STAR", 0, "BIGINT"), "COUNT(b)": ("COUNT", 1, "DOUBLE"), "SUM(a)": ("SUM", 0, "BIGINT"),
             "MIN(a)": ("MIN", 0, "BIGINT"), "MAX(a)": ("MAX", 0, "BIGINT"), "AVG(a)": ("AVG", 0, "BIGINT"),
             "SUM(b)": ("SUM", 1, "DOUBLE"), "AVG(b)": ("AVG", 1, "DOUBLE")}


def run(kind, rows, warmup, steps, n_keys=10**6, sql=None, gaps=None, lateness=None, late_share=0.0):
    """``gaps``: None = the static handle; "constant" / "mixed" = a dynamic-gap handle;
    ``lateness``: not None = a handle with that allowed lateness and ``late_share`` late candidates"""
    import torch
    from flink_amd import abi
    from flink_amd.datastream import (DynamicSessionWindowOperator, LateDynamicSessionWindowOperator, LateSessionWindowOperator,
                                      SessionWindowOperator)
    from flink_amd.table import SessionWindowAggOperator
    dev = torch.device("cuda", 0)
    if kind == "hot":  # a step of the hot key takes far longer than the others: fewer of them
        warmup, steps = min(warmup, 1), min(steps, 3)
    if sql:
        op = SessionWindowAggOperator(GAP_MS, [_SQL_AGGS[a] for a in sql.split(",")], ["BIGINT", "DOUBLE"], nullable_cols=(1,),
                                      state_capacity=1 << 21, max_batch_rows=rows, output_capacity=1 << 22).open()
    elif gaps and lateness is not None:
        # (shorter gaps merge less: the mixed stream holds more sessions over the lateness than the static handle's list takes)
        op = LateDynamicSessionWindowOperator(GAP_MS, lateness, ("sum", "LONG"), state_capacity=1 << 22, max_batch_rows=rows,
                                              output_capacity=1 << 23).open()
    elif gaps:
        op = DynamicSessionWindowOperator(GAP_MS, ("sum", "LONG"), state_capacity=1 << 21, max_batch_rows=rows,
                                          output_capacity=1 << 22).open()
    elif lateness is not None:
        op = LateSessionWindowOperator(GAP_MS, lateness, ("sum", "LONG"), state_capacity=1 << 21, max_batch_rows=rows,
                                       output_capacity=1 << 23).open()
    else:
        op = SessionWindowOperator(GAP_MS, ("sum", "LONG"), state_capacity=1 << 21, max_batch_rows=rows,
                                   output_capacity=1 << 22).open()
    try:
        keys = _keys(kind, n_keys, rows, min(warmup + steps, 8), dev)
        vals = torch.randint(1, 10**6, (rows,), device=dev, dtype=torch.int64)
        if sql:
            g = torch.Generator(device=dev)
            g.manual_seed(99)
            dbl = torch.rand(rows, generator=g, device=dev, dtype=torch.float64) + 0.5
            isnull = (torch.rand(rows, generator=g, device=dev) < 0.1).to(torch.uint8)
        if gaps == "constant":
            gcol = torch.full((rows,), GAP_MS, dtype=torch.int64, device=dev)
        elif gaps == "mixed":
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            gcol = torch.tensor(MIXED_GAPS_MS, dtype=torch.int64, device=dev)[
                torch.randint(0, len(MIXED_GAPS_MS), (rows,), generator=g, device=dev)]
        offs = torch.randint(0, SPAN_MS, (rows,), device=dev, dtype=torch.int64)
        if lateness is not None and late_share > 0:  # late candidates: 3 to 8 s behind the push's span
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            back = torch.rand(rows, generator=g, device=dev) < late_share
            offs = torch.where(back, -GAP_MS - offs % 5000, offs)
        torch.cuda.synchronize()
        ms = []
        for s in range(warmup + steps):
            ts = offs + s * SPAN_MS
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if sql:
                op.process_batch_device(keys[s % len(keys)], ts, [vals, dbl], None, nulls={1: isnull})
            elif gaps:
                op.process_batch_device(keys[s % len(keys)], ts, vals, gcol)
            else:
                op.process_batch_device(keys[s % len(keys)], ts, vals)
            op.handle.advance((s + 1) * SPAN_MS - 1)
            op.handle.reset_results()  # the rows count as consumed (stream-ordered)
            op.handle.sync()
            if s >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        ms = np.array(ms)
        st = op.handle.stats()
        window = "EventTimeSessionWindows.withGap(3s).sum LONG"
        extra = {}
        if sql:
            window = "SQL SESSION(gap 3s) " + sql
            extra = {"accumulator_words": abi.host_sql_session_words(op.cfg)}
        elif gaps and lateness is not None:
            window = "EventTimeSessionWindows.withDynamicGap(<= 3s).allowedLateness.sum LONG"
            extra = {"kind": "FW_WIN_SESSION_DYNAMIC_LATENESS", "gaps": gaps, "lateness_ms": lateness, "late_share": round(late_share, 4)}
        elif gaps:
            window = "EventTimeSessionWindows.withDynamicGap(<= 3s).sum LONG"
            extra = {"gaps": gaps}
        elif lateness is not None:
            window = "EventTimeSessionWindows.withGap(3s).allowedLateness.sum LONG"
            extra = {"lateness_ms": lateness, "late_share": round(late_share, 4)}
        return {"tool": "session_window_bench", "stream": kind, "window": window, **extra,
                "rows_per_push": rows, "keys": 1 if kind == "hot" else n_keys, "warmup": warmup, "steps": steps,
                "ms_per_push_median": round(float(np.median(ms)), 4), "ms_per_push_min": round(float(ms.min()), 4),
                "events_per_s": round(rows / (float(np.median(ms)) * 1e-3)), "fired_windows": st["num_fired_windows"],
                "live_sessions": st["live_state_entries"], "late_dropped": st["num_late_records_dropped"],
                "superbuckets": st["num_superbuckets"], "error_flags": st["error_flags"]}
    finally:
        op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--streams", default="uniform,zipf,hot")
    ap.add_argument("--sql", default=None, metavar="AGGS", help="run a SQL session handle with this aggregate list")
    ap.add_argument("--dynamic-gap", action="store_true", help="static, constant-gap dynamic and mixed-gap dynamic handles in turn")
    ap.add_argument("--lateness", type=int, default=None, metavar="MS", help="run a handle with this allowed lateness")
    ap.add_argument("--late-share", type=float, default=1.0 / 6, help="with --lateness: the share of late candidates per push")
    a = ap.parse_args()
    if a.sql and a.dynamic_gap:
        ap.error("--dynamic-gap is a DataStream run (no --sql)")
    if a.lateness is not None and a.sql:
        ap.error("--lateness is a DataStream run (no --sql)")
    if a.sql and any(x not in _SQL_AGGS for x in a.sql.split(",")):
        ap.error("--sql takes a comma-separated list out of " + ", ".join(_SQL_AGGS))
    for kind in a.streams.split(","):
        if not a.dynamic_gap:
            print(json.dumps(run(kind, a.rows, a.warmup, a.steps, sql=a.sql, lateness=a.lateness, late_share=a.late_share)), flush=True)
            continue
        if a.lateness is not None:      # the dynamic-gap handles with a lateness: constant, mixed
            for gaps in ("constant", "mixed"):
                print(json.dumps(run(kind, a.rows, a.warmup, a.steps, gaps=gaps, lateness=a.lateness, late_share=a.late_share)), flush=True)
            continue
        for _ in range(2):      # alternating: static, constant, mixed, twice
            for gaps in (None, "constant", "mixed"):
                r = run(kind, a.rows, a.warmup, a.steps, gaps=gaps)
                r.setdefault("gaps", "static")
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
