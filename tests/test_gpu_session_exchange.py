"""Session windows behind the N > 1 keyBy exchange, one process: hand-built padded receive buffers
pushed through fw_push_device_segments / fw_push_device_packed_segments into a handle of
parallelism 2, and the watermark of record on the device (fw_advance_device).

Shapes are the smallest that reach every edge.  A partition chunk and a fold tile hold 1024 rows and
max_batch_rows is 2048, so a buffer of 3 segments of 1500 rows is three launches, with segments that
straddle launches and tiles; the count vectors leave a segment empty, full, one row long and over
full (clamped: the overflow went to the spill); the spill-shaped pushes are one segment of 37 and of
1024 rows.  Every padding row is poison -- a key of the OTHER subtask's key groups,
ts = Long.MIN_VALUE + 1, a dynamic gap of 0 -- so reading one would raise FW_ERRF_KEYGROUP or
FW_ERRF_GAP or open a session nobody pushed.

Each case drives a twin handle with the same live rows, compacted, through fw_push_device and the same
watermarks, and the kind's reference (session_window_reference.py, dynamic_session_reference.py,
sql_session_reference.py).  Everything is compared bit-exact except DOUBLE SUM / AVG, at the project's
1e-9 relative (parity_common.REL_TOL): the two handles cut their launches at different rows.  The
streams hold rows that are late when they arrive; the reference must drop some and keep some, so the
cases cannot pass where arrival order is irrelevant.
"""
import struct

import numpy as np
import pytest
from dynamic_session_reference import DynamicSessionReference
from parity_common import REL_TOL
from session_window_reference import SessionWindowReference
from sql_session_reference import SqlSessionReference

import session_exchange_order as order
from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
SEG_LEN, N_SEGS = 1500, 3
GAP = 50
MAX_P = 4
CFG = dict(max_parallelism=MAX_P, parallelism=2, subtask_index=0, state_capacity=1, max_batch_rows=2048,
           output_capacity=1 << 14)
# (segments, segment length, counts): the padded buffers of one case, a watermark after each
PUSHES = [(N_SEGS, SEG_LEN, (0, 1500, 700)), (N_SEGS, SEG_LEN, (1500, 0, 1)), (N_SEGS, SEG_LEN, (1800, 1500, 0)),
          (1, 37, (37,)), (1, 1024, (1024,))]
BASE, WM_STEP = 100_000, 400

# SQL plans by kernel instance (accumulator words): (aggs, value types, NULL-able columns)
SQL2 = ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT")], ["BIGINT"], (0,))
SQL4_NOT_NULL = ([("SUM", 0, "BIGINT"), ("MIN", 1, "INT"), ("MAX", 1, "INT"), ("COUNT_STAR", 0, "BIGINT")], ["BIGINT", "INT"], ())
SQL8 = ([("SUM", 0, "BIGINT"), ("AVG", 1, "DOUBLE"), ("MIN", 2, "INT"), ("MAX", 2, "INT"), ("COUNT", 1, "DOUBLE"),
         ("COUNT_STAR", 0, "BIGINT"), ("SUM", 1, "DOUBLE")], ["BIGINT", "DOUBLE", "INT"], (0, 1, 2))
KINDS = {
    "ds": dict(kind="ds"), "dyn": dict(kind="dyn"),
    "sql2": dict(kind="sql", layout=SQL2, nw=2), "sql4": dict(kind="sql", layout=SQL4_NOT_NULL, nw=4),
    "sql8": dict(kind="sql", layout=SQL8, nw=8),
}
CASES = [("ds", "soa"), ("ds", "packed"), ("dyn", "soa"), ("dyn", "packed"), ("sql2", "soa"), ("sql8", "soa"), ("sql4", "packed")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hash_kind(kd):
    return abi.KEYHASH_BINROW_BIGINT if kd["kind"] == "sql" else abi.KEYHASH_LONG


def _keys(kd):
    """(about 40 keys of subtask 0's key groups, keys of subtask 1's)"""
    cand = np.arange(1, 400, dtype=np.int64) * 7919 + 13
    dest = order.destinations(cand, _hash_kind(kd), MAX_P, 2)
    own, foreign = cand[dest == 0][:40], cand[dest == 1]
    assert len(own) == 40 and len(foreign) > 10
    return own, foreign


def _open(kd, **kw):
    cfg = dict(CFG)
    cfg.update(kw)
    if kd["kind"] == "ds":
        from flink_amd.datastream import SessionWindowOperator
        return SessionWindowOperator(GAP, ("sum", "LONG"), late_side_output=True, **cfg).open()
    if kd["kind"] == "dyn":
        from flink_amd.datastream import DynamicSessionWindowOperator
        return DynamicSessionWindowOperator(GAP, ("sum", "LONG"), late_side_output=True, **cfg).open()
    from flink_amd.table import SessionWindowAggOperator
    aggs, types, nullable = kd["layout"]
    return SessionWindowAggOperator(GAP, aggs, types, nullable_cols=nullable, **cfg).open()


def _reference(kd):
    if kd["kind"] == "ds":
        return SessionWindowReference(GAP, ("sum", "LONG"))
    if kd["kind"] == "dyn":
        return DynamicSessionReference(("sum", "LONG"))
    return SqlSessionReference(GAP, kd["layout"][0])


def _value_cols(kd, rng, n):
    """(value columns, {column: NULL flags}) of n random rows"""
    if kd["kind"] == "ds":
        return [rng.integers(-10**6, 10**6, n).astype(np.int64)], {}
    if kd["kind"] == "dyn":
        return [rng.integers(-10**6, 10**6, n).astype(np.int64), rng.integers(1, GAP + 1, n).astype(np.int64)], {}
    _, types, nullable = kd["layout"]
    vals, nulls = [], {}
    for c, t in enumerate(types):
        if t == "DOUBLE":
            vals.append(rng.uniform(0.5, 100.0, n))
        elif t == "INT":
            vals.append(rng.integers(-1000, 1000, n).astype(np.int64))
        else:
            vals.append(rng.integers(-10**12, 10**12, n).astype(np.int64))
        if c in nullable:
            nulls[c] = (rng.random(n) < 0.3).astype(np.uint8)
    return vals, nulls


def _live_rows(kd, rng, own, b, n):
    """Push b's n live rows: timestamps from 1200 behind the push's base to 1000 ahead, the watermark
    400 behind the base -- a third of the rows is late when it arrives."""
    k = rng.choice(own, n)
    ts = (BASE + b * WM_STEP + rng.integers(-1200, 1000, n)).astype(np.int64)
    vals, nulls = _value_cols(kd, rng, n)
    return k, ts, vals, nulls


def _padded(kd, rng, foreign, n_segs, seg_len, counts, live):
    """The padded buffer of the live rows: poison everywhere, then segment s's first min(count,
    seg_len) rows.  Returns (columns as _live_rows, the live rows' buffer positions)."""
    n = n_segs * seg_len
    k, ts, vals, nulls = live
    pk = rng.choice(foreign, n)
    pts = np.full(n, LONG_MIN + 1, dtype=np.int64)
    pvals, pnulls = _value_cols(kd, rng, n)
    if kd["kind"] == "dyn":
        pvals[1][:] = 0
    pos = np.concatenate([s * seg_len + np.arange(min(c, seg_len)) for s, c in enumerate(counts)]).astype(np.int64)
    assert len(pos) == len(k)
    pk[pos], pts[pos] = k, ts
    for c in range(len(vals)):
        pvals[c][pos] = vals[c]
    for c in nulls:
        pnulls[c][pos] = nulls[c]
    return (pk, pts, pvals, pnulls), pos


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _push_padded(op, kd, layout, counts, cols):
    k, ts, vals, nulls = cols
    sc = _dev(np.asarray(counts, dtype=np.int64))
    if layout == "packed":
        assert not nulls
        rows = np.stack([k, ts] + [v.view(np.int64) for v in vals], axis=1)
        op.process_packed_segments_device(sc, _dev(rows.reshape(-1)), rows.shape[1])
    elif kd["kind"] == "ds":
        op.process_segments_device(sc, _dev(k), _dev(ts), _dev(vals[0]))
    elif kd["kind"] == "dyn":
        op.process_segments_device(sc, _dev(k), _dev(ts), _dev(vals[0]), _dev(vals[1]))
    else:
        op.process_segments_device(sc, _dev(k), _dev(ts), [_dev(v) for v in vals], nulls={c: _dev(f) for c, f in nulls.items()})


def _push_compact(op, kd, live):
    k, ts, vals, nulls = live
    if kd["kind"] == "ds":
        op.process_batch_device(_dev(k), _dev(ts), _dev(vals[0]))
    elif kd["kind"] == "dyn":
        op.process_batch_device(_dev(k), _dev(ts), _dev(vals[0]), _dev(vals[1]))
    else:
        op.process_batch_device(_dev(k), _dev(ts), [_dev(v) for v in vals], nulls={c: _dev(f) for c, f in nulls.items()})


def _push_reference(ref, kd, live, seen):
    """The live rows into the reference; returns the dropped rows' indices and counts the late
    candidates by what became of them."""
    k, ts, vals, nulls = live
    dropped = []
    for i in range(len(k)):
        gap = int(vals[1][i]) if kd["kind"] == "dyn" else GAP
        late = int(ts[i]) + gap - 1 <= ref.watermark
        if kd["kind"] == "ds":
            kept = ref.add(int(k[i]), int(ts[i]), int(vals[0][i]))
        elif kd["kind"] == "dyn":
            kept = ref.add(int(k[i]), int(ts[i]), int(vals[0][i]), gap)
        else:
            row = [None if c in nulls and nulls[c][i] else vals[c][i].item() for c in range(len(vals))]
            kept = ref.add(int(k[i]), int(ts[i]), row)
        assert kept or late
        if late:
            seen["late_kept" if kept else "late_drop"] += 1
        if not kept:
            dropped.append(i)
    return dropped


def _fired(op, kd, res):
    if kd["kind"] == "sql":
        return op.output_rows(res)
    return [(int(k), int(v), int(s), int(e)) for k, v, s, e in zip(res["key"], res["value"], res["window_start"],
                                                                   res["window_end"])]


def _same(got, want):
    """rows as multisets: integers, bounds and NULLs exact, DOUBLE at REL_TOL"""
    def key(r):
        return (r[-1], r[0], r[-2])
    got, want = sorted(got, key=key), sorted((tuple(w) for w in want), key=key)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for x, y in zip(g, w):
            if isinstance(y, float):
                assert x is not None and x == pytest.approx(y, rel=REL_TOL, abs=0.0), (g, w)
            else:
                assert x == y, (g, w)


def _side(op):
    """the late side output since the last call in (push_seq, row) order: (key, ts, value), rows"""
    r = op.late_records()
    o = np.lexsort((r["row"], r["push_seq"]))
    return (list(zip(r["key"][o].tolist(), r["ts"][o].tolist(), r["value"][o].tolist())), r["row"][o].tolist())


def _clean(op):
    s = op.handle.stats()
    assert s["error_flags"] == 0, s["error_flags"]   # no FW_ERRF_KEYGROUP, no FW_ERRF_GAP: no padding row was read
    return s


@pytest.mark.parametrize("kind,layout", CASES)
def test_padded_push_equals_compacted_twin_and_reference(kind, layout):
    import ctypes as C
    kd = KINDS[kind]
    own, foreign = _keys(kd)
    rng = np.random.default_rng(20 + CASES.index((kind, layout)))
    op, twin, ref = _open(kd), _open(kd), _reference(kd)
    seen = {"late_kept": 0, "late_drop": 0}
    try:
        if kd["kind"] == "sql":  # the case runs the instance it names
            nw = C.c_int32()
            _native.check(_native.lib().fw_host_sql_session_words(C.byref(op.cfg), C.byref(nw)))
            assert (1 if nw.value <= 1 else 2 if nw.value <= 2 else 4 if nw.value <= 4 else 8) == kd["nw"]
        for b, (n_segs, seg_len, counts) in enumerate(PUSHES):
            n_live = sum(min(c, seg_len) for c in counts)
            live = _live_rows(kd, rng, own, b, n_live)
            cols, pos = _padded(kd, rng, foreign, n_segs, seg_len, counts, live)
            _push_padded(op, kd, layout, counts, cols)
            _push_compact(twin, kd, live)
            dropped = _push_reference(ref, kd, live, seen)
            wm = BASE + b * WM_STEP
            want = ref.process_watermark(wm)
            got, got_twin = _fired(op, kd, op.process_watermark(wm)), _fired(twin, kd, twin.process_watermark(wm))
            _same(got, want)
            _same(got, got_twin)
            s, st = _clean(op), _clean(twin)
            assert s["num_late_records_dropped"] == st["num_late_records_dropped"] == ref.late_dropped
            assert s["current_watermark"] == st["current_watermark"] == wm
            if kd["kind"] != "sql":  # the late side output; a segmented push's row is the buffer position
                want_side = [(int(live[0][i]), int(live[1][i]), int(live[2][0][i])) for i in dropped]
                side, rows = _side(op)
                side_twin, rows_twin = _side(twin)
                assert side == side_twin == want_side
                assert rows == pos[dropped].tolist() and rows_twin == dropped
        want = ref.process_watermark(LONG_MAX)
        got = _fired(op, kd, op.process_watermark(LONG_MAX))
        _same(got, want)
        _same(got, _fired(twin, kd, twin.process_watermark(LONG_MAX)))
        assert len(want) > 0 and _clean(op)["live_state_entries"] == 0
        # the order dependence was exercised: late candidates on both sides
        assert seen["late_drop"] >= 1 and seen["late_kept"] >= 1, seen
    finally:
        op.close()
        twin.close()


def test_live_foreign_row_is_dropped_and_flagged():
    kd = KINDS["ds"]
    own, foreign = _keys(kd)
    rng = np.random.default_rng(5)
    op, ref, fresh = _open(kd), _reference(kd), None
    try:
        counts = (0, 1500, 700)
        live = _live_rows(kd, rng, own, 0, 2200)
        bad = 1700   # a live row of the third segment (straddling the second launch) gets a foreign key
        live[0][bad] = foreign[0]
        cols, _ = _padded(kd, rng, foreign, N_SEGS, SEG_LEN, counts, live)
        _push_padded(op, kd, "soa", counts, cols)
        keep = np.arange(2200) != bad
        ref.process(live[0][keep].tolist(), live[1][keep].tolist(), live[2][0][keep].tolist())
        s = op.handle.stats()
        assert s["error_flags"] == abi.ERRF["KEYGROUP"]
        assert s["live_state_entries"] == ref.live_sessions() and s["num_late_records_dropped"] == 0
        # the flag is sticky and fw_results reports it, so the sessions are read through a checkpoint:
        # a restore starts with clean flags
        fresh = _open(kd)
        fresh.initialize_state(op.snapshot_state())
        _same(_fired(fresh, kd, fresh.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
        assert fresh.handle.stats()["error_flags"] == 0
    finally:
        op.close()
        if fresh is not None:
            fresh.close()


def test_device_watermark_is_the_watermark_of_record():
    import torch
    kd = KINDS["ds"]
    own, foreign = _keys(kd)
    rng = np.random.default_rng(9)
    op, twin = _open(kd), _open(kd)
    fresh = None

    def wmt(w):
        return torch.tensor([w], dtype=torch.int64, device="cuda")

    try:
        seen = {"late_kept": 0, "late_drop": 0}
        ref = _reference(kd)
        wm = LONG_MIN
        for b, (n_segs, seg_len, counts) in enumerate(PUSHES[:3]):
            live = _live_rows(kd, rng, own, b, sum(min(c, seg_len) for c in counts))
            cols, _ = _padded(kd, rng, foreign, n_segs, seg_len, counts, live)
            _push_padded(op, kd, "soa" if b % 2 == 0 else "packed", counts, cols)
            _push_padded(twin, kd, "soa" if b % 2 == 0 else "packed", counts, cols)
            _push_reference(ref, kd, live, seen)
            wm = BASE + b * WM_STEP
            got = _fired(op, kd, op.process_watermark_device(wmt(wm)))
            _same(got, _fired(twin, kd, twin.process_watermark(wm)))
            _same(got, ref.process_watermark(wm))
            assert _clean(op)["num_late_records_dropped"] == _clean(twin)["num_late_records_dropped"] == ref.late_dropped
        assert seen["late_drop"] >= 1 and seen["late_kept"] >= 1, seen
        live_before = _clean(op)["live_state_entries"]
        assert live_before > 0
        # a lower device watermark and a lower host watermark change nothing
        assert _fired(op, kd, op.process_watermark_device(wmt(wm - 300))) == []
        assert _fired(op, kd, op.process_watermark(wm - 100)) == []
        s = _clean(op)
        assert s["current_watermark"] == wm and s["live_state_entries"] == live_before
        # fw_reserve / fw_commit after the device advance: folds under the device watermark
        k0 = int(own[0])
        late_ts, ok_ts = wm - 5 * GAP - 5000, wm + 5000
        for o in (op, twin):
            o.process_batch([k0, k0], [late_ts, ok_ts], [7, 9])
        ref.process([k0, k0], [late_ts, ok_ts], [7, 9])
        assert _clean(op)["num_late_records_dropped"] == _clean(twin)["num_late_records_dropped"] == ref.late_dropped
        assert [x[:2] for x in _side(op)[0]][-1] == (k0, late_ts)
        # a higher host watermark fires: the device takes the maximum
        wm2 = wm + 350
        got = _fired(op, kd, op.process_watermark(wm2))
        _same(got, _fired(twin, kd, twin.process_watermark(wm2)))
        _same(got, ref.process_watermark(wm2))
        assert len(got) > 0 and _clean(op)["current_watermark"] == wm2
        # and a device advance above that one
        wm3 = wm2 + 350
        got = _fired(op, kd, op.process_watermark_device(wmt(wm3)))
        _same(got, ref.process_watermark(wm3))
        assert len(got) > 0 and _clean(op)["current_watermark"] == wm3
        # snapshot / restore carry the device value: the header's watermark word, and a late row after
        blob = op.snapshot_state()
        assert struct.unpack_from("<q", blob, 16)[0] == wm3
        fresh = _open(kd)
        fresh.initialize_state(blob)
        assert fresh.handle.stats()["current_watermark"] == wm3
        one = (np.array([k0]), np.array([wm3 - 5 * GAP - 5000]), [np.array([1])], {})
        _push_padded(fresh, kd, "soa", (1,), one)          # late under the restored watermark
        assert fresh.handle.stats()["num_late_records_dropped"] == 1
        _same(_fired(fresh, kd, fresh.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
    finally:
        op.close()
        twin.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("kind", ["ds", "dyn", "sql2"])
def test_parallelism_1_handle_refuses_the_exchange_calls(kind):
    import torch
    kd = KINDS[kind]
    op = _open(kd, parallelism=1)
    try:
        h = op.handle
        cnt = torch.ones(1, dtype=torch.int64, device="cuda")
        col = torch.zeros(4, dtype=torch.int64, device="cuda")
        n_vals = 2 if kind == "dyn" else 1
        for call in (lambda: h.advance_device(cnt),
                     lambda: h.push_device_segments(cnt, col[:1], col[:1], [col[:1]] * n_vals),
                     lambda: h.push_device_packed_segments(cnt, col[:2 + n_vals], 2 + n_vals)):
            with pytest.raises(_native.FlinkWinError, match="not for session windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        assert h.stats()["error_flags"] == 0
    finally:
        op.close()


def test_count_handle_of_parallelism_2_keeps_refusing_the_segment_pushes():
    import torch
    from flink_amd.datastream import CountWindowOperator
    op = CountWindowOperator(4, None, ("sum", "LONG"), max_parallelism=MAX_P, parallelism=2, subtask_index=0,
                             max_batch_rows=2048, output_capacity=1 << 12)
    op.open()
    try:
        h = op.handle
        cnt = torch.ones(1, dtype=torch.int64, device="cuda")
        col = torch.zeros(4, dtype=torch.int64, device="cuda")
        for call in (lambda: h.push_device_segments(cnt, col[:1], col[:1], [col[:1]]),
                     lambda: h.push_device_packed_segments(cnt, col[:3], 3)):
            with pytest.raises(_native.FlinkWinError, match="not for count windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
    finally:
        op.close()
