"""Every delivery path of one handle returns the same rows: fw_results with a host copy, fw_results
with device pointers (read back here), fw_results_async + fw_results_ready (kernel stores and DMA),
fw_results_device and fw_results_device_segments.  The host copy equals the reference the other tests of
that kind use (the oracle for time windows, the count, record and SQL session reference modules); every
other path equals the host copy of a second handle fed the same stream.  Rows compare as sorted tuples
(key, window_start, window_end, values..., first_ord, one NULL bit per value): integers exactly, doubles
by their bits.

This is the host layer, so the shapes are column shapes: three result columns with a non-zero NULL mask,
the first_ord column (the last result column of a DataStream handle with ds_first_ordinals), key rows,
a count handle's ordinals, a record count handle's values[1], a SQL session handle's device-written
NULL mask.  Every stream is three pushes of 300 rows over 40 keys with two collections, so each
collection holds several rows per superbucket; on each path a second collection with nothing emitted
since returns no rows.  The late side output is read on a DataStream session handle (a SQL session
plan has none) and on a DataStream tumble handle with two value columns whose aggregate loads column 1."""
import ctypes as C

import numpy as np
import pytest
from count_record_reference import CountRecordReference
from count_window_reference import CountWindowReference
from session_window_reference import SessionWindowReference
from sql_session_reference import SqlSessionReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

CAP = 1 << 10
T0 = 1_600_000_000_000
SMALL = dict(state_capacity=CAP, max_batch_rows=CAP, output_capacity=CAP)
PATHS = ["host", "device", "async_kernel", "async_dma", "results_device", "segments"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _addr(ptr):
    return C.cast(ptr, C.c_void_p).value


def _host(ptr, n, dtype):
    """n elements of host memory, copied"""
    if n == 0:
        return np.empty(0, dtype)
    raw = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(_addr(ptr))
    return np.frombuffer(raw, dtype=dtype).copy()


def _dev(ptr, n, dtype):
    """n elements of device memory through a device-to-host copy (the caller has drained the handle's stream)"""
    import torch
    if n == 0:
        return np.empty(0, dtype)
    size = np.dtype(dtype).itemsize

    class _View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<i8" if size == 8 else "<i4", "data": (_addr(ptr), False),
                                    "version": 3, "strides": None}
    return torch.as_tensor(_View(), device="cuda").cpu().numpy().view(dtype).copy()


def _table(r, n, n_val, rd):
    """the columns of a fw_result through rd(pointer, n, dtype); a key-row handle's keys are decoded from the key rows"""
    from flink_amd.table.key_rows import decode_key_row
    t = {"key": rd(r.key, n, np.int64), "ws": rd(r.window_start, n, np.int64), "we": rd(r.window_end, n, np.int64),
         "values": [rd(r.values[g], n, np.int64) for g in range(n_val)], "null": rd(r.null_mask, n, np.uint32),
         "ord": rd(r.first_ord, n, np.int64) if r.first_ord else None}
    assert not r.values[n_val], "a value column past the handle's result columns"
    if r.key_row_len:
        st = int(r.key_row_stride)
        lens = rd(r.key_row_len, n, np.int32)
        img = rd(C.cast(r.key_row_bytes, C.POINTER(C.c_int64)), n * st // 8, np.int64).view(np.uint8)
        t["key"] = np.array([decode_key_row(img[i * st:i * st + int(lens[i])].tobytes(), ("BIGINT",))[0] for i in range(n)], np.int64)
    return t


def _rows(t):
    n_val = len(t["values"])
    out = []
    for i in range(len(t["key"])):
        out.append((int(t["key"][i]), int(t["ws"][i]), int(t["we"][i]), *[int(v[i]) for v in t["values"]],
                    None if t["ord"] is None else int(t["ord"][i]), *[int(t["null"][i]) >> g & 1 for g in range(n_val)]))
    return sorted(out)


# ---- the paths: each returns the table of the rows emitted since the last collection, consumed
def _read_results(g, n_val, copy):
    r = abi.fw_result()
    _native.check(_native.lib().fw_results(g._h, C.byref(r), copy))
    t = _table(r, int(r.n), n_val, _host if copy else _dev)
    g.reset_results()
    return t


def _read_async(g, n_val):
    L = _native.lib()
    r = abi.fw_result()
    _native.check(L.fw_results_async(g._h))
    _native.check(L.fw_results_ready(g._h, C.byref(r)))
    return _table(r, int(r.n), n_val, _host)


def _read_results_device(g, n_val):
    r, dn = abi.fw_result(), C.c_void_p()
    _native.check(_native.lib().fw_results_device(g._h, C.byref(r), C.byref(dn)))
    g.sync()
    assert int(r.n) == CAP   # the columns' capacity; the row count is *d_n
    return _table(r, int(_dev(dn, 1, np.int64)[0]), n_val, _dev)


def _read_segments(g, n_val):
    seg = g.result_segments()
    res = g.segments_to_host(seg)
    assert seg.n_segments or len(res["key"]) == 0
    return {"key": res["key"], "ws": res["window_start"], "we": res["window_end"], "values": res["values"][:n_val],
            "null": res["null_mask"], "ord": res.get("first_ord")}


def _read(g, path, n_val):
    if path in ("host", "device"):
        return _read_results(g, n_val, 1 if path == "host" else 0)
    if path.startswith("async"):
        return _read_async(g, n_val)
    return _read_results_device(g, n_val) if path == "results_device" else _read_segments(g, n_val)


def _collect(g, path, n_val):
    """one collection, and a second one with nothing emitted since: no rows"""
    rows = _rows(_read(g, path, n_val))
    assert _rows(_read(g, path, n_val)) == []
    return rows


def _new(cfg, path, monkeypatch):
    from flink_amd.runtime.handle import WindowAggHandle
    if path.startswith("async"):
        monkeypatch.setenv("FW_AR_KERNEL", "1" if path == "async_kernel" else "0")
    return WindowAggHandle(cfg)


def _stream(seed):
    """three pushes of 300 rows over 40 keys, event times over several windows each; the two watermarks"""
    rng = np.random.default_rng(seed)
    pushes = []
    for p in range(3):
        k = rng.integers(0, 40, 300).astype(np.int64) * 7919 - 50000
        ts = (T0 + p * 2000 + rng.integers(0, 3000, 300)).astype(np.int64)
        pushes.append((k, ts, rng.integers(-1000, 1000, 300).astype(np.int64), rng.random(300) < 0.4))
    return pushes, (T0 + 3999, T0 + 20000)


# ---- time windows: the oracle
def _t_cfg():   # SQL tumble, SUM / MAX / COUNT over a nullable BIGINT column
    return abi.make_config(api=abi.API_SQL, window_kind=abi.WIN_TUMBLE, size_ms=1000,
                           aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64), (abi.AGG_COUNT, 0, abi.T_I64)],
                           value_col_types=[abi.T_I64], nullable_cols=(0,), key_hash=abi.KEYHASH_BINROW_BIGINT, **SMALL)


def _d_cfg():   # DataStream tumble, minBy over a DOUBLE field with ties: first_ord is the last result column
    return abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_TUMBLE, size_ms=1000, aggs=[(abi.AGG_MINBY, 0, abi.T_F64, 0)],
                           value_col_types=[abi.T_F64], key_hash=abi.KEYHASH_LONG, ds_first_ordinals=True, **SMALL)


_POOL = np.array([1.0, 2.5, -3.0, 0.5, 1e300, -7.25], np.float64).view(np.int64)


def _time_columns(kind, v, flags):
    if kind == "T":
        return [v], {0: flags}
    return [_POOL[np.abs(v) % len(_POOL)]], None


def _oracle_rows(cfg, kind):
    """per watermark, the oracle's rows of _stream(11 or 12) in this module's row shape"""
    from oracle.oracle import OracleOperator
    o = OracleOperator(cfg)
    pushes, wms = _stream(11 if kind == "T" else 12)
    out = []
    for step in (pushes[0], pushes[1], wms[0], pushes[2], wms[1]):
        if isinstance(step, tuple):
            vals, nulls = _time_columns(kind, step[2], step[3])
            o.process_batch(step[0], step[1], vals, nulls)
            continue
        o.process_watermark(step)
        r = o.results(clear=True)
        out.append(_rows({"key": r["key"], "ws": r["window_start"], "we": r["window_end"], "values": r["values"][:cfg.n_aggs],
                          "null": r["null_mask"], "ord": r["first_ord"] if cfg.ds_first_ordinals else None}))
    o.close()
    return out


_WANT = {}


def _want(kind):
    if kind not in _WANT:   # computed once, shared by the paths
        _WANT[kind] = _oracle_rows(_t_cfg() if kind == "T" else _d_cfg(), kind)
    return _WANT[kind]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ["T", "D"])
def test_time_window_paths(kind, path, monkeypatch):
    cfg = _t_cfg() if kind == "T" else _d_cfg()
    pushes, wms = _stream(11 if kind == "T" else 12)
    want = _want(kind)
    assert all(len(w) > 80 for w in want)   # several rows of every key: more than one row per superbucket slab
    if kind == "T":
        assert any(any(r[-3:]) for w in want for r in w) and any(not all(r[-3:-1]) for w in want for r in w)
    else:
        assert all(r[4] is not None for w in want for r in w)
    g = _new(cfg, path, monkeypatch)
    try:
        got = []
        for step in (pushes[0], pushes[1], wms[0], pushes[2], wms[1]):
            if isinstance(step, tuple):
                vals, nulls = _time_columns(kind, step[2], step[3])
                g.push_host(step[0], step[1], vals, nulls=nulls)
            else:
                g.advance(step)
                got.append(_collect(g, path, cfg.n_aggs))
        assert got == want
        assert g.stats()["error_flags"] == 0
    finally:
        g.close()


# ---- key rows: fw_results in both modes
@pytest.mark.parametrize("path", ["host", "device"])
def test_key_row_hop_paths(path, monkeypatch):
    from flink_amd.table.key_rows import KeyRowColumns
    from oracle.oracle import OracleOperator
    kw = dict(api=abi.API_SQL, window_kind=abi.WIN_HOP, size_ms=3000, slide_ms=1000, count_star_index=0,
              aggs=[(abi.AGG_COUNT_STAR, 0, abi.T_I64), (abi.AGG_SUM, 0, abi.T_I64)], value_col_types=[abi.T_I64], **SMALL)
    cfg = abi.make_config(key_hash=abi.KEYHASH_KEYROW, **kw)
    o = OracleOperator(abi.make_config(key_hash=abi.KEYHASH_PRECOMPUTED, **kw))
    g = _new(cfg, path, monkeypatch)
    pushes, wms = _stream(13)
    try:
        for step in (pushes[0], pushes[1], wms[0], pushes[2], wms[1]):
            if isinstance(step, tuple):
                off, img = KeyRowColumns.from_rows([(int(x),) for x in step[0]], ("BIGINT",)).images_host()
                g.push_host_key_rows(off, img, step[1], [step[2]])
                o.process_batch(step[0], step[1], [step[2]])
                continue
            g.advance(step)
            o.process_watermark(step)
            r = o.results(clear=True)
            want = _rows({"key": r["key"], "ws": r["window_start"], "we": r["window_end"], "values": r["values"][:2],
                          "null": r["null_mask"], "ord": None})
            assert len(want) > 80
            assert _collect(g, path, 2) == want
        assert g.stats()["error_flags"] == 0
    finally:
        g.close()
        o.close()


# ---- count and record count windows: first_ord from the count path's own column, values[1] of a record handle
def _ordinal(i):
    return (i // 300) << 32 | (i % 300)


@pytest.mark.parametrize("path", ["host", "device"])
def test_count_paths(path, monkeypatch):
    cfg = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT, size_ms=5, slide_ms=2, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                          value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG, **SMALL)
    ref = CountWindowReference(5, 2, ("sum", "LONG"))
    g = _new(cfg, path, monkeypatch)
    pushes, _ = _stream(14)
    try:
        for p, (k, _, v, _) in enumerate(pushes):
            g.push_host(k, np.zeros(300, np.int64), [v])
            fired = ref.process(k.tolist(), v.tolist())
            if p == 0:
                want = fired
                continue
            want = sorted((key, ws, we, acc, _ordinal(i), 0) for key, acc, ws, we, i in want + fired)
            assert len(want) > 80
            assert _collect(g, path, 1) == want
            want = []
        assert g.stats()["error_flags"] == 0
    finally:
        g.close()


@pytest.mark.parametrize("path", ["host", "device"])
def test_record_count_paths(path, monkeypatch):
    cfg = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT_RECORD, size_ms=5, slide_ms=2,
                          aggs=[(abi.AGG_MIN, 0, abi.T_I64, 0)], value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG,
                          ds_first_ordinals=True, **SMALL)
    ref = CountRecordReference(5, 2, ("min", "LONG"), field=1)
    g = _new(cfg, path, monkeypatch)
    pushes, _ = _stream(15)
    try:
        want = []
        for p, (k, _, v, _) in enumerate(pushes):
            g.push_host(k, np.zeros(300, np.int64), [v])
            g.first_element_events()   # consumed, as an operator does after every push
            want += ref.process(k.tolist(), list(zip(k.tolist(), v.tolist())), [_ordinal(p * 300 + i) for i in range(300)])
            if p == 0:
                continue
            got = _collect(g, path, 2)
            # (key, value, the ordinal of the record the row is built from, the triggering element's ordinal): the
            # reference has no window bounds
            assert sorted((r[0], r[3], r[4], r[5]) for r in got) == sorted((key, rec[1], ro, o) for key, rec, o, ro in want)
            assert len(got) > 80 and all(r[6:] == (0, 0) for r in got)
            want = []
        assert g.stats()["error_flags"] == 0
    finally:
        g.close()


# ---- SQL session: two aggregates, a NULL mask the device writes
@pytest.mark.parametrize("path", ["host", "device"])
def test_sql_session_paths(path, monkeypatch):
    cfg = abi.make_config(api=abi.API_SQL, window_kind=abi.WIN_SESSION, size_ms=400,
                          aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64)], value_col_types=[abi.T_I64],
                          nullable_cols=(0,), key_hash=abi.KEYHASH_BINROW_BIGINT, **SMALL)
    ref = SqlSessionReference(400, [("SUM", 0, "BIGINT"), ("MAX", 0, "BIGINT")])
    g = _new(cfg, path, monkeypatch)
    pushes, wms = _stream(16)
    try:
        nulls_seen = 0
        for step in (pushes[0], pushes[1], wms[0], pushes[2], wms[1]):
            if isinstance(step, tuple):
                k, ts, v, flags = step
                g.push_host(k, ts, [v], nulls={0: flags})
                assert ref.process(k.tolist(), ts.tolist(), [[None if f else int(x)] for x, f in zip(v.tolist(), flags.tolist())]) == []
                continue
            g.advance(step)
            want = sorted((key, s, e, a, b) for key, a, b, s, e in ref.process_watermark(step))
            got = _collect(g, path, 2)
            assert all(r[5] is None for r in got)   # a session handle's rows carry no ordinal
            assert [(r[0], r[1], r[2], None if r[6] else r[3], None if r[7] else r[4]) for r in got] == want
            assert len(got) > 40
            nulls_seen += sum(r[6] for r in got)
        assert nulls_seen > 0
        assert g.stats()["error_flags"] == 0 and g.stats()["num_late_records_dropped"] == 0
    finally:
        g.close()


# ---- the late side output: both kinds' rows are (key, ts, push_seq, row) and the loaded value columns
def test_session_late_records(monkeypatch):
    cfg = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=100, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                          value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG, late_side_output=True, **SMALL)
    ref = SessionWindowReference(100)
    g = _new(cfg, "host", monkeypatch)
    pushes, wms = _stream(17)
    try:
        for seq in (0, 1):
            k, ts, v, _ = pushes[0] if seq == 0 else pushes[2]
            if seq == 1:
                ts = ts - 4000   # the first push's time range again: behind the watermark
            g.push_host(k, ts, [v])
            late = ref.process(k.tolist(), ts.tolist(), v.tolist())
            lr = g.late_records()
            assert sorted(zip(lr["key"].tolist(), lr["ts"].tolist(), lr["push_seq"].tolist(), lr["row"].tolist(), lr["values"][0].tolist())) == \
                sorted((int(k[i]), int(ts[i]), seq, i, int(v[i])) for i in late)
            assert (len(late) > 100) == (seq == 1)
            if seq == 0:
                g.advance(wms[0])
                ref.process_watermark(wms[0])
        assert g.late_records()["key"].size == 0   # consumed
        assert g.stats()["num_late_records_dropped"] == ref.late_dropped
    finally:
        g.close()


def test_time_window_late_records_scatter_loaded_columns(monkeypatch):
    """two value columns, the aggregate loads column 1: a late row carries that column's value in values[1] and 0 in values[0]"""
    from oracle.oracle import OracleOperator
    cfg = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_TUMBLE, size_ms=1000, aggs=[(abi.AGG_SUM, 1, abi.T_I64)],
                          value_col_types=[abi.T_I64, abi.T_I64], key_hash=abi.KEYHASH_LONG, late_side_output=True, **SMALL)
    o = OracleOperator(cfg)
    g = _new(cfg, "host", monkeypatch)
    pushes, wms = _stream(18)
    try:
        for seq in (0, 1):
            k, ts, v, _ = pushes[0] if seq == 0 else pushes[2]
            if seq == 1:
                ts = ts - 4000
            cols = [v * 3 + 1, v]   # column 0 is never loaded
            g.push_host(k, ts, cols)
            o.process_batch(k, ts, cols)
            lr, so = g.late_records(), o.side_output()
            got = sorted(zip(lr["key"].tolist(), lr["ts"].tolist(), lr["push_seq"].tolist(), lr["row"].tolist()))
            assert got == sorted(zip(so["key"].tolist(), so["ts"].tolist(), so["push_seq"].tolist(), so["row"].tolist()))
            assert all(s == seq and (int(k[i]), int(ts[i])) == (key, t) for key, t, s, i in got)
            assert lr["values"][1].tolist() == [int(v[i]) for i in lr["row"].tolist()]
            assert not lr["values"][0].any()
            assert (len(got) > 100) == (seq == 1)
            if seq == 0:
                g.advance(wms[0])
                o.process_watermark(wms[0])
        assert g.stats()["num_late_records_dropped"] == o.late_dropped
    finally:
        g.close()
        o.close()
