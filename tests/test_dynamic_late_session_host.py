"""Dynamic-gap session windows with an allowed lateness (FW_WIN_SESSION_DYNAMIC_LATENESS) without a
GPU: the worked case and the main stream through fw_host_session_add_gap_late (the routine the
kernel's arrival-order walk runs) against the reference restatement, the two degenerate equalities
(one constant gap: the static-gap lateness reference; lateness 0: the dynamic-gap reference),
configuration validation before any device call, the eligibility seam, and what the GPU tests'
streams reach."""
import ctypes as C

import numpy as np
import pytest
from dynamic_late_session_reference import CLASSES, GAP_MESSAGE, LONG_MIN, DynamicLateSessionReference
from dynamic_late_session_streams import (HOT_LATENESS, HOT_MAX_GAP, LATENESS, MAX_GAP, hot_key_stream, main_stream,
                                          value_words)
from dynamic_session_reference import DynamicSessionReference
from late_session_reference import LateSessionReference

from flink_amd import _native, abi
from flink_amd.datastream import (CountTrigger, DynamicEventTimeSessionWindows, EventTimeSessionWindows, EventTimeTrigger,
                                  LateDynamicSessionWindowOperator, is_late_dynamic_session_window_gpu_eligible)
from flink_amd.datastream.late_dynamic_session_window_operator import is_gpu_eligible

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_TYP = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def _cfg(max_gap, lateness, agg=abi.AGG_SUM, typ=abi.T_I64, **kw):
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_DYNAMIC_LATENESS, size_ms=max_gap, allowed_lateness_ms=lateness,
             aggs=[(agg, 0, typ)], value_col_types=[typ, abi.T_I64], key_hash=abi.KEYHASH_LONG)
    d.update(kw)
    return abi.make_config(**d)


class HostDynamicLateSessions:
    """per key a session list in host arrays, driven only through fw_host_session_add_gap_late; the
    advance is rule 4 applied on the host"""

    def __init__(self, max_gap, lateness, agg=("sum", "LONG"), capacity=128):
        self.cfg, self.cap, self.lateness = _cfg(max_gap, lateness, _AGG[agg[0]], _TYP[agg[1]]), capacity, lateness
        self.keys = {}
        self.watermark = LONG_MIN
        self.dropped = 0

    def _list(self, key):
        if key not in self.keys:
            self.keys[key] = [(C.c_int64 * self.cap)(), (C.c_int64 * self.cap)(), (C.c_int64 * self.cap)(), C.c_int32(0)]
        return self.keys[key]

    def add(self, key, ts, v, gap):
        """(kept, the row fired at once or None)"""
        s, e, a, n = self._list(key)
        out, at = C.c_int32(-7), C.c_int32(-7)
        _native.check(_native.lib().fw_host_session_add_gap_late(C.byref(self.cfg), self.watermark, ts, gap, v, s, e, a,
                                                                 C.byref(n), self.cap, C.byref(out), C.byref(at)))
        assert out.value in (0, 1) and -1 <= at.value < n.value
        if not out.value:
            assert at.value == -1
            self.dropped += 1
            return False, None
        i = at.value
        return True, (None if i < 0 else (key, a[i], s[i], e[i]))

    def process(self, keys, timestamps, values, gaps):
        late, rows = [], []
        for i, (k, ts, v, g) in enumerate(zip(keys, timestamps, values, gaps)):
            kept, row = self.add(k, int(ts), v, int(g))
            if not kept:
                late.append(i)
            if row is not None:
                rows.append(row)
        return late, rows

    def advance(self, w):
        if w <= self.watermark:
            return []
        w0, self.watermark = self.watermark, w
        rows = []
        for key, (s, e, a, n) in self.keys.items():
            keep = []
            for i in range(n.value):
                if w0 < e[i] - 1 <= w:
                    rows.append((key, a[i], s[i], e[i]))
                if e[i] - 1 + self.lateness > w:
                    keep.append((s[i], e[i], a[i]))
            for i, (x, y, z) in enumerate(keep):
                s[i], e[i], a[i] = x, y, z
            n.value = len(keep)
        rows.sort(key=lambda r: (r[3] - 1, r[0], r[2]))
        return rows

    def sessions(self):
        return sorted((k, s[i], e[i], a[i]) for k, (s, e, a, n) in self.keys.items() for i in range(n.value))


# the worked case: key 7, largest gap 100, lateness 50, sum.
# ("push", ts, g, v, kept, immediate row) / ("wm", w, rows) / ("live", sessions)
WORKED_MAX_GAP, WORKED_LATENESS = 100, 50
WORKED = [
    ("push", 1000, 100, 1, True, None),                          # session [1000, 1100) = 1
    ("push", 1010, 10, 2, True, None),                           # inside [1000, 1100): acc = 3
    ("push", 1300, 5, 4, True, None),                            # new session [1300, 1305) = 4
    ("wm", 1310, [(7, 3, 1000, 1100), (7, 4, 1300, 1305)]),      # [1000, 1100): 1099 + 50 <= 1310, gone
    ("live", [(7, 1300, 1305, 4)]),
    ("push", 1290, 10, 8, True, (7, 12, 1290, 1305)),
    ("push", 1200, 100, 16, True, (7, 28, 1200, 1305)),
    ("push", 1250, 5, 32, True, (7, 60, 1200, 1305)),            # inside the fired session
    ("push", 1100, 100, 64, True, (7, 124, 1100, 1305)),         # touches at 1200
    ("push", 1050, 5, 128, False, None),                         # 1054 + 50 <= 1310, intersects nothing
    ("push", 1050, 100, 256, True, (7, 380, 1050, 1305)),        # same timestamp, long gap: kept
    ("push", 1306, 3, 1024, True, (7, 1024, 1306, 1309)),        # new session, 1308 <= 1310
    ("push", 1300, 100, 512, True, None),                        # merges both into [1050, 1400) = 1916, unfired
    ("live", [(7, 1050, 1400, 1916)]),
    ("wm", 1354, []),
    ("wm", 1399, [(7, 1916, 1050, 1400)]),
    ("live", [(7, 1050, 1400, 1916)]),
    ("wm", 1449, []),
    ("live", []),
]


def run_worked(add, advance, sessions):
    for step in WORKED:
        if step[0] == "push":
            assert add(7, step[1], step[3], step[2]) == (step[4], step[5]), step
        elif step[0] == "wm":
            assert advance(step[1]) == step[2], step
        else:
            assert sessions() == step[1], step


def test_worked_case_reference():
    r = DynamicLateSessionReference(WORKED_LATENESS, max_gap=WORKED_MAX_GAP)
    run_worked(r.add, r.process_watermark, r.sessions)
    # one drop; nine rows in all: six at once and three from timers
    assert r.late_dropped == 1 and r.fired == 9 and r.counts["fired_at_once"] == 6


def test_worked_case_host_entry():
    h = HostDynamicLateSessions(WORKED_MAX_GAP, WORKED_LATENESS)
    run_worked(h.add, h.advance, h.sessions)
    assert h.dropped == 1


@pytest.mark.parametrize("agg", [("sum", "LONG"), ("sum", "INT"), ("min", "DOUBLE"), ("count", "LONG")], ids=lambda a: "-".join(a))
def test_host_entry_against_reference_on_the_main_stream(agg):
    h, r = HostDynamicLateSessions(MAX_GAP, LATENESS, agg, capacity=256), DynamicLateSessionReference(LATENESS, agg)
    for k, ts, v, g, wm in main_stream(ftype=agg[1]):
        args = (k.tolist(), ts.tolist(), value_words(v), g.tolist())
        assert h.process(*args) == r.process(*args)
        assert h.sessions() == r.sessions()
        assert h.advance(wm) == r.process_watermark(wm)
        assert h.sessions() == r.sessions() and h.dropped == r.late_dropped
    assert r.late_dropped > 0 and r.counts["fired_at_once"] > 0


def test_one_constant_gap_is_the_static_lateness_reference():
    for agg in (("sum", "LONG"), ("min", "DOUBLE"), ("count", "LONG")):
        for gap in (5, 50, 400):
            dyn, static = DynamicLateSessionReference(LATENESS, agg), LateSessionReference(gap, LATENESS, agg)
            for k, ts, v, g, wm in main_stream(ftype=agg[1]):
                a = dyn.process(k.tolist(), ts.tolist(), value_words(v), [gap] * len(k))
                assert a == static.process(k.tolist(), ts.tolist(), value_words(v))
                assert dyn.sessions() == static.sessions() and dyn.late_dropped == static.late_dropped
                assert dyn.process_watermark(wm) == static.process_watermark(wm)
                assert dyn.sessions() == static.sessions()
            assert dyn.counts == static.counts and dyn.fired == static.fired and dyn.max_live == static.max_live


def test_lateness_zero_is_the_dynamic_gap_reference():
    for agg in (("sum", "LONG"), ("min", "DOUBLE"), ("count", "LONG")):
        late, plain = DynamicLateSessionReference(0, agg), DynamicSessionReference(agg)
        for k, ts, v, g, wm in main_stream(ftype=agg[1]):
            d, at_once = late.process(k.tolist(), ts.tolist(), value_words(v), g.tolist())
            assert d == plain.process(k.tolist(), ts.tolist(), value_words(v), g.tolist()) and at_once == []
            assert late.sessions() == sorted((key, s, e, a) for key, lst in plain.windows.items() for s, e, a in lst)
            assert late.process_watermark(wm) == plain.process_watermark(wm)
            assert late.live_sessions() == plain.live_sessions() and late.late_dropped == plain.late_dropped
        assert late.late_dropped > 0


def test_reference_refuses_a_gap_of_zero():
    with pytest.raises(ValueError, match=GAP_MESSAGE):
        DynamicLateSessionReference(5).add(1, 0, 1, 0)


# ---- what the GPU tests' streams reach --------------------------------------------------------------
def test_main_stream_reaches_every_class():
    r = DynamicLateSessionReference(LATENESS, max_gap=MAX_GAP)
    rows = 0
    for k, ts, v, g, wm in main_stream():
        rows += len(k)
        r.process(k.tolist(), ts.tolist(), value_words(v), g.tolist())
        r.process_watermark(wm)
    print(r.counts, "own_gap_only", r.own_gap_only, "inside_held", r.inside_held, "candidate share", r.candidates / rows,
          "max_live", r.max_live, "dropped", r.late_dropped, "fired", r.fired)
    assert all(r.counts[c] >= 20 for c in CLASSES), r.counts
    assert r.own_gap_only >= 100, r.own_gap_only
    assert r.inside_held >= 100, r.inside_held
    assert 0.1 < r.candidates / rows < 0.3, r.candidates / rows
    assert 64 < r.max_live < 1024, r.max_live


def test_hot_key_stream_pins_the_arrival_order():
    got = []
    for reverse in (False, True):
        r = DynamicLateSessionReference(HOT_LATENESS, max_gap=HOT_MAX_GAP)
        (k1, t1, v1, g1, w1), (k2, t2, v2, g2, w2) = hot_key_stream(reverse)
        assert r.process(k1.tolist(), t1.tolist(), v1.tolist(), g1.tolist()) == ([], [])
        assert len(r.process_watermark(w1)) >= 30
        dropped, at_once = r.process(k2.tolist(), t2.tolist(), v2.tolist(), g2.tolist())
        assert len(dropped) >= 20 and len([x for x in at_once if x[0] == 5]) >= 100
        assert len(set(g2.tolist())) > 1 and len(set(g1.tolist())) > 1     # mixed gaps
        assert int(np.sum(k2 == 5)) > 2048              # the hot key's run spans three tiles
        got.append(sorted(at_once))
    assert got[0] != got[1]


# ---- validation without a device -----------------------------------------------------------------
_REJECTED = [
    (dict(size_ms=0), "gap (size_ms) must be > 0"),
    (dict(size_ms=-5), "gap (size_ms) must be > 0"),
    (dict(size_ms=(1 << 40) + 1), "session gap (size_ms) must be <= 2^40"),
    (dict(allowed_lateness_ms=-1), "session windows: allowed_lateness_ms must be in [0, 2^40]"),
    (dict(allowed_lateness_ms=(1 << 40) + 1), "session windows: allowed_lateness_ms must be in [0, 2^40]"),
    (dict(value_col_types=[abi.T_I64]), "dynamic-gap session windows take two value columns"),
    (dict(value_col_types=[abi.T_I64, abi.T_I64, abi.T_I64]), "dynamic-gap session windows take two value columns"),
    (dict(value_col_types=[abi.T_I64, abi.T_I32]), "the gap column (value column 1) must be FW_T_I64"),
    (dict(aggs=[(abi.AGG_SUM, 1, abi.T_I64)]), "the aggregate reads value column 0"),
    (dict(slide_ms=1), "slide_ms"),
    (dict(offset_ms=1), "offset_ms"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64)]), "n_aggs == 1"),
    (dict(aggs=[(abi.AGG_MINBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_AVG, 0, abi.T_I64)]), "not sum / min / max / count"),
    (dict(nullable_cols=[0]), "nullable_cols"),
    (dict(api=abi.API_SQL, key_hash=abi.KEYHASH_BINROW_BIGINT), "is a DataStream window"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_BIGINT), "BINROW"),
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[m.split()[0] + str(i) for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_configs_fail_without_device(overrides, message):
    kw = dict(size_ms=3000, allowed_lateness_ms=100)
    kw.update(overrides)
    cfg = _cfg(kw.pop("size_ms"), kw.pop("allowed_lateness_ms"), **kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    s, n, out, at = (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    assert L.fw_host_session_add_gap_late(C.byref(cfg), 0, 0, 1, 1, s, s, s, C.byref(n), 4, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()
    # the dynamic form's own rejections carry the same message in FW_WIN_SESSION_DYNAMIC
    if "allowed_lateness_ms" not in overrides:
        dyn = _cfg(overrides.get("size_ms", 3000), 0, **dict(kw, window_kind=abi.WIN_SESSION_DYNAMIC))
        assert L.fw_create(C.byref(dyn), C.byref(h)) == abi.FW_E_INVALID and message in L.fw_last_error().decode()


def test_host_entry_refuses_a_gap_out_of_range():
    L = _native.lib()
    s, e, a, n, out, at = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    cfg = _cfg(100, 50)
    for gap in (0, -3, 101):
        assert L.fw_host_session_add_gap_late(C.byref(cfg), 0, 0, gap, 1, s, e, a, C.byref(n), 4, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
        assert "outside (0, size_ms = 100]" in L.fw_last_error().decode() and n.value == 0
    _native.check(L.fw_host_session_add_gap_late(C.byref(cfg), 0, 0, 100, 1, s, e, a, C.byref(n), 4, C.byref(out), C.byref(at)))
    assert (out.value, n.value, s[0], e[0]) == (1, 1, 0, 100)


def test_bounds_of_gap_and_lateness_are_accepted():
    s, e, a, n, out, at = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    for gap, lateness in ((1, 0), (1 << 40, 1 << 40)):
        n.value = 0
        _native.check(_native.lib().fw_host_session_add_gap_late(C.byref(_cfg(gap, lateness)), 0, (1 << 62) - 1, gap, 1, s, e, a,
                                                                 C.byref(n), 4, C.byref(out), C.byref(at)))
        assert (out.value, at.value, n.value) == (1, -1, 1) and e[0] == (1 << 62) - 1 + gap


def test_capacity_and_other_kinds():
    L = _native.lib()
    h = HostDynamicLateSessions(10, 5, capacity=2)
    assert h.add(1, 0, 1, 10)[0] and h.add(1, 100, 1, 3)[0]
    s, e, a, n = h.keys[1]
    out, at = C.c_int32(), C.c_int32()
    assert L.fw_host_session_add_gap_late(C.byref(h.cfg), LONG_MIN, 200, 4, 1, s, e, a, C.byref(n), 2, C.byref(out), C.byref(at)) == abi.FW_E_CAPACITY
    assert h.add(1, 102, 1, 10)[0] and n.value == 2      # a merge still fits
    kw = dict(api=abi.API_DATASTREAM, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)], value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    plain = abi.make_config(window_kind=abi.WIN_SESSION, **kw)
    late = abi.make_config(window_kind=abi.WIN_SESSION_LATENESS, allowed_lateness_ms=5, **kw)
    dyn = abi.make_config(window_kind=abi.WIN_SESSION_DYNAMIC, **dict(kw, value_col_types=[abi.T_I64, abi.T_I64]))
    tumble = abi.make_config(window_kind=abi.WIN_TUMBLE, **kw)
    for other in (plain, late, dyn, tumble):   # the new entry keeps to its kind
        assert L.fw_host_session_add_gap_late(C.byref(other), 0, 0, 5, 1, s, e, a, C.byref(n), 2, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
        assert "needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration" in L.fw_last_error().decode()
    # and the three older entries refuse the new kind
    assert L.fw_host_session_add(C.byref(h.cfg), 0, 0, 1, s, e, a, C.byref(n), 2, C.byref(out)) == abi.FW_E_INVALID
    assert "needs a FW_WIN_SESSION configuration" in L.fw_last_error().decode()
    assert L.fw_host_session_add_gap(C.byref(h.cfg), 0, 0, 5, 1, s, e, a, C.byref(n), 2, C.byref(out)) == abi.FW_E_INVALID
    assert "needs a FW_WIN_SESSION_DYNAMIC configuration" in L.fw_last_error().decode()
    assert L.fw_host_session_add_late(C.byref(h.cfg), 0, 0, 1, s, e, a, C.byref(n), 2, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
    assert "needs a FW_WIN_SESSION_LATENESS configuration" in L.fw_last_error().decode()
    nw = C.c_int32()
    assert L.fw_host_sql_session_words(C.byref(h.cfg), C.byref(nw)) == abi.FW_E_INVALID
    t = C.c_int64()
    assert L.fw_host_time_op(C.byref(h.cfg), 3, 0, C.byref(t)) == abi.FW_E_INVALID
    assert "not for session windows" in L.fw_last_error().decode()


def test_the_older_kinds_keep_their_lateness_rules():
    """FW_WIN_SESSION_DYNAMIC still refuses a lateness; FW_WIN_SESSION_LATENESS is still a static-gap kind"""
    L, h = _native.lib(), C.c_void_p()
    kw = dict(api=abi.API_DATASTREAM, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)], key_hash=abi.KEYHASH_LONG)
    dyn = abi.make_config(window_kind=abi.WIN_SESSION_DYNAMIC, allowed_lateness_ms=5, value_col_types=[abi.T_I64, abi.T_I64], **kw)
    assert L.fw_create(C.byref(dyn), C.byref(h)) == abi.FW_E_INVALID and "allowed_lateness_ms must be 0" in L.fw_last_error().decode()


# ---- eligibility and exports -----------------------------------------------------------------------
def test_eligibility_accepts():
    a, t = DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 5), EventTimeTrigger.create()
    assert is_late_dynamic_session_window_gpu_eligible is is_gpu_eligible
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("count", "LONG")]:
        for lateness in (0, 1, 60000, 1 << 40):
            for max_gap in (1, 400, 1 << 40):
                assert is_gpu_eligible(a, t, agg, max_gap=max_gap, allowed_lateness=lateness) == (True, "")
    assert is_gpu_eligible(a, t, ("sum", "LONG"), allowed_lateness=5, conf={"gpu.window-agg.enabled": "true"}) == (True, "")
    op = LateDynamicSessionWindowOperator(400, 500, ("max", "DOUBLE"), late_side_output=True)
    assert op.cfg.window_kind == abi.WIN_SESSION_DYNAMIC_LATENESS == 7
    assert op.cfg.allowed_lateness_ms == 500 and op.cfg.size_ms == 400 and op.cfg.n_value_cols == 2
    assert list(op.cfg.value_col_types[:2]) == [abi.T_F64, abi.T_I64]
    for name in ("process_batch", "process_batch_device", "process_segments_device", "process_packed_segments_device",
                 "process_watermark", "process_watermark_device", "collect", "late_records", "snapshot_state", "initialize_state",
                 "_check_gaps"):
        assert callable(getattr(op, name))
    with pytest.raises(ValueError, match=GAP_MESSAGE):       # the host gap checks, before anything is pushed
        op.process_batch([1], [0], [1.0], [0])
    with pytest.raises(ValueError, match="exceeds max_gap_ms = 400"):
        op.process_batch([1], [0], [1.0], [401])


def test_eligibility_refusals_give_reasons():
    a, t, sl = DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 5), EventTimeTrigger.create(), ("sum", "LONG")
    cases = [
        (dict(allowed_lateness=-1), "allowedLateness must be in [0, 2^40]"),
        (dict(allowed_lateness=(1 << 40) + 1), "allowedLateness must be in [0, 2^40]"),
        (dict(max_gap=0), "max_gap must be in (0, 2^40]"),
        (dict(max_gap=(1 << 40) + 1), "max_gap must be in (0, 2^40]"),
        (dict(evictor=object()), "evictor"),
        (dict(trigger=CountTrigger.of(3)), "EventTimeTrigger"),
        (dict(aggregation=("minBy", "LONG")), "minBy"),
        (dict(aggregation=("sum", "FLOAT")), "FLOAT"),
        (dict(assigner=EventTimeSessionWindows.with_gap(3000)), "DynamicEventTimeSessionWindows"),
    ]
    for kw, why in cases:
        args = dict(assigner=a, trigger=t, aggregation=sl)
        args.update(kw)
        ok, reason = is_gpu_eligible(args.pop("assigner"), args.pop("trigger"), args.pop("aggregation"), **args)
        assert not ok and why in reason, (why, reason)
    ok, reason = is_gpu_eligible(a, t, sl, conf={"gpu.window-agg.enabled": "false"})
    assert not ok and "gpu.window-agg.enabled" in reason
    with pytest.raises(ValueError, match="allowedLateness"):
        LateDynamicSessionWindowOperator(400, -1)
    with pytest.raises(ValueError, match="max_gap"):
        LateDynamicSessionWindowOperator(0, 5)
    # the two older seams keep their refusals
    from flink_amd.datastream import is_dynamic_session_window_gpu_eligible, is_late_session_window_gpu_eligible
    ok, reason = is_dynamic_session_window_gpu_eligible(a, t, sl, allowed_lateness=1)
    assert not ok and "allowedLateness" in reason
    ok, reason = is_late_session_window_gpu_eligible(a, t, sl, allowed_lateness=1)
    assert not ok and "dynamic gaps" in reason


def test_abi():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_session_add_gap_late") and "fw_host_session_add_gap_late" in _native.EXPORTED
    assert abi.WIN_SESSION_DYNAMIC_LATENESS == 7
