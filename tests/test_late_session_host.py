"""Session windows with an allowed lateness (FW_WIN_SESSION_LATENESS) without a GPU: the worked case
and random streams through fw_host_session_add_late (the routine the kernel's arrival-order walk
runs) against the reference restatement, lateness 0 against the plain session reference,
configuration validation before any device call, the eligibility seam, and what the GPU tests'
streams reach."""
import ctypes as C

import numpy as np
import pytest
from late_session_reference import CLASSES, LONG_MIN, LateSessionReference
from late_session_streams import GAP, LATENESS, hot_key_stream, HOT_GAP, HOT_LATENESS, main_stream, value_words
from session_window_reference import SessionWindowReference

from flink_amd import _native, abi
from flink_amd.datastream import (CountTrigger, EventTimeSessionWindows, EventTimeTrigger, LateSessionWindowOperator,
                                  TumblingEventTimeWindows, is_late_session_window_gpu_eligible)
from flink_amd.datastream.late_session_window_operator import is_gpu_eligible

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_TYP = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def _cfg(gap, lateness, agg=abi.AGG_SUM, typ=abi.T_I64, **kw):
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_LATENESS, size_ms=gap, allowed_lateness_ms=lateness,
             aggs=[(agg, 0, typ)], value_col_types=[typ], key_hash=abi.KEYHASH_LONG)
    d.update(kw)
    return abi.make_config(**d)


class HostLateSessions:
    """per key a session list in host arrays, driven only through fw_host_session_add_late; the
    advance is rule 4 applied on the host"""

    def __init__(self, gap, lateness, agg=("sum", "LONG"), capacity=128):
        self.cfg, self.cap, self.lateness = _cfg(gap, lateness, _AGG[agg[0]], _TYP[agg[1]]), capacity, lateness
        self.keys = {}
        self.watermark = LONG_MIN
        self.dropped = 0

    def _list(self, key):
        if key not in self.keys:
            self.keys[key] = [(C.c_int64 * self.cap)(), (C.c_int64 * self.cap)(), (C.c_int64 * self.cap)(), C.c_int32(0)]
        return self.keys[key]

    def add(self, key, ts, v):
        """(kept, the row fired at once or None)"""
        s, e, a, n = self._list(key)
        out, at = C.c_int32(-7), C.c_int32(-7)
        _native.check(_native.lib().fw_host_session_add_late(C.byref(self.cfg), self.watermark, ts, v, s, e, a, C.byref(n),
                                                             self.cap, C.byref(out), C.byref(at)))
        assert out.value in (0, 1) and -1 <= at.value < n.value
        if not out.value:
            assert at.value == -1
            self.dropped += 1
            return False, None
        i = at.value
        return True, (None if i < 0 else (key, a[i], s[i], e[i]))

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


# the worked case (Lateness; transcribed from a hand-checked model): key A, gap 3, lateness 5.  ("push", ts, v, kept, immediate row) / ("wm", w, rows)
WORKED = [
    ("push", 0, 1, True, None), ("push", 2, 2, True, None),
    ("wm", 4, [("A", 3, 0, 5)]),
    ("push", 1, 10, True, ("A", 13, 0, 5)),
    ("push", 5, 100, True, None),                 # touches [0, 5): [0, 8), unfired
    ("wm", 7, [("A", 113, 0, 8)]),
    ("push", -10, 7, False, None),
    ("push", 9, 1, True, None),
    ("wm", 12, [("A", 1, 9, 12)]),                # [0, 8) is cleaned silently: 7 + 5 <= 12
    ("push", 6, 5, True, ("A", 6, 6, 12)),        # late but allowed; touches [9, 12)
    ("push", 1, 3, False, None),
    ("wm", 20, []),
]


def test_worked_case_reference():
    r = LateSessionReference(3, 5)
    for step in WORKED:
        if step[0] == "push":
            assert r.add("A", step[1], step[2]) == (step[3], step[4]), step
        else:
            assert r.process_watermark(step[1]) == step[2], step
    assert r.live_sessions() == 0 and r.late_dropped == 2 and r.fired == 5
    assert r.counts["cleaned_silent"] == 2 and r.counts["fired_at_once"] == 2


def test_worked_case_host_entry():
    h = HostLateSessions(3, 5)
    for step in WORKED:
        if step[0] == "push":
            assert h.add("A", step[1], step[2]) == (step[3], step[4]), step
        else:
            assert h.advance(step[1]) == step[2], step
    assert h.sessions() == [] and h.dropped == 2


def test_two_late_elements_into_one_fired_session_emit_cumulative_rows():
    for order, rows in (((4, 10), (6, 100)), ((6, 100), (4, 10))):
        h, r = HostLateSessions(10, 100), LateSessionReference(10, 100)
        for x in (h, r):
            assert x.add(1, 5, 1) == (True, None)
        assert h.advance(50) == r.process_watermark(50) == [(1, 1, 5, 15)]
        got = [h.add(1, ts, v) for ts, v in (order, rows)]
        assert got == [r.add(1, ts, v) for ts, v in (order, rows)]
        first = order[1] + 1
        assert [g[1][1] for g in got] == [first, first + rows[1]]      # the second row holds the first element


def test_boundaries_of_drop_fire_and_cleanup():
    h, r = HostLateSessions(10, 20), LateSessionReference(10, 20)
    assert h.advance(129) == r.process_watermark(129) == []
    assert h.add(1, 100, 1) == r.add(1, 100, 1) == (False, None)                 # 100 + 9 + 20 == W: dropped
    assert h.add(1, 101, 2) == r.add(1, 101, 2) == (True, (1, 2, 101, 111))      # one later: kept, fires at once, alone
    assert h.add(1, 120, 4) == r.add(1, 120, 4) == (True, (1, 4, 120, 130))      # end - 1 == W: fires at once
    assert h.add(1, 121, 8) == r.add(1, 121, 8) == (True, None)                  # touches [120, 130): [120, 131), unfired
    assert h.advance(130) == r.process_watermark(130) == [(1, 12, 120, 131)]     # [101, 111): 110 + 20 <= 130, silent
    assert h.sessions() == r.sessions() == [(1, 120, 131, 12)]
    assert h.advance(149) == r.process_watermark(149) == [] and h.sessions() == [(1, 120, 131, 12)]
    assert h.advance(150) == r.process_watermark(150) == [] and h.sessions() == r.sessions() == []


@pytest.mark.parametrize("agg", [("sum", "LONG"), ("sum", "INT"), ("min", "DOUBLE"), ("max", "DOUBLE"), ("sum", "DOUBLE"),
                                 ("count", "LONG")], ids=lambda a: "-".join(a))
def test_random_streams_against_reference(agg):
    rng = np.random.default_rng(sum(map(ord, "".join(agg))))
    for gap, lateness in ((5, 0), (5, 3), (7, 40), (3, 1000)):
        h, r = HostLateSessions(gap, lateness, agg), LateSessionReference(gap, lateness, agg)
        w = 0
        for step in range(600):
            if rng.random() < 0.08:
                w += int(rng.integers(0, 25))
                assert h.advance(w) == r.process_watermark(w)
                continue
            key, ts = int(rng.integers(0, 3)), w + int(rng.integers(-60, 30))
            v = float(rng.integers(-50, 50)) / 4 if agg[1] == "DOUBLE" else int(rng.integers(-2**31, 2**31))
            word = value_words(np.array([v]))[0] if agg[1] == "DOUBLE" else v
            assert h.add(key, ts, word) == r.add(key, ts, word), (gap, lateness, step)
        assert h.sessions() == r.sessions() and h.dropped == r.late_dropped
        assert (lateness >= 1000 or r.counts["dropped"]) and (lateness == 0 or r.counts["fired_at_once"])


def test_lateness_zero_is_the_plain_session_reference():
    for agg in (("sum", "LONG"), ("min", "DOUBLE"), ("count", "LONG")):
        rows = main_stream(ftype=agg[1])
        late, plain = LateSessionReference(GAP, 0, agg), SessionWindowReference(GAP, agg)
        for k, ts, v, wm in rows:
            d, at_once = late.process(k.tolist(), ts.tolist(), value_words(v))
            assert d == plain.process(k.tolist(), ts.tolist(), value_words(v)) and at_once == []
            assert late.process_watermark(wm) == plain.process_watermark(wm)
        assert late.live_sessions() == plain.live_sessions() and late.late_dropped == plain.late_dropped > 0


def test_capacity_and_other_kinds():
    L = _native.lib()
    h = HostLateSessions(10, 5, capacity=2)
    assert h.add(1, 0, 1)[0] and h.add(1, 100, 1)[0]
    s, e, a, n = h.keys[1]
    out, at = C.c_int32(), C.c_int32()
    assert L.fw_host_session_add_late(C.byref(h.cfg), LONG_MIN, 200, 1, s, e, a, C.byref(n), 2, C.byref(out), C.byref(at)) == abi.FW_E_CAPACITY
    assert h.add(1, 105, 1)[0] and n.value == 2      # a merge still fits
    kw = dict(api=abi.API_DATASTREAM, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)], value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    plain = abi.make_config(window_kind=abi.WIN_SESSION, **kw)
    dyn = abi.make_config(window_kind=abi.WIN_SESSION_DYNAMIC, **dict(kw, value_col_types=[abi.T_I64, abi.T_I64]))
    tumble = abi.make_config(window_kind=abi.WIN_TUMBLE, **kw)
    for other in (plain, dyn, tumble):   # the new entry keeps to its kind
        assert L.fw_host_session_add_late(C.byref(other), 0, 0, 1, s, e, a, C.byref(n), 2, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
        assert "FW_WIN_SESSION_LATENESS" in L.fw_last_error().decode()
    # and the other kinds' entries refuse the new kind
    assert L.fw_host_session_add(C.byref(h.cfg), 0, 0, 1, s, e, a, C.byref(n), 2, C.byref(out)) == abi.FW_E_INVALID
    assert "needs a FW_WIN_SESSION configuration" in L.fw_last_error().decode()
    assert L.fw_host_session_add_gap(C.byref(h.cfg), 0, 0, 5, 1, s, e, a, C.byref(n), 2, C.byref(out)) == abi.FW_E_INVALID
    assert "FW_WIN_SESSION_DYNAMIC" in L.fw_last_error().decode()
    nw = C.c_int32()
    assert L.fw_host_sql_session_words(C.byref(h.cfg), C.byref(nw)) == abi.FW_E_INVALID
    t = C.c_int64()
    assert L.fw_host_time_op(C.byref(h.cfg), 3, 0, C.byref(t)) == abi.FW_E_INVALID
    assert "not for session windows" in L.fw_last_error().decode()


# ---- validation without a device -----------------------------------------------------------------
_REJECTED = [
    (dict(size_ms=0), "gap (size_ms) must be > 0"),
    (dict(size_ms=-5), "gap (size_ms) must be > 0"),
    (dict(size_ms=(1 << 40) + 1), "session gap (size_ms) must be <= 2^40"),
    (dict(allowed_lateness_ms=-1), "allowed_lateness_ms must be in [0, 2^40]"),
    (dict(allowed_lateness_ms=(1 << 40) + 1), "allowed_lateness_ms must be in [0, 2^40]"),
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
def test_invalid_late_session_configs_fail_without_device(overrides, message):
    kw = dict(size_ms=3000, allowed_lateness_ms=100)
    kw.update(overrides)
    cfg = _cfg(kw.pop("size_ms"), kw.pop("allowed_lateness_ms"), **kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    s, n, out, at = (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    assert L.fw_host_session_add_late(C.byref(cfg), 0, 0, 1, s, s, s, C.byref(n), 4, C.byref(out), C.byref(at)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_bounds_of_gap_and_lateness_are_accepted():
    s, e, a, n, out, at = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    for gap, lateness in ((1, 0), (1 << 40, 1 << 40)):
        n.value = 0
        _native.check(_native.lib().fw_host_session_add_late(C.byref(_cfg(gap, lateness)), 0, (1 << 62) - 1, 1, s, e, a, C.byref(n), 4,
                                                             C.byref(out), C.byref(at)))
        assert (out.value, at.value, n.value) == (1, -1, 1)


# ---- eligibility ---------------------------------------------------------------------------------
def test_eligibility_accepts_lateness():
    a, t = EventTimeSessionWindows.with_gap(3000), EventTimeTrigger.create()
    assert is_late_session_window_gpu_eligible is is_gpu_eligible
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("count", "LONG")]:
        for lateness in (0, 1, 60000, 1 << 40):
            assert is_gpu_eligible(a, t, agg, allowed_lateness=lateness) == (True, "")
    assert is_gpu_eligible(a, t, ("sum", "LONG"), allowed_lateness=5, conf={"gpu.window-agg.enabled": "true"}) == (True, "")
    op = LateSessionWindowOperator(3000, 500, ("max", "DOUBLE"), late_side_output=True)
    assert op.cfg.window_kind == abi.WIN_SESSION_LATENESS == 6 and op.cfg.allowed_lateness_ms == 500 and op.cfg.size_ms == 3000
    for name in ("process_batch", "process_batch_device", "process_segments_device", "process_packed_segments_device",
                 "process_watermark", "process_watermark_device", "collect", "late_records", "snapshot_state", "initialize_state"):
        assert callable(getattr(op, name))


def test_eligibility_refusals_give_reasons():
    a, t, sl = EventTimeSessionWindows.with_gap(3000), EventTimeTrigger.create(), ("sum", "LONG")

    class DynamicGap:
        def is_event_time(self):
            return True
    cases = [
        (dict(allowed_lateness=-1), "allowedLateness"),
        (dict(allowed_lateness=(1 << 40) + 1), "allowedLateness"),
        (dict(evictor=object()), "evictor"),
        (dict(trigger=CountTrigger.of(3)), "EventTimeTrigger"),
        (dict(aggregation=("minBy", "LONG")), "minBy"),
        (dict(aggregation=("sum", "FLOAT")), "FLOAT"),
        (dict(assigner=DynamicGap()), "dynamic gaps"),
        (dict(assigner=TumblingEventTimeWindows.of(1000)), "EventTimeSessionWindows"),
    ]
    for kw, why in cases:
        args = dict(assigner=a, trigger=t, aggregation=sl)
        args.update(kw)
        ok, reason = is_gpu_eligible(args.pop("assigner"), args.pop("trigger"), args.pop("aggregation"), **args)
        assert not ok and why in reason, (why, reason)
    ok, reason = is_gpu_eligible(a, t, sl, conf={"gpu.window-agg.enabled": "false"})
    assert not ok and "gpu.window-agg.enabled" in reason
    with pytest.raises(ValueError, match="allowedLateness"):
        LateSessionWindowOperator(3000, -1)
    # the plain session seam still refuses a lateness
    from flink_amd.datastream import is_session_window_gpu_eligible
    ok, reason = is_session_window_gpu_eligible(a, t, sl, allowed_lateness=1)
    assert not ok and "allowedLateness" in reason


# ---- what the GPU tests' streams reach --------------------------------------------------------------
def test_main_stream_reaches_every_class():
    r = LateSessionReference(GAP, LATENESS)
    candidates = rows = 0
    for k, ts, v, wm in main_stream():
        candidates += int(np.sum(ts + GAP - 1 <= r.watermark))
        rows += len(k)
        r.process(k.tolist(), ts.tolist(), value_words(v))
        r.process_watermark(wm)
    assert all(r.counts[c] >= 20 for c in CLASSES), r.counts
    assert 0.1 < candidates / rows < 0.3, candidates / rows
    assert 64 < r.max_live < 1024, r.max_live


def test_hot_key_stream_pins_the_arrival_order():
    got = []
    for reverse in (False, True):
        r = LateSessionReference(HOT_GAP, HOT_LATENESS)
        (k1, t1, v1, w1), (k2, t2, v2, w2) = hot_key_stream(reverse)
        assert r.process(k1.tolist(), t1.tolist(), v1.tolist()) == ([], [])
        assert len(r.process_watermark(w1)) >= 30
        dropped, at_once = r.process(k2.tolist(), t2.tolist(), v2.tolist())
        assert len(dropped) >= 20 and len([x for x in at_once if x[0] == 5]) >= 100
        per_session = {}
        for key, acc, s, e in at_once:
            per_session.setdefault(key, []).append(e)
        assert int(np.sum(k2 == 5)) > 2048              # the hot key's run spans three tiles
        got.append(sorted(at_once))
    assert got[0] != got[1]


def test_abi():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_session_add_late") and "fw_host_session_add_late" in _native.EXPORTED
    assert abi.WIN_SESSION_LATENESS == 6
