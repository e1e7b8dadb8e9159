"""Session windows (EventTimeSessionWindows.withGap) without a GPU: the reference restatement's hand
vectors and the transcribed testSessionWindows case, the library's per-key session arithmetic
(fw_host_session_add, the routine the kernel's exact path runs) against the reference,
configuration validation before any device call, the eligibility seam, the assigner mirror and the
ABI."""
import ctypes as C

import numpy as np
import pytest
from session_window_reference import LONG_MIN, SessionWindowReference

from flink_amd import _native, abi
from flink_amd.datastream import (CountTrigger, EventTimeSessionWindows, EventTimeTrigger, TumblingEventTimeWindows)
from flink_amd.datastream.session_window_operator import is_gpu_eligible

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}


def _cfg(gap, agg=abi.AGG_SUM, typ=abi.T_I64, **kw):
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=gap, aggs=[(agg, 0, typ)],
             value_col_types=[typ], key_hash=abi.KEYHASH_LONG)
    d.update(kw)
    return abi.make_config(**d)


class HostSessions:
    """one key's session list in host arrays, driven only through fw_host_session_add"""

    def __init__(self, cfg, capacity=256):
        self.cfg, self.cap = cfg, capacity
        self.s = (C.c_int64 * capacity)()
        self.e = (C.c_int64 * capacity)()
        self.a = (C.c_int64 * capacity)()
        self.n = C.c_int32(0)

    def add(self, watermark, ts, v):
        out = C.c_int32(-7)
        _native.check(_native.lib().fw_host_session_add(C.byref(self.cfg), watermark, ts, v, self.s, self.e, self.a,
                                                        C.byref(self.n), self.cap, C.byref(out)))
        assert out.value in (0, 1)
        return bool(out.value)

    def sessions(self):
        return [[self.s[i], self.e[i], self.a[i]] for i in range(self.n.value)]

    def fire(self, watermark):
        """what fw_advance does to the list: sessions with end - 1 <= watermark leave"""
        keep = [x for x in self.sessions() if x[1] - 1 > watermark]
        fired = [x for x in self.sessions() if x[1] - 1 <= watermark]
        for i, (s, e, a) in enumerate(keep):
            self.s[i], self.e[i], self.a[i] = s, e, a
        self.n.value = len(keep)
        return fired


def _both(gap, agg=("sum", "LONG")):
    fn, ft = agg
    typ = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}[ft]
    return HostSessions(_cfg(gap, _AGG[fn], typ)), SessionWindowReference(gap, agg)


def _add(h, r, ts, v, key=7):
    got, want = h.add(r.watermark, ts, v), r.add(key, ts, v)
    assert got == want
    assert h.sessions() == r.windows.get(key, [])
    return got


# ---- the transcribed case -------------------------------------------------------------------------
def test_reference_transcribed_session_windows_case():
    """WindowOperatorTest.testSessionWindows (gap 3000, sum), recalled from the reference's test: the
    elements, the two watermarks and the rows they fire; a snapshot / restore after the fifth element."""
    r = SessionWindowReference(3000, ("sum", "LONG"))
    first = [("key2", 0, 1), ("key2", 1000, 2), ("key2", 2500, 3), ("key1", 10, 1), ("key1", 1000, 2)]
    for k, ts, v in first:
        assert r.add(k, ts, v)
    snap = r.snapshot()
    r = SessionWindowReference(3000, ("sum", "LONG"))
    r.restore(snap)
    for k, ts, v in [("key1", 2500, 3), ("key2", 5501, 4), ("key2", 6000, 5), ("key2", 6000, 5), ("key2", 6050, 6)]:
        assert r.add(k, ts, v)
    assert r.process_watermark(12000) == [("key1", 6, 10, 5500), ("key2", 6, 0, 5500), ("key2", 20, 5501, 9050)]
    assert r.add("key1", 15000, 10) and r.add("key1", 15000, 20)
    assert r.process_watermark(17999) == [("key1", 30, 15000, 18000)]
    assert r.live_sessions() == 0 and r.late_dropped == 0


# ---- fw_host_session_add: the explicit cases --------------------------------------------------------
def test_touch_at_exactly_gap_merges_and_gap_plus_one_does_not():
    h, r = _both(10)
    _add(h, r, 100, 1)
    _add(h, r, 110, 2)            # [110, 120) touches [100, 110)
    assert h.sessions() == [[100, 120, 3]]
    _add(h, r, 131, 4)            # 131 > 120: apart
    assert h.sessions() == [[100, 120, 3], [131, 141, 4]]
    _add(h, r, 89, 8)             # 89 + 10 = 99 < 100: apart
    _add(h, r, 79, 16)            # 79 + 10 = 89: touches
    assert h.sessions() == [[79, 99, 24], [100, 120, 3], [131, 141, 4]]


def test_one_element_bridges_two_and_three_sessions():
    """Sessions are at least a gap long and an element's window exactly a gap, so one element joins at
    most two sessions of a non-touching list (three windows with its own); three sessions become one
    through two elements."""
    h, r = _both(10)
    for ts in (0, 20, 40):
        _add(h, r, ts, 1)
    assert h.n.value == 3
    _add(h, r, 10, 100)           # [10, 20) touches [0, 10) and [20, 30)
    assert h.sessions() == [[0, 30, 102], [40, 50, 1]]
    h, r = _both(10)
    for ts in (0, 15, 30, 60):
        _add(h, r, ts, 1)
    _add(h, r, 8, 100)            # [8, 18): [0, 10) and [15, 25)
    assert h.sessions() == [[0, 25, 102], [30, 40, 1], [60, 70, 1]]
    h, r = _both(20)
    for ts, g in ((0, 1), (25, 2), (50, 4)):
        _add(h, r, ts, g)
    assert h.n.value == 3
    _add(h, r, 22, 100)           # [22, 42) reaches back to [0, 20)?  no: 22 > 20 -- joins [25, 45) only
    assert h.sessions() == [[0, 20, 1], [22, 45, 102], [50, 70, 4]]
    _add(h, r, 20, 1000)          # [20, 40): touches [0, 20), inside [22, 45)
    _add(h, r, 30, 10000)         # [30, 50): touches [50, 70): three became one
    assert h.sessions() == [[0, 70, 11107]]


def test_late_alone_boundary():
    h, r = _both(10)
    r.process_watermark(109)
    assert not _add(h, r, 100, 1)      # 100 + 10 - 1 == W: late, alone: dropped
    assert _add(h, r, 101, 2)          # == W + 1: stays
    assert h.sessions() == [[101, 111, 2]] and r.late_dropped == 1


def test_rule_3_both_orders():
    # late A then on-time B whose window would have reached A: A is dropped
    h, r = _both(10)
    r.process_watermark(104)
    assert not _add(h, r, 95, 1)       # A: [95, 105), late, alone
    assert _add(h, r, 100, 2)          # B: [100, 110)
    assert h.sessions() == [[100, 110, 2]]
    # B then A: A is kept and moves the session's start back
    h, r = _both(10)
    r.process_watermark(104)
    assert _add(h, r, 100, 2)
    assert _add(h, r, 95, 1)
    assert h.sessions() == [[95, 110, 3]]


def test_backward_chain_of_three_late_candidates():
    h, r = _both(10)
    r.process_watermark(104)
    assert _add(h, r, 100, 1)          # live: [100, 110)
    assert _add(h, r, 90, 2)           # [90, 100) late but touches -> [90, 110)
    assert _add(h, r, 80, 4)           # enabled by the one before
    assert _add(h, r, 70, 8)
    assert h.sessions() == [[70, 110, 15]]
    h, r = _both(10)                   # the same three without the anchor, farthest first: all dropped
    r.process_watermark(104)
    assert not _add(h, r, 70, 8) and not _add(h, r, 80, 4) and not _add(h, r, 90, 2)
    assert h.sessions() == [] and r.late_dropped == 3


def test_fire_boundary():
    h, r = _both(10)
    _add(h, r, 100, 1)                 # end 110
    _add(h, r, 121, 2)                 # end 131
    assert r.process_watermark(108) == [] and h.fire(108) == []      # end - 1 == W' + 1
    assert r.process_watermark(109) == [(7, 1, 100, 110)] and h.fire(109) == [[100, 110, 1]]   # end - 1 == W'
    assert r.process_watermark(109) == [] and r.process_watermark(50) == []
    assert h.sessions() == r.windows[7] == [[121, 131, 2]]


# ---- fw_host_session_add over random streams ---------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 3, 1000])
@pytest.mark.parametrize("agg", [("sum", "LONG"), ("min", "LONG"), ("max", "INT"), ("count", "LONG"), ("sum", "INT")])
def test_host_session_add_equals_reference(gap, agg):
    rng = np.random.default_rng(gap * 7 + len(agg[0]))
    h, r = _both(gap, agg)
    base, late_cands, dropped, fired = 0, 0, 0, 0
    for step in range(3000):
        ts = base + int(rng.integers(0, 8 * gap + 2))     # a few gaps wide: touching and bridging are frequent
        if rng.random() < 0.1:                            # about a tenth behind the watermark
            ts = r.watermark - int(rng.integers(0, 3 * gap + 1)) if r.watermark > LONG_MIN else ts
        v = int(rng.integers((1 << 31) - 1000, 1 << 31)) if agg == ("sum", "INT") else int(rng.integers(-1000, 1000))
        late_cands += ts + gap - 1 <= r.watermark
        dropped += not _add(h, r, ts, v)
        if step % 7 == 6:
            base += int(rng.integers(0, 12 * gap + 1))
            w = base - int(rng.integers(0, 2 * gap + 1))
            want = [[s, e, a] for _, a, s, e in r.process_watermark(w)]
            got = h.fire(w)
            assert sorted(got) == sorted(want)
            fired += len(want)
            assert h.sessions() == r.windows.get(7, [])
    assert 150 < late_cands < 600 and 20 < dropped < late_cands and fired > 100   # the stream is what it should be


@pytest.mark.parametrize("fn", ["min", "max"])
def test_host_session_add_double_compare_order(fn):
    nz, pz = np.float64(-0.0).view(np.int64).item(), 0
    one = np.float64(1.0).view(np.int64).item()
    nan = 0x7FF8000000000000
    for vals in ([pz, nz], [nz, pz], [one, nan], [nan, one], [nz, one, pz]):
        h, r = _both(10, (fn, "DOUBLE"))
        for i, v in enumerate(vals):
            _add(h, r, 100 + i, v)
    h, r = _both(10, ("sum", "DOUBLE"))
    for i, x in enumerate([1.5, 2.25, 1e10]):
        _add(h, r, 100 + i, np.float64(x).view(np.int64).item())
    assert np.int64(h.sessions()[0][2]).view(np.float64) == 1.5 + 2.25 + 1e10


def test_host_session_add_capacity_and_arguments():
    h = HostSessions(_cfg(10), capacity=2)
    assert h.add(LONG_MIN, 0, 1) and h.add(LONG_MIN, 100, 1)
    out = C.c_int32()
    L = _native.lib()
    assert L.fw_host_session_add(C.byref(h.cfg), LONG_MIN, 200, 1, h.s, h.e, h.a, C.byref(h.n), 2, C.byref(out)) == abi.FW_E_CAPACITY
    assert h.add(LONG_MIN, 105, 1) and h.n.value == 2      # a merge still fits
    tumble = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_TUMBLE, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                             value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    assert L.fw_host_session_add(C.byref(tumble), 0, 0, 1, h.s, h.e, h.a, C.byref(h.n), 2, C.byref(out)) == abi.FW_E_INVALID
    assert "FW_WIN_SESSION" in L.fw_last_error().decode()


# ---- validation without a device -----------------------------------------------------------------
_REJECTED = [
    (dict(size_ms=0), "gap (size_ms) must be > 0"),
    (dict(size_ms=-5), "gap (size_ms) must be > 0"),
    (dict(size_ms=(1 << 40) + 1), "2^40"),
    (dict(allowed_lateness_ms=5), "allowed_lateness_ms"),
    (dict(allowed_lateness_ms=-1), "allowed_lateness_ms"),
    (dict(slide_ms=1), "slide_ms"),
    (dict(offset_ms=1), "offset_ms"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64)]), "n_aggs == 1"),
    (dict(aggs=[(abi.AGG_MINBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_MAXBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_AVG, 0, abi.T_I64)]), "not sum / min / max / count"),
    (dict(nullable_cols=[0]), "nullable_cols"),
    (dict(api=abi.API_SQL, key_hash=abi.KEYHASH_LONG), "DataStream"),
    (dict(ds_first_ordinals=True), "ds_first_ordinals"),
    (dict(shift_zone="Europe/Berlin"), "tz_n"),
    (dict(agg_phase=abi.PHASE_LOCAL), "agg_phase"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_BIGINT), "BINROW"),
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[m.split()[0] + str(i) for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_session_configs_fail_without_device(overrides, message):
    kw = dict(size_ms=3000)
    kw.update(overrides)
    cfg = _cfg(kw.pop("size_ms"), **kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    s, n, out = (C.c_int64 * 4)(), C.c_int32(0), C.c_int32()
    assert L.fw_host_session_add(C.byref(cfg), 0, 0, 1, s, s, s, C.byref(n), 4, C.byref(out)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_session_config_is_not_a_time_window_config():
    out = C.c_int64()
    assert _native.lib().fw_host_time_op(C.byref(_cfg(3000)), 3, 0, C.byref(out)) == abi.FW_E_INVALID
    assert "not for session windows" in _native.lib().fw_last_error().decode()


# ---- eligibility, assigner mirror --------------------------------------------------------------------
def test_eligibility_accepts_static_gap_sessions():
    a, t = EventTimeSessionWindows.with_gap(3000), EventTimeTrigger.create()
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("count", "LONG")]:
        assert is_gpu_eligible(a, t, agg) == (True, "")
    assert is_gpu_eligible(a, t, ("sum", "LONG"), allowed_lateness=0, evictor=None,
                           conf={"gpu.window-agg.enabled": "true"}) == (True, "")


def test_eligibility_refusals_give_reasons():
    a, t, sl = EventTimeSessionWindows.with_gap(3000), EventTimeTrigger.create(), ("sum", "LONG")

    class DynamicGap:   # EventTimeSessionWindows.withDynamicGap: not the mirror
        def is_event_time(self):
            return True
    cases = [
        (dict(allowed_lateness=1), "allowedLateness"),
        (dict(evictor=object()), "evictor"),
        (dict(trigger=CountTrigger.of(3)), "EventTimeTrigger"),
        (dict(aggregation=("minBy", "LONG")), "minBy"),
        (dict(aggregation=("maxBy", "LONG", True)), "minBy"),
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


def test_time_window_seam_still_refuses_sessions():
    from flink_amd.datastream import is_gpu_eligible as time_window_eligible
    ok, reason = time_window_eligible(EventTimeSessionWindows.with_gap(3000), EventTimeTrigger.create(), ("sum", "LONG"))
    assert not ok and "assigner" in reason


def test_assigner_mirror():
    a = EventTimeSessionWindows.with_gap(3000)
    assert a.assign_windows(17) == [(17, 3017)] and a.assign_windows(-5) == [(-5, 2995)]
    assert a.is_event_time() is True and a.gap == 3000
    for bad in (0, -1):
        with pytest.raises(ValueError):
            EventTimeSessionWindows.with_gap(bad)


# ---- ABI ------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_session_add") and "fw_host_session_add" in _native.EXPORTED
    assert abi.WIN_SESSION == 4
