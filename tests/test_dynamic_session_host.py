"""Dynamic-gap session windows (EventTimeSessionWindows.withDynamicGap) without a GPU: the library's
per-key session arithmetic with a gap per element (fw_host_session_add_gap, the routine the kernel's
exact path runs) against the element-by-element restatement, its equality with the static routine
under a constant gap, configuration validation before any device call, the eligibility seam, the
assigner mirror and the ABI."""
import ctypes as C

import numpy as np
import pytest
from dynamic_session_reference import GAP_MESSAGE, DynamicSessionReference
from session_window_reference import LONG_MIN

from flink_amd import _native, abi
from flink_amd.datastream import (CountTrigger, DynamicEventTimeSessionWindows, EventTimeSessionWindows, EventTimeTrigger)
from flink_amd.datastream.dynamic_session_window_operator import DynamicSessionWindowOperator, is_gpu_eligible

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}
GAPS = (1, 7, 50, 400)


def _cfg(max_gap=400, agg=abi.AGG_SUM, typ=abi.T_I64, **kw):
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_DYNAMIC, size_ms=max_gap, aggs=[(agg, 0, typ)],
             value_col_types=[typ, abi.T_I64], key_hash=abi.KEYHASH_LONG)
    d.update(kw)
    return abi.make_config(**d)


class HostSessions:
    """one key's session list in host arrays, driven only through fw_host_session_add_gap"""

    def __init__(self, cfg, capacity=256):
        self.cfg, self.cap = cfg, capacity
        self.s = (C.c_int64 * capacity)()
        self.e = (C.c_int64 * capacity)()
        self.a = (C.c_int64 * capacity)()
        self.n = C.c_int32(0)

    def add(self, watermark, ts, gap, v):
        out = C.c_int32(-7)
        _native.check(_native.lib().fw_host_session_add_gap(C.byref(self.cfg), watermark, ts, gap, v, self.s, self.e, self.a,
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


def _both(agg=("sum", "LONG"), max_gap=400):
    fn, ft = agg
    return HostSessions(_cfg(max_gap, _AGG[fn], _TYPE[ft])), DynamicSessionReference(agg)


def _add(h, r, ts, gap, v, key=7):
    got, want = h.add(r.watermark, ts, gap, v), r.add(key, ts, v, gap)
    assert got == want
    assert h.sessions() == r.windows.get(key, [])
    return got


# ---- explicit cases ---------------------------------------------------------------------------------
def test_window_nested_in_an_earlier_longer_one():
    h, r = _both(max_gap=1000)
    _add(h, r, 0, 1000, 1)             # [0, 1000)
    _add(h, r, 10, 1, 2)               # [10, 11): inside
    _add(h, r, 500, 1, 4)              # three rows later it is still the first row's window that covers
    assert h.sessions() == [[0, 1000, 7]]
    _add(h, r, 1000, 1, 8)             # [1000, 1001) touches
    _add(h, r, 1002, 1, 16)            # 1002 > 1001: apart
    assert h.sessions() == [[0, 1001, 15], [1002, 1003, 16]]


def test_late_test_uses_the_elements_own_gap():
    h, r = _both()
    r.process_watermark(109)
    assert not _add(h, r, 100, 10, 1)     # 100 + 10 - 1 == W: late, alone: dropped
    assert _add(h, r, 100, 11, 2)         # the same ts with a longer gap is not late
    assert _add(h, r, 100, 1, 4)          # late candidate [100, 101) inside the session: kept
    assert _add(h, r, 60, 40, 8)          # late candidate [60, 100) touches it: kept, moves the start back
    assert h.sessions() == [[60, 111, 14]] and r.late_dropped == 1


def test_one_long_window_bridges_many_sessions():
    h, r = _both()
    for i in range(5):
        _add(h, r, 100 * i, 1, 1 << i)
    assert h.n.value == 5
    _add(h, r, 50, 300, 1000)             # [50, 350): sessions at 100, 200, 300 -- and not 0 or 400
    assert h.sessions() == [[0, 1, 1], [50, 350, 1014], [400, 401, 16]]
    assert r.seen["bridge3"] == 1


# ---- fw_host_session_add_gap over a random stream ----------------------------------------------------
def _random_stream(seed, n=3000):
    """single-key elements (ts, gap, value) and watermarks, a few longest gaps wide so that nesting,
    touching and bridging are frequent; about a tenth of the elements lie behind the watermark"""
    rng = np.random.default_rng(seed)
    steps, base, wm = [], 0, LONG_MIN
    for i in range(n):
        ts = base + int(rng.integers(0, 900))
        if rng.random() < 0.1 and wm > LONG_MIN:
            ts = wm - int(rng.integers(0, 450))
        steps.append(("add", ts, int(GAPS[rng.integers(0, 4)]), int(rng.integers(-1000, 1000))))
        if i % 7 == 6:
            base += int(rng.integers(0, 1300))
            wm = max(wm, base - int(rng.integers(0, 500)))
            steps.append(("wm", wm))
    return steps


def _pick_seed():
    """the first seed whose stream makes the reference alone see every case at least once"""
    for seed in range(50):
        r = DynamicSessionReference()
        for st in _random_stream(seed):
            if st[0] == "add":
                r.add(7, st[1], st[3], st[2])
            else:
                r.process_watermark(st[1])
        if all(r.seen.values()):
            return seed
    raise AssertionError("no seed covers every case")


@pytest.mark.parametrize("agg", [("sum", "LONG"), ("min", "LONG"), ("max", "INT"), ("count", "LONG")])
def test_host_session_add_gap_equals_reference(agg):
    h, r = _both(agg)
    fired = 0
    for st in _random_stream(_pick_seed()):
        if st[0] == "add":
            _add(h, r, st[1], st[2], st[3])
        else:
            want = [[s, e, a] for _, a, s, e in r.process_watermark(st[1])]
            assert sorted(h.fire(st[1])) == sorted(want)
            fired += len(want)
            assert h.sessions() == r.windows.get(7, [])
    # the reference alone saw each case
    assert all(v >= 1 for v in r.seen.values()), r.seen
    assert fired > 100


@pytest.mark.parametrize("gap", [1, 50])
def test_constant_gap_equals_the_static_routine_bit_for_bit(gap):
    L = _native.lib()
    static = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=gap, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                             value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    dyn = HostSessions(_cfg(gap))
    s, e, a, n = (C.c_int64 * 256)(), (C.c_int64 * 256)(), (C.c_int64 * 256)(), C.c_int32(0)
    rng = np.random.default_rng(gap)
    wm, base = LONG_MIN, 0
    for i in range(2000):
        ts = base + int(rng.integers(0, 8 * gap + 2))
        if rng.random() < 0.1 and wm > LONG_MIN:
            ts = wm - int(rng.integers(0, 3 * gap + 1))
        v, out = int(rng.integers(-1000, 1000)), C.c_int32(-7)
        _native.check(L.fw_host_session_add(C.byref(static), wm, ts, v, s, e, a, C.byref(n), 256, C.byref(out)))
        assert dyn.add(wm, ts, gap, v) == bool(out.value)
        assert dyn.sessions() == [[s[j], e[j], a[j]] for j in range(n.value)]
        if i % 7 == 6:
            base += int(rng.integers(0, 12 * gap + 1))
            wm = max(wm, base - int(rng.integers(0, 2 * gap + 1)))
            keep = dyn.sessions()
            dyn.fire(wm)
            keep = [x for x in keep if x[1] - 1 > wm]
            for j, (ss, ee, aa) in enumerate(keep):
                s[j], e[j], a[j] = ss, ee, aa
            n.value = len(keep)


def test_host_session_add_gap_arguments():
    h = HostSessions(_cfg(400), capacity=2)
    L = _native.lib()
    out = C.c_int32()
    assert h.add(LONG_MIN, 0, 5, 1) and h.add(LONG_MIN, 100, 5, 1)
    args = (h.s, h.e, h.a, C.byref(h.n), 2, C.byref(out))
    assert L.fw_host_session_add_gap(C.byref(h.cfg), LONG_MIN, 200, 5, 1, *args) == abi.FW_E_CAPACITY
    assert h.add(LONG_MIN, 50, 50, 1) and h.sessions() == [[0, 5, 1], [50, 105, 2]]      # a merge still fits
    for bad in (0, -1, 401):
        assert L.fw_host_session_add_gap(C.byref(h.cfg), LONG_MIN, 0, bad, 1, *args) == abi.FW_E_INVALID
        assert "outside (0, size_ms" in L.fw_last_error().decode()
    static = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                             value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    assert L.fw_host_session_add_gap(C.byref(static), 0, 0, 5, 1, *args) == abi.FW_E_INVALID
    assert "FW_WIN_SESSION_DYNAMIC" in L.fw_last_error().decode()
    assert L.fw_host_session_add(C.byref(h.cfg), 0, 0, 1, h.s, h.e, h.a, C.byref(h.n), 2, C.byref(out)) == abi.FW_E_INVALID


# ---- validation without a device ---------------------------------------------------------------------
_REJECTED = [
    (dict(value_col_types=[abi.T_I64]), "n_value_cols == 2"),
    (dict(value_col_types=[abi.T_I64, abi.T_I64, abi.T_I64]), "n_value_cols == 2"),
    (dict(value_col_types=[abi.T_I64, abi.T_F64]), "gap column"),
    (dict(value_col_types=[abi.T_I64, abi.T_I32]), "gap column"),
    (dict(aggs=[(abi.AGG_SUM, 1, abi.T_I64)]), "column 1 is the gap"),
    (dict(size_ms=0), "gap (size_ms) must be > 0"),
    (dict(size_ms=-5), "gap (size_ms) must be > 0"),
    (dict(size_ms=(1 << 40) + 1), "2^40"),
    (dict(api=abi.API_SQL, key_hash=abi.KEYHASH_BINROW_BIGINT), "DataStream"),
    (dict(allowed_lateness_ms=5), "allowed_lateness_ms"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(nullable_cols=[0]), "nullable_cols"),
    (dict(nullable_cols=[1]), "nullable_cols"),
    (dict(aggs=[(abi.AGG_MINBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_AVG, 0, abi.T_I64)]), "not sum / min / max / count"),
    (dict(slide_ms=1), "slide_ms"),
    (dict(ds_first_ordinals=True), "ds_first_ordinals"),
    (dict(agg_phase=abi.PHASE_LOCAL), "agg_phase"),
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[m.split()[0] + str(i) for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_dynamic_session_configs_fail_without_device(overrides, message):
    kw = dict(overrides)
    cfg = _cfg(kw.pop("size_ms", 400), **kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    s, n, out = (C.c_int64 * 4)(), C.c_int32(0), C.c_int32()
    assert L.fw_host_session_add_gap(C.byref(cfg), 0, 0, 1, 1, s, s, s, C.byref(n), 4, C.byref(out)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_largest_gap_bound_is_accepted_by_the_plan():
    h = HostSessions(_cfg(1 << 40))
    assert h.add(LONG_MIN, 0, 1 << 40, 1) and h.sessions() == [[0, 1 << 40, 1]]
    assert HostSessions(_cfg(400, abi.AGG_COUNT_STAR)).add(LONG_MIN, 0, 400, 123)      # a count reads no column


def test_dynamic_config_is_not_a_time_window_config():
    out = C.c_int64()
    assert _native.lib().fw_host_time_op(C.byref(_cfg()), 3, 0, C.byref(out)) == abi.FW_E_INVALID
    assert "not for session windows" in _native.lib().fw_last_error().decode()


# ---- eligibility, assigner mirror ----------------------------------------------------------------------
def test_eligibility_accepts_dynamic_gap_sessions():
    a, t = EventTimeSessionWindows.with_dynamic_gap(lambda e: e[1]), EventTimeTrigger.create()
    assert isinstance(a, DynamicEventTimeSessionWindows)
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("count", "LONG")]:
        assert is_gpu_eligible(a, t, agg, max_gap=5000) == (True, "")
    assert is_gpu_eligible(a, t, ("sum", "LONG"), max_gap=1 << 40, conf={"gpu.window-agg.enabled": "true"}) == (True, "")


def test_eligibility_refusals_give_reasons():
    a, t, sl = DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 5), EventTimeTrigger.create(), ("sum", "LONG")
    cases = [
        (dict(assigner=EventTimeSessionWindows.with_gap(3000)), "DynamicEventTimeSessionWindows"),
        (dict(trigger=CountTrigger.of(3)), "EventTimeTrigger"),
        (dict(evictor=object()), "evictor"),
        (dict(allowed_lateness=1), "allowedLateness"),
        (dict(aggregation=("minBy", "LONG")), "minBy"),
        (dict(aggregation=("sum", "FLOAT")), "FLOAT"),
        (dict(max_gap=0), "max_gap"),
        (dict(max_gap=(1 << 40) + 1), "max_gap"),
    ]
    for kw, why in cases:
        args = dict(assigner=a, trigger=t, aggregation=sl)
        args.update(kw)
        ok, reason = is_gpu_eligible(args.pop("assigner"), args.pop("trigger"), args.pop("aggregation"), **args)
        assert not ok and why in reason, (why, reason)
    ok, reason = is_gpu_eligible(a, t, sl, conf={"gpu.window-agg.enabled": "false"})
    assert not ok and "gpu.window-agg.enabled" in reason
    with pytest.raises(ValueError, match="max_gap"):
        DynamicSessionWindowOperator(0)


def test_static_seam_still_refuses_dynamic_gaps():
    from flink_amd.datastream import is_session_window_gpu_eligible
    ok, reason = is_session_window_gpu_eligible(DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 5),
                                                EventTimeTrigger.create(), ("sum", "LONG"))
    assert not ok and "dynamic gaps" in reason


def test_assigner_mirror():
    a = DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: e[1])
    assert a.assign_windows(("k", 30), 17) == [(17, 47)] and a.assign_windows(("k", 1), -5) == [(-5, -4)]
    assert a.is_event_time() is True
    for bad in (0, -1):
        with pytest.raises(ValueError) as e:
            a.assign_windows(("k", bad), 0)
        assert str(e.value) == GAP_MESSAGE == "Dynamic session time gap must satisfy 0 < gap"
    r = DynamicSessionReference()
    with pytest.raises(ValueError, match=GAP_MESSAGE):
        r.add(1, 0, 1, 0)


# ---- ABI -------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_session_add_gap") and "fw_host_session_add_gap" in _native.EXPORTED
    assert abi.WIN_SESSION_DYNAMIC == 5 and abi.ERRF["GAP"] == 256
