"""Count windows (KeyedStream.countWindow) without a GPU: the reference restatement's hand vectors,
the library's count-slice arithmetic (fw_host_count_step, the code the kernel runs) against the
element-list reference, configuration validation before any device call, the eligibility seam
and the ABI."""
import ctypes as C
import math

import numpy as np
import pytest
from count_window_reference import CountWindowReference

from flink_amd import _native, abi
from flink_amd.datastream import (CountEvictor, CountTrigger, EventTimeTrigger, GlobalWindows, PurgingTrigger,
                                  TumblingEventTimeWindows)
from flink_amd.datastream.count_window_operator import is_gpu_eligible

PAIRS = [(250, 150), (3, 5), (5, 1), (6, 4), (4, 2), (1, 1), (7, 7), (16, 1)]


def _cfg(size, slide, agg=abi.AGG_SUM, typ=abi.T_I64, **kw):
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT, size_ms=size, slide_ms=slide, aggs=[(agg, 0, typ)],
             value_col_types=[typ], key_hash=abi.KEYHASH_LONG)
    d.update(kw)
    return abi.make_config(**d)


# ---- hand vectors ---------------------------------------------------------------------------
def test_reference_sliding_3_2_sum():
    r = CountWindowReference(3, 2, ("sum", "LONG")).process(["k"] * 7, range(1, 8))
    assert [(v, at) for _, v, _, _, at in r] == [(3, 1), (9, 3), (15, 5)]
    assert [(ws, we) for _, _, ws, we, _ in r] == [(0, 2), (1, 4), (3, 6)]


def test_reference_sliding_4_2_two_keys():
    keys = ["k2", "k2", "k2", "k1", "k1", "k1", "k1", "k2", "k2", "k2"]
    r = CountWindowReference(4, 2, ("sum", "LONG")).process(keys, [1] * 10)
    assert [(k, v, at) for k, v, _, _, at in r] == [("k2", 2, 1), ("k1", 2, 4), ("k1", 4, 6), ("k2", 4, 7), ("k2", 4, 9)]


def test_reference_tumbling_3_sum_drops_partial_window():
    ref = CountWindowReference(3, None, ("sum", "LONG"))
    r = ref.process(["k"] * 7, range(1, 8))
    assert [v for _, v, _, _, _ in r] == [6, 15]
    assert ref.process_watermark((1 << 63) - 1) == []   # nothing fires at end of input


def test_reference_size_equal_slide_is_the_purging_form():
    rng = np.random.default_rng(0)
    k, v = rng.integers(0, 3, 200).tolist(), rng.integers(-50, 50, 200).tolist()
    assert CountWindowReference(4, 4, ("max", "LONG")).process(k, v) == CountWindowReference(4, None, ("max", "LONG")).process(k, v)


def test_reference_java_reduce_rules():
    big = (1 << 31) - 1
    assert CountWindowReference(2, None, ("sum", "INT")).process([0, 0], [big, 1])[0][1] == -(1 << 31)
    nz, pz = np.float64(-0.0).view(np.int64).item(), 0
    assert CountWindowReference(2, None, ("min", "DOUBLE")).process([0, 0], [pz, nz])[0][1] == nz
    assert CountWindowReference(2, None, ("max", "DOUBLE")).process([0, 0], [pz, nz])[0][1] == pz
    nan = 0x7FF00000DEADBEEF
    assert CountWindowReference(2, None, ("max", "DOUBLE")).process([0, 0], [nan, np.float64(1e300).view(np.int64).item()])[0][1] == nan


# ---- fw_host_count_step against the reference ----------------------------------------------------
def _step(cfg, i):
    sl, rs, f, ws, ns = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    _native.check(_native.lib().fw_host_count_step(C.byref(cfg), i, C.byref(sl), C.byref(rs), C.byref(f), C.byref(ws),
                                                   C.byref(ns)))
    return sl.value, rs.value, f.value, ws.value, ns.value


_OPS = {"sum": lambda a, b: a + b, "min": min, "max": max}


@pytest.mark.parametrize("size,slide", PAIRS)
@pytest.mark.parametrize("fn", ["sum", "min", "max"])
def test_host_count_step_ring_equals_reference(size, slide, fn):
    """A ring of size / gcd slots driven only by the function's outputs reproduces every fire of the
    evicting operator: which elements fire, the aggregate, and the window's bounds."""
    cfg = _cfg(size, slide, {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX}[fn])
    R = size // math.gcd(size, slide)
    vals = np.random.default_rng(size * 31 + slide).integers(-1000, 1000, 2000).tolist()
    want = CountWindowReference(size, slide, (fn, "LONG")).process([7] * 2000, vals)
    ring, last_slice, got = [None] * R, -1, []
    for i, v in enumerate(vals):
        sl, rs, fires, ws, ns = _step(cfg, i)
        assert 0 <= rs < R
        if sl != last_slice:   # the slice's first element resets its slot
            ring[rs], last_slice = None, sl
        ring[rs] = v if ring[rs] is None else _OPS[fn](ring[rs], v)
        if fires:
            assert 1 <= ns <= R
            acc = None
            for k in range(ns - 1, -1, -1):   # oldest slice first
                part = ring[(rs - k) % R]
                acc = part if acc is None else _OPS[fn](acc, part)
            got.append((7, acc, ws, i + 1, i))
    assert got == want and len(want) == 2000 // slide


def test_host_count_step_tumbling_form_slide_zero():
    assert [_step(_cfg(3, 0), i) for i in range(6)] == [_step(_cfg(3, 3), i) for i in range(6)]
    assert _step(_cfg(3, 0), 2) == (0, 0, 1, 0, 1) and _step(_cfg(3, 0), 5) == (1, 0, 1, 3, 1)


# ---- validation without a device -----------------------------------------------------------------
_REJECTED = [
    (dict(api=abi.API_SQL, key_hash=abi.KEYHASH_LONG), "DataStream"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64)]), "n_aggs == 1"),
    (dict(aggs=[(abi.AGG_MINBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_MAXBY, 0, abi.T_I64)]), "minBy / maxBy"),
    (dict(aggs=[(abi.AGG_AVG, 0, abi.T_I64)]), "not sum / min / max / count"),
    (dict(aggs=[(abi.AGG_COUNT, 0, abi.T_I64)]), "not sum / min / max / count"),
    (dict(size_ms=0), "size must be >= 1"),
    (dict(slide_ms=-1), "slide must be >= 1"),
    (dict(size_ms=17, slide_ms=1), "FW_COUNT_MAX_SLICES"),
    (dict(size_ms=251, slide_ms=150), "FW_COUNT_MAX_SLICES"),
    (dict(offset_ms=1), "offset_ms"),
    (dict(allowed_lateness_ms=5), "allowed_lateness_ms"),
    (dict(late_side_output=True), "late_side_output"),
    (dict(ds_first_ordinals=True), "ds_first_ordinals"),
    (dict(nullable_cols=[0]), "nullable_cols"),
    (dict(shift_zone="Europe/Berlin"), "tz_n"),
    (dict(agg_phase=abi.PHASE_LOCAL), "agg_phase"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_BIGINT), "BINROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_INT), "BINROW"),
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[m + str(i) for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_count_configs_fail_without_device(overrides, message):
    kw = dict(size_ms=4, slide_ms=2)
    kw.update(overrides)
    cfg = _cfg(kw.pop("size_ms"), kw.pop("slide_ms"), **kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    out = [C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()]
    assert L.fw_host_count_step(C.byref(cfg), 0, *[C.byref(o) for o in out]) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_count_config_is_not_a_time_window_config():
    out = C.c_int64()
    assert _native.lib().fw_host_time_op(C.byref(_cfg(4, 2)), 3, 0, C.byref(out)) == abi.FW_E_INVALID
    assert "not for count windows" in _native.lib().fw_last_error().decode()


# ---- eligibility ------------------------------------------------------------------------------
def test_eligibility_accepts_the_two_count_window_shapes():
    gw = GlobalWindows.create()
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("count", "LONG")]:
        assert is_gpu_eligible(gw, PurgingTrigger.of(CountTrigger.of(250)), agg) == (True, "")
        assert is_gpu_eligible(gw, CountTrigger.of(150), agg, evictor=CountEvictor.of(250)) == (True, "")
    assert is_gpu_eligible(gw, CountTrigger.of(5), ("sum", "LONG"), evictor=CountEvictor.of(3)) == (True, "")


def test_eligibility_refusals_give_reasons():
    gw, sl = GlobalWindows.create(), ("sum", "LONG")
    cases = [
        (TumblingEventTimeWindows.of(1000), PurgingTrigger.of(CountTrigger.of(3)), sl, None, "GlobalWindows"),
        (gw, CountTrigger.of(3), sl, None, "without CountEvictor"),
        (gw, EventTimeTrigger.create(), sl, CountEvictor.of(3), "other than CountTrigger"),
        (gw, PurgingTrigger.of(CountTrigger.of(3)), sl, CountEvictor.of(3), "other than CountTrigger"),
        (gw, EventTimeTrigger.create(), sl, None, "PurgingTrigger"),
        (gw, CountTrigger.of(2), sl, object(), "not CountEvictor"),
        (gw, CountTrigger.of(2), sl, CountEvictor.of(3, True), "doEvictAfter"),
        (gw, CountTrigger.of(2), ("minBy", "LONG"), CountEvictor.of(3), "minBy"),
        (gw, CountTrigger.of(2), ("minBy", "LONG", True), CountEvictor.of(3), "minBy"),
        (gw, CountTrigger.of(2), ("sum", "FLOAT"), CountEvictor.of(3), "FLOAT"),
        (gw, CountTrigger.of(1), sl, CountEvictor.of(17), "count slices"),
        (gw, CountTrigger.of(0), sl, CountEvictor.of(3), ">= 1"),
    ]
    for assigner, trigger, agg, evictor, why in cases:
        ok, reason = is_gpu_eligible(assigner, trigger, agg, evictor=evictor)
        assert not ok and why in reason, (why, reason)
    ok, reason = is_gpu_eligible(gw, CountTrigger.of(2), sl, evictor=CountEvictor.of(4), conf={"gpu.window-agg.enabled": "false"})
    assert not ok and "gpu.window-agg.enabled" in reason


# ---- ABI ------------------------------------------------------------------------------------
def test_abi_version_and_symbol():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_count_step") and "fw_host_count_step" in _native.EXPORTED
    assert abi.WIN_COUNT == 3 and abi.FW_COUNT_MAX_SLICES == 16
