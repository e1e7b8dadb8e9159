"""Record-shaped count windows (FW_WIN_COUNT_RECORD) without a GPU: the reference restatement's hand
vectors, the library's pair fold (fw_host_count_record_fold, the code the kernel runs) against the
reference's reduce, configuration validation before any device call, the eligibility seam and the
ABI."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
from count_record_reference import CountRecordReference, bits_of, double_of, record_image, reduce_records

from flink_amd import _native, abi
from flink_amd.datastream import (CountEvictor, CountTrigger, EventTimeTrigger, GlobalWindows, PurgingTrigger,
                                  TumblingEventTimeWindows)
from flink_amd.datastream.record_count_window_operator import is_gpu_eligible

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "minBy": abi.AGG_MINBY, "maxBy": abi.AGG_MAXBY}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}
# (fn, first): the five aggregates, minBy / maxBy under both tie rules
_FNS = [("sum", True), ("min", True), ("max", True), ("minBy", True), ("minBy", False), ("maxBy", True), ("maxBy", False)]


def _cfg(size=4, slide=2, fn="sum", ftype="LONG", first=True, kind=None, **kw):
    t = _TYPE[ftype]
    flags = abi.AGGF_LAST if fn in ("minBy", "maxBy") and not first else 0
    d = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT_RECORD if kind is None else kind, size_ms=size, slide_ms=slide,
             aggs=[(_AGG[fn], 0, t, flags)], value_col_types=[t], key_hash=abi.KEYHASH_LONG, ds_first_ordinals=True)
    d.update(kw)
    return abi.make_config(**d)


def _fold(cfg, av, ao, bv, bo):
    ov, oo = C.c_int64(), C.c_int64()
    _native.check(_native.lib().fw_host_count_record_fold(C.byref(cfg), av, ao, bv, bo, C.byref(ov), C.byref(oo)))
    return ov.value, oo.value


# ---- the reference's hand vectors ------------------------------------------------------------------
def test_reference_sum_emits_oldest_element_with_field_set():
    recs = [("k", i, f"tag{i}") for i in range(1, 8)]
    r = CountRecordReference(3, 2, ("sum", "LONG"), field=1).process(["k"] * 7, recs, range(7))
    assert [(rec, at, ro) for _, rec, at, ro in r] == [(("k", 3, "tag1"), 1, 0), (("k", 9, "tag2"), 3, 1), (("k", 15, "tag4"), 5, 3)]


def test_reference_min_keeps_value1_fields_and_takes_newer_on_ties():
    n1, n2 = double_of(0x7FF8000000000001), double_of(0x7FF00000DEADBEEF)
    recs = [("k", n1, "a"), ("k", n2, "b")]
    (_, rec, _, ro), = CountRecordReference(2, None, ("max", "DOUBLE"), field=1).process(["k"] * 2, recs, [10, 11])
    assert record_image(rec) == ("k", ("f64", 0x7FF00000DEADBEEF), "a") and ro == 10
    recs = [("k", 0.0, "a"), ("k", -0.0, "b"), ("k", 0.0, "c")]
    (_, rec, _, _), = CountRecordReference(3, None, ("min", "DOUBLE"), field=1).process(["k"] * 3, recs, range(3))
    assert record_image(rec) == ("k", ("f64", bits_of(-0.0)), "a")


def test_reference_min_by_tie_rules():
    recs = [("k", 2, "a"), ("k", 1, "b"), ("k", 1, "c"), ("k", 3, "d")]
    for first, want, ro in [(True, "b", 1), (False, "c", 2)]:
        (_, rec, at, o), = CountRecordReference(4, None, ("minBy", "LONG", first), field=1).process(["k"] * 4, recs, range(4))
        assert rec[2] == want and o == ro and at == 3
    (_, rec, _, o), = CountRecordReference(4, None, ("maxBy", "LONG", False), field=1).process(["k"] * 4, recs, range(4))
    assert rec == ("k", 3, "d") and o == 3


def test_reference_held_ordinals():
    ref = CountRecordReference(4, 2, ("sum", "LONG"), field=1)   # g = 2, R = 2
    ref.process(["k"] * 5, [("k", i) for i in range(5)], range(100, 105))
    assert ref.held() == {102, 104}    # slices 1 and 2: their first elements
    by = CountRecordReference(4, 2, ("maxBy", "LONG", False), field=1)
    by.process(["k"] * 5, [("k", v) for v in (5, 5, 1, 7, 0)], range(100, 105))
    assert by.held() == {103, 104}


# ---- fw_host_count_record_fold against the reference's reduce -------------------------------------
_INTS = {"LONG": [0, 1, -1, 7, 7, (1 << 63) - 1, -(1 << 63), 12345],
         "INT": [0, 1, -1, 7, 7, (1 << 31) - 1, -(1 << 31), 12345]}
_DBL_BITS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF00000DEADBEEF, 0x8000000000000000, 0,
             bits_of(1.0), bits_of(1.0), bits_of(-1.0), bits_of(float("inf")), bits_of(float("-inf")), bits_of(1e300), bits_of(5e-324)]


def _values(ftype):
    """field values as the device words (int64) and as the record's Python values"""
    if ftype == "DOUBLE":
        words = [bits_of(double_of(b)) for b in _DBL_BITS]   # as signed 64-bit words
        return words, [double_of(w) for w in words]
    return _INTS[ftype], _INTS[ftype]


def _want(fn, ftype, first, a, ao, b, bo):
    """the reference's reduce on two one-element records, as (result word, ordinal)"""
    rec = reduce_records(fn, ftype, first, 1, ("k", a, ao), ("k", b, bo))
    v = rec[1]
    word = bits_of(v) if ftype == "DOUBLE" else v
    return word, (rec[2] if fn in ("minBy", "maxBy") else ao)


@pytest.mark.parametrize("ftype", ["LONG", "INT", "DOUBLE"])
@pytest.mark.parametrize("fn,first", _FNS)
def test_pair_fold_equals_the_reference_reduce(fn, first, ftype):
    """every ordered pair of the value set: equal values, NaN against NaN (different payloads) and
    against numbers, -0.0 against 0.0, the extremes; bit for bit, ordinal included"""
    cfg = _cfg(fn=fn, ftype=ftype, first=first)
    words, vals = _values(ftype)
    for (i, (wa, va)), (j, (wb, vb)) in itertools.product(enumerate(zip(words, vals)), repeat=2):
        assert _fold(cfg, wa, 100 + i, wb, 200 + j) == _want(fn, ftype, first, va, 100 + i, vb, 200 + j), (va, vb)


@pytest.mark.parametrize("ftype", ["LONG", "INT", "DOUBLE"])
@pytest.mark.parametrize("fn,first", _FNS)
def test_pair_fold_is_associative(fn, first, ftype):
    cfg = _cfg(fn=fn, ftype=ftype, first=first)
    words, _ = _values(ftype)
    if fn == "sum" and ftype == "DOUBLE":   # DOUBLE addition is associative only where it is exact: small integers
        words = [bits_of(float(x)) for x in range(-4, 5)]
    rng = np.random.default_rng(len(fn) * 7 + len(ftype) + first)
    for _ in range(300):
        (a, b, c) = [(words[i], 1000 + n * 50 + int(i)) for n, i in enumerate(rng.integers(0, len(words), 3))]
        left = _fold(cfg, *_fold(cfg, *a, *b), *c)
        right = _fold(cfg, *a, *_fold(cfg, *b, *c))
        assert left == right, (a, b, c)


@pytest.mark.parametrize("ftype", ["LONG", "INT", "DOUBLE"])
@pytest.mark.parametrize("fn,first", _FNS)
def test_run_folded_as_slices_equals_the_sequential_reduce(fn, first, ftype):
    """a run of elements cut into slices, each folded on its own and the slice results folded oldest
    first -- the kernel's shape -- against the reference's element-by-element reduce"""
    cfg = _cfg(fn=fn, ftype=ftype, first=first)
    rng = np.random.default_rng(11 + len(fn) + len(ftype))
    words, vals = _values(ftype)
    if fn == "sum" and ftype == "DOUBLE":   # exact sums only: small integers as doubles
        vals = [float(x) for x in range(-4, 5)]
        words = [bits_of(x) for x in vals]
    for g in (1, 3, 50):
        pick = rng.integers(0, len(words), 4 * g + g // 2 + 1)
        elems = [(words[i], 5000 + n) for n, i in enumerate(pick)]
        recs = [("k", vals[i], 5000 + n) for n, i in enumerate(pick)]
        want = recs[0]
        for r in recs[1:]:
            want = reduce_records(fn, ftype, first, 1, want, r)
        parts = []
        for s in range(0, len(elems), g):
            cur = elems[s]
            for e in elems[s + 1:s + g]:
                cur = _fold(cfg, *cur, *e)
            parts.append(cur)
        acc = parts[0]
        for p in parts[1:]:
            acc = _fold(cfg, *acc, *p)
        wv = bits_of(want[1]) if ftype == "DOUBLE" else want[1]
        assert acc == (wv, want[2] if fn in ("minBy", "maxBy") else recs[0][2])


def test_pair_fold_refuses_other_kinds():
    ov, oo = C.c_int64(), C.c_int64()
    L = _native.lib()
    cfg = _cfg(kind=abi.WIN_COUNT, ds_first_ordinals=False)
    assert L.fw_host_count_record_fold(C.byref(cfg), 1, 2, 3, 4, C.byref(ov), C.byref(oo)) == abi.FW_E_INVALID
    assert "FW_WIN_COUNT_RECORD" in L.fw_last_error().decode()
    cfg = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_TUMBLE, size_ms=1000, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                          value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    assert L.fw_host_count_record_fold(C.byref(cfg), 1, 2, 3, 4, C.byref(ov), C.byref(oo)) == abi.FW_E_INVALID


def test_count_step_accepts_the_record_kind():
    out = lambda: [C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()]
    L = _native.lib()
    for i in range(40):
        a, b = out(), out()
        _native.check(L.fw_host_count_step(C.byref(_cfg(6, 4)), i, *[C.byref(o) for o in a]))
        _native.check(L.fw_host_count_step(C.byref(_cfg(6, 4, kind=abi.WIN_COUNT, ds_first_ordinals=False)), i, *[C.byref(o) for o in b]))
        assert [o.value for o in a] == [o.value for o in b]


# ---- validation without a device ----------------------------------------------------------------
_REJECTED = [
    # the record kind's own
    (dict(aggs=[(abi.AGG_COUNT_STAR, 0, abi.T_I64)]), "FW_AGG_COUNT_STAR"),
    (dict(ds_first_ordinals=False), "ds_first_ordinals must be 1"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_I64, abi.AGGF_LAST)]), "FW_AGGF_LAST"),
    (dict(aggs=[(abi.AGG_MIN, 0, abi.T_I64, abi.AGGF_LAST)]), "FW_AGGF_LAST"),
    (dict(aggs=[(abi.AGG_MINBY, 0, abi.T_I64, 2)]), "aggs[0].flags"),
    (dict(size_ms=17, slide_ms=1), "FW_COUNT_MAX_SLICES"),
    (dict(size_ms=251, slide_ms=150), "FW_COUNT_MAX_SLICES"),
    # FW_WIN_COUNT's, carried over
    (dict(api=abi.API_SQL), "DataStream"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_I64), (abi.AGG_MAX, 0, abi.T_I64)]), "n_aggs == 1"),
    (dict(aggs=[(abi.AGG_AVG, 0, abi.T_I64)]), "aggs[0].kind"),
    (dict(aggs=[(abi.AGG_COUNT, 0, abi.T_I64)]), "aggs[0].kind"),
    (dict(aggs=[(abi.AGG_SUM, 0, 7)], value_col_types=[7]), "bad aggregate type"),
    (dict(aggs=[(abi.AGG_SUM, 1, abi.T_I64)]), "input_col"),
    (dict(aggs=[(abi.AGG_SUM, 0, abi.T_F64)]), "value column type"),
    (dict(size_ms=0), "size must be >= 1"),
    (dict(slide_ms=-1), "slide must be >= 1"),
    (dict(offset_ms=1), "offset_ms"),
    (dict(allowed_lateness_ms=5), "allowed_lateness_ms"),
    (dict(late_side_output=True), "late_side_output"),
    (dict(nullable_cols=[0]), "nullable_cols"),
    (dict(shift_zone="Europe/Berlin"), "tz_n"),
    (dict(agg_phase=abi.PHASE_LOCAL), "agg_phase"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_BIGINT), "BINROW"),
    (dict(key_hash=abi.KEYHASH_BINROW_INT), "BINROW"),
    (dict(max_batch_rows=0), "max_batch_rows"),
    (dict(output_capacity=0), "output_capacity"),
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[f"{i}-{m}" for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_record_count_configs_fail_without_device(overrides, message):
    kw = dict(size=4, slide=2)
    kw.update({{"size_ms": "size", "slide_ms": "slide"}.get(k, k): v for k, v in overrides.items()})
    cfg = _cfg(**kw)
    h = C.c_void_p()
    L = _native.lib()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    ov, oo = C.c_int64(), C.c_int64()
    assert L.fw_host_count_record_fold(C.byref(cfg), 1, 2, 3, 4, C.byref(ov), C.byref(oo)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_valid_record_configs_plan_without_device():
    for (fn, first), ftype in itertools.product(_FNS, _TYPE):
        for size, slide in [(3, 0), (3, 1), (250, 150), (16, 1)]:
            assert _fold(_cfg(size, slide, fn, ftype, first), 1, 10, 1, 11)[1] in (10, 11)


# ---- eligibility -------------------------------------------------------------------------------
def test_eligibility_accepts_record_shapes():
    gw = GlobalWindows.create()
    for agg in [("sum", "LONG"), ("min", "INT"), ("max", "DOUBLE"), ("minBy", "LONG"), ("maxBy", "DOUBLE", True),
                ("minBy", "INT", False)]:
        assert is_gpu_eligible(gw, PurgingTrigger.of(CountTrigger.of(250)), agg, field=2) == (True, "")
        assert is_gpu_eligible(gw, CountTrigger.of(150), agg, evictor=CountEvictor.of(250), field=0) == (True, "")


def test_eligibility_refusals_give_reasons():
    gw, sl = GlobalWindows.create(), ("sum", "LONG")
    cases = [
        (TumblingEventTimeWindows.of(1000), PurgingTrigger.of(CountTrigger.of(3)), sl, None, 1, "GlobalWindows"),
        (gw, CountTrigger.of(3), sl, None, 1, "without CountEvictor"),
        (gw, EventTimeTrigger.create(), sl, CountEvictor.of(3), 1, "other than CountTrigger"),
        (gw, CountTrigger.of(2), sl, CountEvictor.of(3, True), 1, "doEvictAfter"),
        (gw, CountTrigger.of(2), ("count", "LONG"), CountEvictor.of(3), 1, "no record-shaped form"),
        (gw, CountTrigger.of(2), ("sum", "LONG", True), CountEvictor.of(3), 1, "tie rule"),
        (gw, CountTrigger.of(2), ("minBy", "LONG", 1), CountEvictor.of(3), 1, "tie rule"),
        (gw, CountTrigger.of(2), ("sum", "FLOAT"), CountEvictor.of(3), 1, "FLOAT"),
        (gw, CountTrigger.of(2), sl, CountEvictor.of(3), None, "field="),
        (gw, CountTrigger.of(2), sl, CountEvictor.of(3), -1, "field="),
        (gw, CountTrigger.of(1), sl, CountEvictor.of(17), 1, "count slices"),
        (gw, CountTrigger.of(0), sl, CountEvictor.of(3), 1, ">= 1"),
    ]
    for assigner, trigger, agg, evictor, field, why in cases:
        ok, reason = is_gpu_eligible(assigner, trigger, agg, evictor=evictor, field=field)
        assert not ok and why in reason, (why, reason)
    ok, reason = is_gpu_eligible(gw, CountTrigger.of(2), sl, evictor=CountEvictor.of(4), field=1,
                                 conf={"gpu.window-agg.enabled": "false"})
    assert not ok and "gpu.window-agg.enabled" in reason


# ---- ABI ------------------------------------------------------------------------------------------
def test_abi_and_symbol():
    L = _native.lib()
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
    assert hasattr(L, "fw_host_count_record_fold") and "fw_host_count_record_fold" in _native.EXPORTED
    assert abi.WIN_COUNT_RECORD == 8 and abi.WIN_COUNT == 3
    assert abi.result_columns(_cfg()) == 2 and math.gcd(250, 150) == 50
