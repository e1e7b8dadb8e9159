"""Record-shaped count windows (FW_WIN_COUNT_RECORD, RecordCountWindowOperator) on the GPU against the
element-list reference (count_record_reference.py): the output records in emission order, record for
record, the ordinal of the triggering element and of the element each output is built from, and --
after every batch -- the set of records the operator holds.

Everything compares bit for bit (floats by their bits, a NaN with its payload) except DOUBLE sums,
which compare at 1e-9 relative, the project's DOUBLE-sum rule: the device adds count-slice partials,
the reference adds left to right, and <= 250 addends in [0, 1000) differ by about 250 * 2^-53.
A record is (key, field, serial, weight): two fields besides the key and the aggregated one, the
weight a float that is sometimes a NaN with a payload.  Shapes sit at the fold's edges: a tile holds
1024 rows, so 3000 rows of one key split slices between tiles, most of their slices come and go inside
the push, and -- cut into pushes of 1, 7 and 1025 rows -- a slice continues across pushes and tiles."""
import ctypes as C

import numpy as np
import pytest
from count_record_reference import CountRecordReference, bits_of, double_of, record_image
from count_window_reference import CountWindowReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

SHAPES = [(3, None), (3, 1), (250, 150), (16, 1)]   # R = 1 purging; g = 1; CFG1 (g = 50, R = 5); R = FW_COUNT_MAX_SLICES
_NAN_WEIGHT = double_of(0x7FF80000000ABCDE)
_SPECIAL = [0x7FF8000000000000, 0xFFF8000000000001 - (1 << 64), 0x7FF00000DEADBEEF, -(1 << 63), 0, bits_of(1.0), bits_of(-1.0),
            bits_of(float("inf")), bits_of(float("-inf")), bits_of(2.5)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(size, slide, agg, **kw):
    from flink_amd.datastream import RecordCountWindowOperator
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return RecordCountWindowOperator(size, slide, agg, field=1, **kw).open()


def _batch(keys, words, ftype, serial0):
    """(keys, the field's column, records) of one batch; ``words``: the field as int64 device words"""
    words = np.asarray(words, np.int64)
    if ftype == "DOUBLE":
        col, fld = words.view(np.float64), [double_of(w) for w in words.tolist()]
    else:
        col, fld = words, words.tolist()
    ks = keys.tolist() if isinstance(keys, np.ndarray) else list(keys)
    recs = [(k, f, serial0 + i, _NAN_WEIGHT if (serial0 + i) % 5 == 0 else (serial0 + i) * 0.5) for i, (k, f) in enumerate(zip(ks, fld))]
    return keys, col, recs


def _drive(op, ref, batches, got, want):
    """pushes the batches; after each, the operator holds exactly the reference's set of records"""
    for keys, col, recs in batches:
        seq = op.handle.push_seq
        op.process_batch(keys, col, recs)
        assert op.handle.push_seq == seq + 1
        out = op.collect()
        got += list(zip(out["key"], out["records"], out["trigger_ord"].tolist(), out["record_ord"].tolist()))
        ks = keys.tolist() if isinstance(keys, np.ndarray) else list(keys)
        want += ref.process(ks, recs, [(seq << 32) | i for i in range(len(recs))])
        assert op.retained_ordinals() == ref.held()
        assert np.all(out["timestamp"] == (1 << 63) - 1)


def _compare(got, want, agg):
    assert len(got) == len(want)
    if agg[:2] == ("sum", "DOUBLE"):
        cut = lambda rows: [(k, record_image(r[:1] + r[2:]), t, o) for k, r, t, o in rows]
        assert cut(got) == cut(want)
        np.testing.assert_allclose([r[1] for _, r, _, _ in got], [r[1] for _, r, _, _ in want], rtol=1e-9, atol=0)
    else:
        img = lambda rows: [(k, record_image(r), t, o) for k, r, t, o in rows]
        assert img(got) == img(want)


def _run(size, slide, agg, batches, **kw):
    op, ref = _op(size, slide, agg, **kw), CountRecordReference(size, slide, agg, field=1)
    got, want = [], []
    try:
        _drive(op, ref, batches, got, want)
        _compare(got, want, agg)
        st = op.handle.stats()
        assert st["error_flags"] == 0 and st["num_fired_windows"] == len(want) and st["pending_rows"] == 0
    finally:
        op.close()
    return want


def _cut(keys, words, ftype, per):
    return [_batch(keys[o:o + per], words[o:o + per], ftype, o) for o in range(0, len(keys), per)]


# ---- one key: tiles split slices, most slices are transient ---------------------------------------
_HOT_N = 3000
_HOT = np.random.default_rng(5).integers(-3, 4, _HOT_N).astype(np.int64)   # a small range: ties everywhere
_HOT_AGGS = [("sum", "LONG"), ("min", "LONG"), ("minBy", "LONG", True), ("maxBy", "LONG", False)]


@pytest.mark.parametrize("size,slide", SHAPES)
@pytest.mark.parametrize("agg", _HOT_AGGS, ids=lambda a: "-".join(map(str, a)))
def test_hot_key_one_push(size, slide, agg):
    """3000 rows of one key in one push: results name elements that were never retained"""
    want = _run(size, slide, agg, _cut(np.full(_HOT_N, 42, np.int64), _HOT, "LONG", _HOT_N))
    assert len(want) == _HOT_N // (slide or size)


@pytest.mark.parametrize("size,slide", SHAPES)
@pytest.mark.parametrize("agg", [("sum", "LONG"), ("minBy", "LONG", False)], ids=lambda a: "-".join(map(str, a)))
@pytest.mark.parametrize("per", [1, 7, 1025])
def test_hot_key_split_pushes(size, slide, agg, per):
    """the same stream in pushes of 1, 7 and 1025 rows: a slice begun in one push (or tile) continues in
    the next against the table"""
    _run(size, slide, agg, _cut(np.full(_HOT_N, 42, np.int64), _HOT, "LONG", per))


# ---- many keys and a hot one, values from {0, 1, 2} --------------------------------------------------
def _tie_stream(n, seed):
    rng = np.random.default_rng(seed)
    keys = np.where(rng.random(n) < 0.4, 7, rng.integers(100, 160, n) * 977).astype(np.int64)
    return keys, rng.integers(0, 3, n).astype(np.int64)


_TIE_AGGS = [("minBy", "LONG", True), ("minBy", "LONG", False), ("maxBy", "LONG", True), ("maxBy", "LONG", False),
             ("min", "LONG"), ("max", "LONG"), ("sum", "LONG")]


@pytest.mark.parametrize("size,slide,n", [(250, 150, 30000), (3, 1, 4000)])
@pytest.mark.parametrize("agg", _TIE_AGGS, ids=lambda a: "-".join(map(str, a)))
def test_many_keys_with_ties(size, slide, n, agg):
    keys, words = _tie_stream(n, size)
    want = _run(size, slide, agg, _cut(keys, words, "LONG", n // 4))
    assert len({k for k, _, _, _ in want}) == 61   # every key fired


# ---- DOUBLE fields -----------------------------------------------------------------------------
@pytest.mark.parametrize("agg", [("min", "DOUBLE"), ("max", "DOUBLE"), ("minBy", "DOUBLE", False), ("maxBy", "DOUBLE", True)],
                         ids=lambda a: "-".join(map(str, a)))
@pytest.mark.parametrize("size,slide", [(16, 1), (250, 150)])
def test_double_nan_zero_infinity(size, slide, agg):
    rng = np.random.default_rng(17)
    n = 2400
    words = np.array(_SPECIAL, np.int64)[rng.integers(0, len(_SPECIAL), n)]
    keys = rng.integers(0, 3, n).astype(np.int64)
    _run(size, slide, agg, _cut(keys, words, "DOUBLE", 800))


@pytest.mark.parametrize("size,slide", [(250, 150), (3, 1)])
def test_double_sums(size, slide):
    rng = np.random.default_rng(19)
    n = 2400
    words = (rng.random(n) * 1000).view(np.int64)
    _run(size, slide, ("sum", "DOUBLE"), _cut(rng.integers(0, 3, n).astype(np.int64), words, "DOUBLE", 800))


# ---- INT sums wrap -------------------------------------------------------------------------------
@pytest.mark.parametrize("size,slide", [(3, None), (250, 150)])
def test_int_sums_wrap(size, slide):
    rng = np.random.default_rng(23)
    n = 2400
    words = rng.integers((1 << 31) - 1000, 1 << 31, n).astype(np.int64)
    want = _run(size, slide, ("sum", "INT"), _cut(rng.integers(0, 3, n).astype(np.int64), words, "INT", 800))
    # every window adds at least three values just below 2^31: an INT result means the sum wrapped
    assert want and all(-(1 << 31) <= r[1] < (1 << 31) for _, r, _, _ in want)


# ---- STRING keys ---------------------------------------------------------------------------------
def test_string_keys():
    rng = np.random.default_rng(29)
    n = 1500
    keys = [f"user-{i}" for i in rng.integers(0, 20, n)]
    want = _run(3, 1, ("maxBy", "LONG", True), _cut(keys, rng.integers(0, 3, n).astype(np.int64), "LONG", 500), key_type="STRING")
    assert all(isinstance(k, str) for k, _, _, _ in want)


# ---- a subtask of parallelism 2 --------------------------------------------------------------------
def _dest(keys, p):
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_LONG, 128, p, None, d.ctypes.data))
    return d


def test_parallelism_two_own_key_groups_and_a_foreign_key():
    keys, words = _tie_stream(6000, 31)
    d = _dest(keys, 2)
    agg = ("minBy", "LONG", True)
    for i in range(2):
        _run(250, 150, agg, _cut(keys[d == i], words[d == i], "LONG", 2000), parallelism=2, subtask_index=i)
    op = _op(250, 150, agg, parallelism=2, subtask_index=0)
    try:
        stray = keys[d == 1][:1]
        op.handle.push_host(stray, np.zeros(1, np.int64), [np.ones(1, np.int64)])
        assert op.handle.stats()["error_flags"] & abi.ERRF["KEYGROUP"]
    finally:
        op.close()


# ---- checkpoint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg,key_type", [(("sum", "LONG"), "LONG"), (("maxBy", "LONG", False), "LONG"), (("minBy", "LONG", True), "STRING")],
                         ids=["sum", "maxBy-last", "minBy-first-string"])
def test_snapshot_mid_slice_and_restore(agg, key_type):
    keys, words = _tie_stream(9000, 37)
    if key_type == "STRING":
        keys = [f"k{k}" for k in keys.tolist()]
    batches = _cut(keys, words, "LONG", 1777)   # 1777 rows: the hot key stands in the middle of a slice
    ref = CountRecordReference(250, 150, agg, field=1)
    a, b = _op(250, 150, agg, key_type=key_type), None
    got, want = [], []
    try:
        _drive(a, ref, batches[:3], got, want)
        assert a.retained_ordinals() and any(len(v) % 50 for v in ref.elements.values())
        blob = a.snapshot_state()
        a.close()
        b = _op(250, 150, agg, key_type=key_type)
        b.initialize_state(blob)
        assert b.retained_ordinals() == ref.held() and b.handle.push_seq == 3
        _drive(b, ref, batches[3:], got, want)
        _compare(got, want, agg)
        assert b.handle.stats()["error_flags"] == 0
    finally:
        a.close()
        if b is not None:
            b.close()


def test_blobs_do_not_cross_tie_rules_or_kinds():
    from flink_amd.datastream import CountWindowOperator
    keys = np.full(120, 9, np.int64)
    ops = {"first": _op(4, 2, ("minBy", "LONG", True)), "last": _op(4, 2, ("minBy", "LONG", False)), "min": _op(4, 2, ("min", "LONG")),
           "plain": CountWindowOperator(4, 2, ("min", "LONG"), max_batch_rows=1 << 14, output_capacity=1 << 16).open()}
    try:
        for name, op in ops.items():
            if name == "plain":
                op.process_batch(keys, np.arange(120, dtype=np.int64))
            else:
                op.process_batch(*_batch(keys, np.arange(120), "LONG", 0))
        blobs = {name: op.handle.snapshot() for name, op in ops.items()}
        for src, dst, why in [("last", "first", "tie rule"), ("first", "last", "tie rule"), ("min", "first", "tie rule"),
                              ("plain", "min", "not a record count-window snapshot"), ("min", "plain", "not a count-window")]:
            with pytest.raises(_native.FlinkWinError, match=why) as e:
                ops[dst].handle.restore(blobs[src])
            assert e.value.code == abi.FW_E_INVALID
        ops["first"].handle.restore(blobs["first"])   # its own blob restores
    finally:
        for op in ops.values():
            op.close()


# ---- event capacity ----------------------------------------------------------------------------------
def test_event_buffer_capacity():
    """The buffer holds 2 * max_batch_rows events, what one push can raise.  countWindow(1) over distinct
    keys is the densest case: every row of the first push retains (n events), every row of the second
    releases and retains (2n): 3n > 2n without a read in between.  max_batch_rows = 64 is the smallest
    batch the test needs; the key table's minimum is larger."""
    n = 64
    op = _op(1, None, ("sum", "LONG"), max_batch_rows=n, state_capacity=1024)
    try:
        keys = np.arange(n, dtype=np.int64) * 13
        h = op.handle
        h.push_host(keys, np.zeros(n, np.int64), [np.ones(n, np.int64)])
        assert h.stats()["error_flags"] == 0
        h.push_host(keys, np.zeros(n, np.int64), [np.ones(n, np.int64)])
        assert h.stats()["error_flags"] == abi.ERRF["ORDEV"]
        retain, release = h.first_element_events()
        assert len(retain) + len(release) == 2 * n   # clamped to the capacity: 3n were raised
        assert set(retain.tolist()) | set(release.tolist()) <= {(s << 32) | i for s in range(2) for i in range(n)}
        with pytest.raises(_native.FlinkWinError) as e:   # the results stay refused: events were lost
            h.results()
        assert e.value.code == abi.FW_E_CAPACITY
        assert h.first_element_events()[0].size == 0
    finally:
        op.close()
    # read after every push, the same stream is clean
    _run(1, None, ("sum", "LONG"), [_batch(keys, np.ones(n, np.int64), "LONG", 0)] * 3, max_batch_rows=n, state_capacity=1024)


# ---- refused calls ---------------------------------------------------------------------------------
def test_calls_a_record_count_handle_refuses():
    import torch
    op = _op(4, 2, ("sum", "LONG"), parallelism=2, subtask_index=0, max_batch_rows=64)
    try:
        h, L = op.handle, _native.lib()
        for call in (h.results_async, h.results_ready, h.result_segments, h.late_records,
                     lambda: h.device_results_async("cuda"), lambda: h.snapshot_key_group_heap(0),
                     lambda: h.ds_key_group_windows(0)):
            with pytest.raises(_native.FlinkWinError, match="not for count windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        size = C.c_int64()
        for rc in (L.fw_push_device_count_segments(h._h, 0, 1, None, None, None, None),
                   L.fw_push_device_count_packed_segments(h._h, 0, 1, None, None, 3),
                   L.fw_snapshot_key_group(h._h, 0, None, 0, C.byref(size)),
                   L.fw_restore_key_group(h._h, b"x" * 128, 128)):
            assert rc == abi.FW_E_INVALID and "not for record count windows" in L.fw_last_error().decode()
        assert L.fw_push_device_segments(h._h, 0, 1, None, None, None, None, None, None) == abi.FW_E_INVALID
        assert L.fw_push_device_packed_segments(h._h, 0, 1, None, None, 3) == abi.FW_E_INVALID
        assert L.fw_push_device_key_rows(h._h, 0, None, None, None, None, None) == abi.FW_E_INVALID
        k = torch.zeros(65, dtype=torch.int64, device="cuda")   # more than max_batch_rows rows in one push
        with pytest.raises(_native.FlinkWinError, match="max_batch_rows"):
            h.push_device(k, None, [k])
        assert h.first_element_events()[0].size == 0 and h.stats()["error_flags"] == 0
    finally:
        op.close()


# ---- FW_WIN_COUNT is untouched -------------------------------------------------------------------------
def test_same_sums_as_the_count_window_operator():
    from flink_amd.datastream import CountWindowOperator
    rng = np.random.default_rng(41)
    n = 12000
    keys = (rng.integers(0, 40, n) * 977).astype(np.int64)
    vals = rng.integers(-10**6, 10**6, n).astype(np.int64)
    want = [(k, v) for k, v, _, _, _ in CountWindowReference(250, 150, ("sum", "LONG")).process(keys.tolist(), vals.tolist())]
    plain = CountWindowOperator(250, 150, ("sum", "LONG"), max_batch_rows=1 << 14, output_capacity=1 << 16).open()
    rec = _op(250, 150, ("sum", "LONG"))
    try:
        a, b = [], []
        for o in range(0, n, 4000):
            k, v = keys[o:o + 4000], vals[o:o + 4000]
            plain.process_batch(k, v)
            r = plain.collect()
            a += list(zip(r["key"].tolist(), r["value"].tolist()))
            rec.process_batch(k, v, list(zip(k.tolist(), v.tolist())))   # two-field records
            b += [tuple(x) for x in rec.collect()["records"]]
        assert a == b == want and len(want) > 0
    finally:
        plain.close()
        rec.close()
