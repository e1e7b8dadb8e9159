"""Dynamic-gap session windows (EventTimeSessionWindows.withDynamicGap) on the GPU against the
element-by-element reference (dynamic_session_reference.py): the rows of every watermark as a
multiset, the late drops and the late side output.

Integers and DOUBLE min / max compare exactly (a NaN as the canonical NaN); DOUBLE sums at 1e-9
relative, the project's DOUBLE-sum rule: the device adds tile-session partials, the reference adds in
arrival order, and for <= 3000 positive addends the two differ by about 3000 * 2^-53 relative.
Shapes are the smallest that cross every boundary: a tile holds 1024 rows, so the cases sit at
1023 / 1024 / 1025 rows and a few tiles."""
import ctypes as C

import numpy as np
import pytest
from dynamic_session_reference import DynamicSessionReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MAX = (1 << 63) - 1
GAPS = np.array([1, 7, 50, 400], np.int64)
_CANON_NAN = 0x7FF8000000000000
_SPECIAL = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x8000000000000000, 0,
                     np.float64(1.0).view(np.int64), np.float64(-1.0).view(np.int64)], dtype=np.uint64).view(np.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(max_gap, agg=("sum", "LONG"), **kw):
    from flink_amd.datastream import DynamicSessionWindowOperator
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return DynamicSessionWindowOperator(max_gap, agg, **kw).open()


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def _canon(bits):
    return _CANON_NAN if np.isnan(np.int64(bits).view(np.float64)) else int(bits)


def _rows(res):
    return sorted(zip(res["key"].tolist(), res["value"].tolist(), res["window_start"].tolist(), res["window_end"].tolist()),
                  key=lambda r: (r[3], str(r[0]), r[2]))


def _want(rows):
    return sorted(rows, key=lambda r: (r[3], str(r[0]), r[2]))


def _same(got, want, agg=("sum", "LONG")):
    fn, ftype = agg
    assert len(got) == len(want)
    if ftype == "DOUBLE" and fn in ("min", "max"):
        got = [(k, _canon(v), s, e) for k, v, s, e in got]
        want = [(k, _canon(v), s, e) for k, v, s, e in want]
    if ftype == "DOUBLE" and fn == "sum":
        assert [(g[0],) + g[2:] for g in got] == [(w[0],) + w[2:] for w in want]
        gv = np.array([g[1] for g in got], np.int64).view(np.float64)
        wv = np.array([w[1] for w in want], np.int64).view(np.float64)
        np.testing.assert_allclose(gv, wv, rtol=1e-9, atol=0)
    else:
        assert got == want


def _drive(op, ref, steps, agg=("sum", "LONG"), device=False, side=False):
    """steps: ("push", keys, ts, values, gaps) | ("wm", w).  Every watermark's rows, the drop count and
    -- with ``side`` -- the late side output's (push_seq, row) are compared with the reference's."""
    import torch
    fired, seq = 0, 0
    for st in steps:
        if st[0] == "wm":
            got, want = _rows(op.process_watermark(st[1])), _want(ref.process_watermark(st[1]))
            _same(got, want, agg)
            fired += len(want)
            continue
        _, k, ts, v, g = st
        late = ref.process(np.asarray(k).tolist(), np.asarray(ts).tolist(), np.asarray(v).tolist(), np.asarray(g).tolist())
        if device:
            op.process_batch_device(*[torch.tensor(_i64(x), device="cuda") for x in (k, ts, v, g)])
        else:      # a HOST_HASHED operator gets one hash for every key: all keys share a superbucket
            op.process_batch(k, ts, v, g, np.zeros(len(k), np.int32) if op.key_type == "HOST_HASHED" else None)
        if side:
            lr = op.late_records()
            assert sorted(zip(lr["push_seq"].tolist(), lr["row"].tolist())) == [(seq, i) for i in late]
            assert sorted(zip(lr["row"].tolist(), lr["ts"].tolist(), lr["value"].tolist())) == \
                [(i, int(ts[i]), int(v[i])) for i in late]
        if len(k):
            seq += 1
    s = op.handle.stats()
    assert s["num_late_records_dropped"] == ref.late_dropped
    assert s["live_state_entries"] == ref.live_sessions() and s["num_fired_windows"] == fired
    assert s["error_flags"] == 0 and s["pending_rows"] == 0 and s["current_watermark"] == ref.watermark
    return fired


def _run(max_gap, steps, agg=("sum", "LONG"), **kw):
    device, side = kw.pop("device", False), kw.get("late_side_output", False)
    op, ref = _op(max_gap, agg, **kw), DynamicSessionReference(agg)
    try:
        return _drive(op, ref, steps, agg, device, side), ref
    finally:
        op.close()


# ---- nested windows -----------------------------------------------------------------------------------
def _nested(filler):
    """one key: ``filler`` rows of one far-away earlier session, then a row with gap 1000 at ts 0, rows
    with gap 1 at 10, 20, ... 990 inside it, a row at 1000 (touching) and one at 1002 (not)"""
    inner = np.arange(10, 1000, 10)
    ts = np.concatenate([-10**6 + np.arange(filler), [0], inner, [1000, 1002]])
    g = np.concatenate([np.ones(filler), [1000], np.ones(len(inner)), [1, 1]])
    n = len(ts)
    return np.full(n, 5, np.int64), _i64(ts), _i64(np.arange(n) + 1), _i64(g)


@pytest.mark.parametrize("filler", [0, 1023, 1024, 1025])
@pytest.mark.parametrize("device", [False, True])
def test_nested_windows_one_key(filler, device):
    k, ts, v, g = _nested(filler)
    steps = [("push", k, ts, v, g), ("wm", 999), ("wm", 1000), ("wm", LONG_MAX)]
    fired, ref = _run(1000, steps, device=device)
    assert fired == 2 + (filler > 0) and ref.seen["nested"] == 99 and ref.seen["touch"] >= 1


@pytest.mark.parametrize("cut", [1, 50, 101])
def test_nested_windows_split_over_two_pushes(cut):
    k, ts, v, g = _nested(0)      # cut 1: the long window alone is the state; 101: the touching row arrives alone
    steps = [("push", k[:cut], ts[:cut], v[:cut], g[:cut]), ("push", k[cut:], ts[cut:], v[cut:], g[cut:]), ("wm", LONG_MAX)]
    assert _run(1000, steps)[0] == 2


def test_nested_windows_arriving_before_the_long_one():
    """the short windows first, in descending order, then the long one that covers them all"""
    k, ts, v, g = _nested(0)
    o = np.arange(len(k))[::-1]
    steps = [("push", k[o][:60], ts[o][:60], v[o][:60], g[o][:60]), ("push", k[o][60:], ts[o][60:], v[o][60:], g[o][60:]),
             ("wm", LONG_MAX)]
    assert _run(1000, steps)[0] == 2


# ---- one hot key ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pushes", [1, 3])
def test_hot_key_random_gaps_straddling_tiles(n_pushes):
    rng = np.random.default_rng(3)
    n = 3000
    # a row per 50 ms on average: nesting, bridges and about 280 sessions (a superbucket's list holds 1024)
    ts = _i64(rng.integers(0, 150000, n))
    g = GAPS[rng.integers(0, 4, n)]
    cuts = np.linspace(0, n, n_pushes + 1).astype(int)
    k, v = np.full(n, 42, np.int64), _i64(rng.integers(-10**6, 10**6, n))
    steps = [("push", k[a:b], ts[a:b], v[a:b], g[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [("wm", 75000), ("wm", LONG_MAX)]
    fired, ref = _run(400, steps)
    assert fired > 100 and ref.seen["nested"] > 100 and ref.seen["bridge3"] > 0


# ---- many keys --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True])
def test_many_keys_few_superbuckets(side):
    rng = np.random.default_rng(5)
    steps = []
    for p in range(4):
        n = 1000
        k = _i64(rng.integers(0, 50, n)) * 977 - 5000
        ts = _i64(p * 1500 + rng.integers(-1400, 2500, n))    # out of order, a part behind the last watermark (p * 1500 - 800)
        steps.append(("push", k, ts, _i64(rng.integers(-1000, 1000, n)), GAPS[rng.integers(0, 4, n)]))
        steps.append(("wm", p * 1500 + 700))
    steps.append(("wm", LONG_MAX))
    # 2 key groups x 1 superbucket: 50 keys x tens of sessions in two lists
    fired, ref = _run(400, steps, max_parallelism=2, state_capacity=1, late_side_output=side)
    assert fired > 500 and all(v >= 1 for v in ref.seen.values()), ref.seen


# ---- late candidates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("filler", [0, 1023])
@pytest.mark.parametrize("side", [False, True])
def test_late_a_and_b_reaching_a(order, filler, side):
    """watermark 104: A = (95, gap 10) is late alone, B = (60, gap 400) is on time and covers A"""
    fk, ft = np.full(filler, 9, np.int64), _i64(5000 + np.arange(filler))
    a, b = ([9], [95], [1], [10]), ([9], [60], [2], [400])
    first, second = (a, b) if order == "AB" else (b, a)
    cols = [_i64(np.concatenate(x)) for x in zip(first, (fk, ft, np.ones(filler), np.ones(filler)), second)]
    steps = [("push", _i64([9]), _i64([0]), _i64([7]), _i64([50])), ("wm", 104), ("push", *cols), ("wm", LONG_MAX)]
    op, ref = _op(400, max_parallelism=1, state_capacity=1, late_side_output=side), DynamicSessionReference()
    try:
        _drive(op, ref, steps, side=side)
        assert ref.late_dropped == (1 if order == "AB" else 0) and ref.seen["late_kept"] == (0 if order == "AB" else 1)
    finally:
        op.close()


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_same_ts_short_gap_late_long_gap_not(order):
    a, b = (100, 5, 1), (100, 300, 2)      # under watermark 104: [100, 105) is late, [100, 400) is not
    first, second = (a, b) if order == "AB" else (b, a)
    ts, g, v = zip(first, second)
    steps = [("wm", 104), ("push", _i64([3, 3]), _i64(ts), _i64(v), _i64(g)), ("wm", LONG_MAX)]
    fired, ref = _run(400, steps, late_side_output=True)
    assert fired == 1 and ref.late_dropped == (1 if order == "AB" else 0)


@pytest.mark.parametrize("side", [False, True])
def test_backward_chain_of_late_candidates(side):
    # key 1: an anchor, then a chain backwards with different gaps, each touching the one before;
    # key 2: the same chain without the anchor, farthest first: all dropped
    chain = [(90, 10), (60, 30), (59, 1), (9, 50)]
    k, ts, g = [1], [100], [10]
    for t, gg in chain:
        k += [1]
        ts += [t]
        g += [gg]
    for t, gg in reversed(chain):
        k += [2]
        ts += [t]
        g += [gg]
    steps = [("push", _i64([1, 2]), _i64([-500, -500]), _i64([1, 1]), _i64([1, 1])), ("wm", 104),
             ("push", _i64(k), _i64(ts), _i64(np.arange(len(k)) + 1), _i64(g)), ("wm", LONG_MAX)]
    fired, ref = _run(400, steps, late_side_output=side)
    assert ref.late_dropped == 4 and ref.seen["late_kept"] == 4 and fired == 3


# ---- arithmetic ------------------------------------------------------------------------------------------------
def _stream(seed, n_keys=30, n_pushes=3, per=1200, lo=-10**6, hi=10**6):
    rng = np.random.default_rng(seed)
    steps = []
    for p in range(n_pushes):
        k = rng.integers(0, n_keys, per).astype(np.int64) * 31 - 100
        ts = _i64(p * 1500 + rng.integers(0, 3000, per))
        steps.append(("push", k, ts, rng.integers(lo, hi, per).astype(np.int64), GAPS[rng.integers(0, 4, per)]))
        steps.append(("wm", p * 1500 + 600))
    steps.append(("wm", LONG_MAX))
    return steps


@pytest.mark.parametrize("agg", [(fn, ft) for fn in ("sum", "min", "max", "count") for ft in ("LONG", "INT", "DOUBLE")],
                         ids=lambda a: f"{a[0]}-{a[1]}")
def test_aggregations(agg):
    fn, ft = agg
    rng = np.random.default_rng(11)
    steps = _stream(7, lo=(1 << 31) - 5000 if ft == "INT" else -10**6, hi=1 << 31 if ft == "INT" else 10**6)
    if ft == "DOUBLE":
        out = []
        for st in steps:
            if st[0] == "push":
                if fn == "sum":      # positive addends: the sum's tolerance is the one derived above
                    dv = (rng.random(len(st[1])) * 1000.0).view(np.int64).copy()
                else:
                    dv = (rng.random(len(st[1])) * 100.0 - 50.0).view(np.int64).copy()
                    sp = rng.random(len(dv)) < 0.4
                    dv[sp] = _SPECIAL[rng.integers(0, len(_SPECIAL), int(sp.sum()))]
                st = ("push", st[1], st[2], dv, st[4])
            out.append(st)
        steps = out
    op, ref = _op(400, agg), DynamicSessionReference(agg)
    try:
        assert _drive(op, ref, steps[:-1], agg) >= 30
        res = op.process_watermark(LONG_MAX)
        _same(_rows(res), _want(ref.process_watermark(LONG_MAX)), agg)
        if agg == ("sum", "INT"):
            assert any(v < 0 for v in res["value"].tolist())      # sums of values near 2^31 wrapped
    finally:
        op.close()


# ---- constant gap: the static operator's rows ---------------------------------------------------------------------
def test_constant_gap_equals_the_static_operator():
    from flink_amd.datastream import SessionWindowOperator
    rng = np.random.default_rng(21)
    n, gap = 3000, 50
    k = _i64(rng.integers(0, 40, n)) * 13
    ts = _i64(rng.integers(0, 6000, n))
    v = _i64(rng.integers(-1000, 1000, n))
    st = SessionWindowOperator(gap, ("sum", "LONG"), max_batch_rows=1 << 14, output_capacity=1 << 16).open()
    dy = _op(gap)
    try:
        total = 0
        for a, b, wm in [(0, 1500, 2000), (1500, 3000, 4000), (3000, 3000, LONG_MAX)]:
            if b > a:
                st.process_batch(k[a:b], ts[a:b], v[a:b])
                dy.process_batch(k[a:b], ts[a:b], v[a:b], np.full(b - a, gap, np.int64))
            rs, rd = st.process_watermark(wm), dy.process_watermark(wm)
            assert _rows(rs) == _rows(rd)
            total += len(rs["key"])
        assert total > 200
        assert st.handle.stats()["num_late_records_dropped"] == dy.handle.stats()["num_late_records_dropped"] > 0
    finally:
        st.close()
        dy.close()


# ---- gaps out of range on the device path -------------------------------------------------------------------------------
def test_out_of_range_gaps_on_the_device_path():
    import torch
    rng = np.random.default_rng(31)
    n = 2100      # three tiles of one superbucket share
    k = _i64(rng.integers(0, 20, n))
    ts = _i64(rng.integers(0, 5000, n))
    v = _i64(rng.integers(-1000, 1000, n))
    g = GAPS[rng.integers(0, 4, n)].copy()
    bad = rng.random(n) < 0.05
    g[bad] = np.array([0, -1, 401], np.int64)[rng.integers(0, 3, int(bad.sum()))]
    g[:3], bad[:3] = [0, -1, 401], True
    ok = ~bad
    ref = DynamicSessionReference()
    ref.process(k[ok].tolist(), ts[ok].tolist(), v[ok].tolist(), g[ok].tolist())
    a = _op(400, max_parallelism=1, state_capacity=1)
    b = None
    try:
        with pytest.raises(ValueError, match="0 < gap"):      # the host path checks before it pushes
            a.process_batch(k, ts, v, g)
        with pytest.raises(ValueError, match="max_gap_ms"):
            a.process_batch(k[:1], ts[:1], v[:1], _i64([401]))
        assert a.handle.stats()["live_state_entries"] == 0
        a.process_batch_device(*[torch.tensor(x, device="cuda") for x in (k, ts, v, g)])
        st = a.handle.stats()
        assert st["error_flags"] == abi.ERRF["GAP"] and st["live_state_entries"] == ref.live_sessions()
        assert st["num_late_records_dropped"] == 0
        with pytest.raises(ValueError, match="0 < gap"):
            a.process_watermark(LONG_MAX)
        # the state holds the valid rows' sessions: a whole restore clears the flags, as after a restart
        blob = a.snapshot_state()
        a.close()
        b = _op(400, max_parallelism=1, state_capacity=1)
        b.initialize_state(blob)
        _same(_rows(b.process_watermark(LONG_MAX)), _want(ref.process_watermark(LONG_MAX)))
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- checkpoint -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", ["LONG", "STRING"])
def test_snapshot_restore_mid_session(key_type):
    steps = _stream(41, n_keys=100, n_pushes=4)
    if key_type == "STRING":
        steps = [("push", [f"w{int(x)}" for x in s[1]], *s[2:]) if s[0] == "push" else s for s in steps]
    ref = DynamicSessionReference()
    a = _op(400, key_type=key_type, state_capacity=1 << 12)
    b = c = None
    try:
        _drive(a, ref, steps[:5])                  # stops behind a push: sessions are open
        blob = a.snapshot_state()
        a.close()
        b = _op(400, key_type=key_type, state_capacity=1 << 18 if key_type == "LONG" else 1 << 12)
        b.initialize_state(blob)
        st = b.handle.stats()
        assert st["live_state_entries"] == ref.live_sessions() and st["current_watermark"] == ref.watermark
        for s in steps[5:]:
            if s[0] == "push":
                ref.process(np.asarray(s[1]).tolist(), s[2].tolist(), s[3].tolist(), s[4].tolist())
                b.process_batch(*s[1:])
            else:
                _same(_rows(b.process_watermark(s[1])), _want(ref.process_watermark(s[1])))
        assert b.handle.stats()["live_state_entries"] == 0 and b.handle.stats()["error_flags"] == 0
        if key_type == "LONG":      # the fingerprint names the kind and size_ms
            from flink_amd.datastream import SessionWindowOperator
            c = SessionWindowOperator(400, max_batch_rows=1 << 14, output_capacity=1 << 16).open()
            with pytest.raises(_native.FlinkWinError, match="different operator configuration"):
                b.initialize_state(c.snapshot_state())
            with pytest.raises(_native.FlinkWinError, match="different operator configuration"):
                c.initialize_state(blob)
            c.close()
            c = _op(401)
            with pytest.raises(_native.FlinkWinError, match="different operator configuration"):
                c.initialize_state(blob)
    finally:
        for op in (a, b, c):
            if op is not None:
                op.close()


def _dest(keys, p):
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_LONG, 128, p, None,
                                                          d.ctypes.data))
    return d


@pytest.mark.parametrize("src,dst", [(1, 2), (2, 1)])
def test_key_group_snapshots_rescale(src, dst):
    steps = _stream(43, n_keys=200, n_pushes=4)
    ref = DynamicSessionReference()
    olds = [_op(400, parallelism=src, subtask_index=i) for i in range(src)]
    news = []

    def run(ops, part):
        for s in part:
            if s[0] == "push":
                d = _dest(s[1], len(ops))
                ref.process(s[1].tolist(), s[2].tolist(), s[3].tolist(), s[4].tolist())
                for i, op in enumerate(ops):
                    op.process_batch(*[x[d == i] for x in s[1:]])
            else:
                got = [r for op in ops for r in _rows(op.process_watermark(s[1]))]
                _same(_want(got), _want(ref.process_watermark(s[1])))
    try:
        run(olds, steps[:5])
        blobs = {}
        for op in olds:
            blobs.update(op.handle.snapshot_key_groups()[0])
        assert len(blobs) == 128
        wm = ref.watermark
        for op in olds:
            op.close()
        news = [_op(400, parallelism=dst, subtask_index=i) for i in range(dst)]
        for op in news:
            op.handle.restore_key_groups(blobs, [])
            op.handle.initialize_watermark(wm)      # the DataStream operator's watermark comes from the stream
        assert sum(op.handle.stats()["live_state_entries"] for op in news) == ref.live_sessions() > 0
        run(news, steps[5:])
        assert all(op.handle.stats()["error_flags"] == 0 for op in news)
    finally:
        for op in olds + news:
            op.close()


# ---- capacity ---------------------------------------------------------------------------------------------
def test_output_capacity_raises_output_flag():
    op = _op(400, output_capacity=16)
    try:
        op.process_batch(_i64(np.arange(10)), np.zeros(10, np.int64), np.ones(10, np.int64), np.full(10, 7, np.int64))
        assert len(op.process_watermark(50)["key"]) == 10 and op.handle.stats()["error_flags"] == 0
        op.process_batch(_i64(np.arange(40)), np.full(40, 1000, np.int64), np.ones(40, np.int64), np.full(40, 7, np.int64))
        with pytest.raises(_native.FlinkWinError) as e:
            op.process_watermark(2000)      # 40 fires
        assert e.value.code == abi.FW_E_CAPACITY
        assert op.handle.stats()["error_flags"] & abi.ERRF["OUTPUT"]
    finally:
        op.close()


def test_state_capacity_raises_state_flag():
    op = _op(400, state_capacity=1, max_parallelism=1)      # the smallest state: 2 superbuckets of 1024 sessions
    try:
        op.process_batch(_i64(np.arange(5000)), np.zeros(5000, np.int64), np.ones(5000, np.int64), np.full(5000, 7, np.int64))
        st = op.handle.stats()
        assert st["error_flags"] & abi.ERRF["STATE"] and 0 < st["live_state_entries"] <= 2048
        with pytest.raises(_native.FlinkWinError) as e:
            op.process_watermark(10)
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()


def test_late_capacity_raises_late_flag():
    op = _op(400, late_side_output=True, max_batch_rows=64)      # the side output holds 128 rows
    try:
        op.process_watermark(1000)
        for _ in range(3):
            op.process_batch(_i64(np.arange(64)), np.zeros(64, np.int64), np.ones(64, np.int64), np.full(64, 7, np.int64))
        st = op.handle.stats()
        assert st["error_flags"] & abi.ERRF["LATE"] and st["num_late_records_dropped"] == 192
        with pytest.raises(_native.FlinkWinError) as e:
            op.late_records()
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()


# ---- refused calls ---------------------------------------------------------------------------------------------
def test_calls_a_dynamic_session_handle_refuses():
    import torch
    op, ref = _op(400), DynamicSessionReference()
    try:
        h, L = op.handle, _native.lib()
        op.process_batch(_i64([1]), _i64([0]), _i64([5]), _i64([9]))
        ref.process([1], [0], [5], [9])
        wm = torch.zeros(1, dtype=torch.int64, device="cuda")
        with pytest.raises(_native.FlinkWinError, match="not for session windows") as e:
            h.advance_device(wm)
        assert e.value.code == abi.FW_E_INVALID
        assert L.fw_push_device_segments(h._h, 0, 1, None, None, None, None, None, None) == abi.FW_E_INVALID
        assert "not for session windows" in L.fw_last_error().decode()
        assert L.fw_push_device_key_rows(h._h, 0, None, None, None, None, None) == abi.FW_E_INVALID
        assert "not for session windows" in L.fw_last_error().decode()
        arr = (C.c_void_p * abi.FW_MAX_COLS)(wm.data_ptr())      # the gap column is required
        assert L.fw_push_device(h._h, 1, wm.data_ptr(), wm.data_ptr(), None, arr, None) == abi.FW_E_INVALID
        assert "value column 1 is NULL" in L.fw_last_error().decode()
        # the handle is still usable
        _same(_rows(op.process_watermark(LONG_MAX)), _want(ref.process_watermark(LONG_MAX)))
    finally:
        op.close()
