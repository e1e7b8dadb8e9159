"""Session windows (EventTimeSessionWindows.withGap) on the GPU against the element-by-element
reference (session_window_reference.py): the rows of every watermark as a multiset, the late drops
and the late side output.

Integers and DOUBLE min / max compare exactly (a NaN as the canonical NaN); DOUBLE sums at 1e-9
relative, the project's DOUBLE-sum rule: the device adds tile-session partials, the reference adds
in arrival order, and for <= 3000 positive addends the two differ by about 3000 * 2^-53 relative.
Shapes are the smallest that cross every boundary: a tile holds 1024 rows, so the cases sit at
1023 / 1024 / 1025 rows and a few tiles."""
import ctypes as C

import numpy as np
import pytest
from session_window_reference import SessionWindowReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MAX = (1 << 63) - 1
_CANON_NAN = 0x7FF8000000000000
_SPECIAL = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x8000000000000000, 0,
                     np.float64(1.0).view(np.int64), np.float64(-1.0).view(np.int64)], dtype=np.uint64).view(np.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(gap, agg=("sum", "LONG"), **kw):
    from flink_amd.datastream import SessionWindowOperator
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return SessionWindowOperator(gap, agg, **kw).open()


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
    """steps: ("push", keys, ts, values) | ("wm", w).  Every watermark's rows, the drop count and --
    with ``side`` -- the late side output's (push_seq, row) are compared with the reference's."""
    import torch
    fired, seq = 0, 0
    for st in steps:
        if st[0] == "wm":
            got, want = _rows(op.process_watermark(st[1])), _want(ref.process_watermark(st[1]))
            _same(got, want, agg)
            fired += len(want)
            continue
        _, k, ts, v = st
        late = ref.process(np.asarray(k).tolist(), np.asarray(ts).tolist(), np.asarray(v).tolist())
        if device:
            if len(k):
                op.process_batch_device(torch.tensor(np.asarray(k, np.int64), device="cuda"),
                                        torch.tensor(np.asarray(ts, np.int64), device="cuda"),
                                        torch.tensor(np.asarray(v, np.int64), device="cuda"))
        else:      # a HOST_HASHED operator gets one hash for every key: all keys share a superbucket
            op.process_batch(k, ts, v, np.zeros(len(k), np.int32) if op.key_type == "HOST_HASHED" else None)
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


def _run(gap, steps, agg=("sum", "LONG"), **kw):
    device, side = kw.pop("device", False), kw.get("late_side_output", False)
    op, ref = _op(gap, agg, **kw), SessionWindowReference(gap, agg)
    try:
        return _drive(op, ref, steps, agg, device, side)
    finally:
        op.close()


def _i64(x):
    return np.asarray(x, dtype=np.int64)


# ---- the transcribed case -------------------------------------------------------------------------
def test_transcribed_session_windows_case():
    """WindowOperatorTest.testSessionWindows (gap 3000, sum), recalled from the reference's test, with its
    snapshot / restore after the fifth element; STRING keys."""
    a = _op(3000, key_type="STRING")
    b = None
    try:
        a.process_batch(["key2", "key2", "key2", "key1", "key1"], [0, 1000, 2500, 10, 1000], [1, 2, 3, 1, 2])
        blob = a.snapshot_state()
        a.close()
        b = _op(3000, key_type="STRING")
        b.initialize_state(blob)
        b.process_batch(["key1", "key2", "key2", "key2", "key2"], [2500, 5501, 6000, 6000, 6050], [3, 4, 5, 5, 6])
        res = b.process_watermark(12000)
        assert b.output_records(res) == [("key1", 6, 5499), ("key2", 6, 5499), ("key2", 20, 9049)]
        assert _rows(res) == _want([("key1", 6, 10, 5500), ("key2", 6, 0, 5500), ("key2", 20, 5501, 9050)])
        b.process_batch(["key1", "key1"], [15000, 15000], [10, 20])
        res = b.process_watermark(17999)
        assert _rows(res) == [("key1", 30, 15000, 18000)] and b.output_records(res) == [("key1", 30, 17999)]
        st = b.handle.stats()
        assert st["live_state_entries"] == 0 and st["num_late_records_dropped"] == 0 and st["num_fired_windows"] == 4
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- one hot key ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3000])
@pytest.mark.parametrize("n_pushes", [1, 10])
def test_hot_key_one_session(n, n_pushes):
    rng = np.random.default_rng(n)
    ts = rng.permutation(n).astype(np.int64) * 3          # one session: neighbours 3 apart, gap 5
    v = rng.integers(-10**6, 10**6, n).astype(np.int64)
    k = np.full(n, 42, np.int64)
    cuts = np.linspace(0, n, n_pushes + 1).astype(int)
    steps = [("push", k[a:b], ts[a:b], v[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    steps += [("wm", 3 * n), ("wm", 3 * n + 1), ("wm", 3 * n + 2)]     # end - 1 = 3 (n - 1) + 4 = 3 n + 1
    assert _run(5, steps) == 1


def test_hot_key_device_columns():
    n = 2500
    ts = np.arange(n, dtype=np.int64) * 2
    steps = [("push", np.full(n, 7, np.int64), ts, np.ones(n, np.int64)), ("wm", LONG_MAX)]
    assert _run(2, steps, device=True) == 1


# ---- sessions straddling tiles and pushes -----------------------------------------------------------
@pytest.mark.parametrize("cut", [1023, 1024, 1025])
@pytest.mark.parametrize("split", [False, True])
def test_sessions_straddling_tiles_and_pushes(cut, split):
    """three alternating keys in one superbucket's arrival order; each key's sessions break where its
    row index passes ``cut`` and again 700 rows later"""
    n = 3 * 1100
    i = np.arange(n)
    k = _i64(i % 3)
    per = i // 3
    ts = _i64(per * 4 + (per * 3 >= cut) * 1000 + (per * 3 >= cut + 700) * 1000)
    v = _i64(i + 1)
    if split:
        steps = [("push", k[:cut], ts[:cut], v[:cut]), ("push", k[cut:], ts[cut:], v[cut:])]
    else:
        steps = [("push", k, ts, v)]
    steps += [("wm", 500), ("wm", int(ts[cut]) + 100), ("wm", LONG_MAX)]
    assert _run(4, steps, key_type="HOST_HASHED") == 9


# ---- bridges ------------------------------------------------------------------------------------------
def test_bridges_between_state_sessions():
    pad_k = _i64(np.arange(1100) % 50 + 100)      # 50 other keys, one session each, filling a tile
    pad_t = _i64(10000 + (np.arange(1100) // 50) * 5)
    pad_v = np.ones(1100, np.int64)
    steps = [
        ("push", _i64([1, 1, 2, 2, 2, 3, 3]), _i64([0, 20, 0, 15, 30, 0, 20]), _i64([1, 2, 4, 8, 16, 32, 64])),
        ("push", _i64([1]), _i64([10]), _i64([100])),              # [10, 20) joins [0, 10) and [20, 30)
        ("push", _i64([2, 2]), _i64([8, 23]), _i64([100, 200])),   # three state sessions become one in one tile
        # the bridging element of key 3 in a later tile of the same push
        ("push", np.concatenate([pad_k, _i64([3])]), np.concatenate([pad_t, _i64([10])]), np.concatenate([pad_v, _i64([1000])])),
        ("wm", 500),
        ("wm", LONG_MAX),
    ]
    assert _run(10, steps, key_type="HOST_HASHED") == 3 + 50


# ---- many keys ------------------------------------------------------------------------------------------
def test_many_keys_few_superbuckets():
    rng = np.random.default_rng(5)
    gap, steps = 50, []
    for p in range(4):
        reps = rng.integers(1, 7, 3000)
        k = np.repeat(np.arange(3000, dtype=np.int64) * 977 - 5000, reps)
        ts = _i64(p * 400 + rng.integers(0, 600, len(k)))
        order = rng.permutation(len(k))
        steps.append(("push", k[order], ts[order], rng.integers(-1000, 1000, len(k)).astype(np.int64)))
        steps.append(("wm", p * 400 + 150))       # fires part of each key's sessions
    steps.append(("wm", LONG_MAX))
    # 2 key groups x 16 sub-buckets: about 3000 keys x a few sessions in 32 lists of 1024
    assert _run(gap, steps, max_parallelism=2, state_capacity=16384, max_batch_rows=1 << 15) > 6000


# ---- late candidates -----------------------------------------------------------------------------------
def _rule3(order, filler):
    """watermark 104, gap 10: A = (95) is late alone, B = (100) is on time and reaches A.  ``filler`` rows
    of the same key, one far-away session, put the two on either side of a tile boundary."""
    fk, ft, fv = np.full(filler, 9, np.int64), _i64(1000 + np.arange(filler)), np.ones(filler, np.int64)
    a, b = (_i64([9]), _i64([95]), _i64([1])), (_i64([9]), _i64([100]), _i64([2]))
    first, second = (a, b) if order == "AB" else (b, a)
    cols = [np.concatenate(x) for x in zip(first, (fk, ft, fv), second)]
    return [("push", _i64([9]), _i64([60]), _i64([7])), ("wm", 104), ("push", cols[0], cols[1], cols[2]), ("wm", LONG_MAX)]


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("filler", [0, 1023])
@pytest.mark.parametrize("side", [False, True])
def test_rule_3_orders(order, filler, side):
    op, ref = _op(10, max_parallelism=1, state_capacity=1, late_side_output=side), SessionWindowReference(10)
    try:
        _drive(op, ref, _rule3(order, filler), side=side)
        assert ref.late_dropped == (1 if order == "AB" else 0)
    finally:
        op.close()


@pytest.mark.parametrize("side", [False, True])
def test_backward_chain_of_late_candidates(side):
    steps = [("push", _i64([1, 2]), _i64([0, 0]), _i64([1, 1])), ("wm", 104),
             # key 1: anchor then a chain backwards; key 2: the chain without an anchor, farthest first
             ("push", _i64([1, 2, 1, 2, 1, 2, 1]), _i64([100, 70, 90, 80, 80, 90, 70]), _i64([1, 8, 2, 4, 4, 2, 8])),
             ("wm", LONG_MAX)]
    op, ref = _op(10, late_side_output=side), SessionWindowReference(10)
    try:
        _drive(op, ref, steps, side=side)
        assert ref.late_dropped == 3
    finally:
        op.close()


def test_push_of_late_candidates_only():
    """2048 rows, all late candidates: 32 keys with a live session each; per key 32 rows chain backwards
    from it (accepted) and 32 lie a gap further back, farthest first (dropped)."""
    import time
    gap, W = 10, 10_000
    anchors = _i64(np.arange(32))      # [W - 8, W + 2): live under W
    k, ts = [], []
    for key in range(32):
        for j in range(32):
            k += [key, key]
            ts += [W - 8 - gap * (j + 1), W - 5000 - gap * (32 - j)]    # the chain, nearest first; the unreachable ones
    k, ts = _i64(k), _i64(ts)
    steps = [("push", anchors, np.full(32, W - 8, np.int64), np.ones(32, np.int64)), ("wm", W),
             ("push", k, ts, _i64(np.arange(len(k)))), ("wm", LONG_MAX)]
    assert len(k) == 2048 and bool(np.all(ts + gap - 1 <= W))
    op, ref = _op(gap, late_side_output=True, max_parallelism=1, state_capacity=1), SessionWindowReference(gap)
    try:
        t0 = time.perf_counter()
        _drive(op, ref, steps, side=True)
        assert ref.late_dropped == 1024 and time.perf_counter() - t0 < 5.0
    finally:
        op.close()


# ---- rule 4 ------------------------------------------------------------------------------------------
def test_fire_boundaries_and_fresh_start():
    steps = [("push", _i64([1, 2]), _i64([100, 101]), _i64([1, 2])),
             ("wm", 108),                       # end - 1 == W' + 1 for key 1: nothing
             ("wm", 109),                       # key 1 fires (end - 1 == W'), key 2 not (110 == W' + 1)
             ("wm", 109), ("wm", 50),           # W' <= W changes nothing
             # key 1 starts afresh: 100 is now late alone, 105 is not and opens a new session
             ("push", _i64([1, 1, 2]), _i64([100, 105, 111]), _i64([10, 20, 30])),
             ("wm", 114), ("wm", LONG_MAX)]
    assert _run(10, steps) == 3


def test_initialize_watermark_and_empty_pushes():
    op, ref = _op(10), SessionWindowReference(10)
    try:
        assert len(op.process_watermark(5)["key"]) == 0      # a watermark with no state
        ref.process_watermark(5)
        op.handle.initialize_watermark(1000)
        ref.watermark = 1000
        e = np.empty(0, np.int64)
        steps = [("push", e, e, e), ("push", _i64([3]), _i64([990]), _i64([1])),      # late: 990 + 10 - 1 <= 1000
                 ("push", _i64([3]), _i64([992]), _i64([2])), ("push", e, e, e),
                 ("push", _i64([3]), _i64([985]), _i64([4])), ("wm", 1001), ("wm", 1002)]
        assert _drive(op, ref, steps) == 1 and ref.late_dropped == 1
        op.handle.flush()
        assert op.handle.stats()["results_available"] == 0
    finally:
        op.close()


# ---- arithmetic and keys ------------------------------------------------------------------------------
def _stream(seed, n_keys, n_pushes, per, gap, lo=-10**6, hi=10**6):
    rng = np.random.default_rng(seed)
    steps = []
    for p in range(n_pushes):
        k = rng.integers(0, n_keys, per).astype(np.int64) * 31 - 100
        ts = _i64(p * 6 * gap + rng.integers(0, 12 * gap, per))
        steps.append(("push", k, ts, rng.integers(lo, hi, per).astype(np.int64)))
        steps.append(("wm", p * 6 * gap + 2 * gap))
    steps.append(("wm", LONG_MAX))
    return steps


def test_int_sum_wraps_at_32_bits():
    steps = _stream(3, 40, 4, 2000, 2, lo=(1 << 31) - 5000, hi=1 << 31)
    op, ref = _op(2, ("sum", "INT")), SessionWindowReference(2, ("sum", "INT"))
    try:
        _drive(op, ref, steps[:-1], ("sum", "INT"))
        res = op.process_watermark(LONG_MAX)
        _same(_rows(res), _want(ref.process_watermark(LONG_MAX)), ("sum", "INT"))
        assert any(v < 0 for v in res["value"].tolist())          # sums of values near 2^31 wrapped
    finally:
        op.close()


@pytest.mark.parametrize("fn", ["min", "max"])
def test_double_min_max_special_values(fn):
    rng = np.random.default_rng(11)
    steps = []
    for st in _stream(5, 30, 4, 2000, 3):
        if st[0] == "push":
            dv = (rng.random(len(st[1])) * 100.0 - 50.0).view(np.int64).copy()
            sp = rng.random(len(dv)) < 0.4
            dv[sp] = _SPECIAL[rng.integers(0, len(_SPECIAL), int(sp.sum()))]
            st = ("push", st[1], st[2], dv)
        steps.append(st)
    assert _run(3, steps, (fn, "DOUBLE")) >= 30


def test_double_sum_of_positive_values():
    rng = np.random.default_rng(13)
    steps = [("push", s[1], s[2], (rng.random(len(s[1])) * 1000.0).view(np.int64).copy()) if s[0] == "push" else s
             for s in _stream(9, 20, 4, 3000, 3)]
    assert _run(3, steps, ("sum", "DOUBLE")) >= 20


def test_count():
    assert _run(4, _stream(17, 25, 3, 2000, 4), ("count", "LONG")) >= 25


def test_string_keys_and_precomputed_hashes():
    steps = _stream(19, 60, 3, 1500, 5)
    op, ref = _op(5, key_type="STRING"), SessionWindowReference(5)
    try:
        steps = [("push", [f"user-{int(x)}" for x in s[1]], s[2], s[3]) if s[0] == "push" else s for s in steps]
        assert _drive(op, ref, steps) >= 60
    finally:
        op.close()
    op, ref = _op(5, key_type="HOST_HASHED"), SessionWindowReference(5)
    try:
        for s in _stream(23, 60, 3, 1500, 5):
            if s[0] == "push":
                op.process_batch(s[1], s[2], s[3], key_hashes=(s[1] * 2654435761 % (1 << 31)).astype(np.int32))
                ref.process(s[1].tolist(), s[2].tolist(), s[3].tolist())
            else:
                _same(_rows(op.process_watermark(s[1])), _want(ref.process_watermark(s[1])))
        assert op.handle.stats()["num_late_records_dropped"] == ref.late_dropped and op.handle.stats()["error_flags"] == 0
    finally:
        op.close()


# ---- sharding -------------------------------------------------------------------------------------
def _dest(keys, p):
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_LONG, 128, p, None,
                                                          d.ctypes.data))
    return d


def test_sharding_two_subtasks():
    steps = _stream(29, 300, 4, 3000, 5)
    ref = SessionWindowReference(5)
    ops = [_op(5, parallelism=2, subtask_index=i) for i in range(2)]
    try:
        for s in steps:
            if s[0] == "push":
                d = _dest(s[1], 2)
                ref.process(s[1].tolist(), s[2].tolist(), s[3].tolist())
                for i, op in enumerate(ops):
                    op.process_batch(s[1][d == i], s[2][d == i], s[3][d == i])
            else:
                parts = [_rows(op.process_watermark(s[1])) for op in ops]
                _same(_want(parts[0] + parts[1]), _want(ref.process_watermark(s[1])))
                assert not {r[0] for r in parts[0]} & {r[0] for r in parts[1]}      # no key fired by both
        assert sum(op.handle.stats()["num_late_records_dropped"] for op in ops) == ref.late_dropped
        assert all(op.handle.stats()["error_flags"] == 0 for op in ops)
        stray = steps[0][1][_dest(steps[0][1], 2) == 1][:1]      # a row pushed to the wrong subtask
        ops[0].process_batch(stray, _i64([LONG_MAX // 4]), np.ones(1, np.int64))
        assert ops[0].handle.stats()["error_flags"] & abi.ERRF["KEYGROUP"]
    finally:
        for op in ops:
            op.close()


# ---- checkpoint -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", ["LONG", "STRING"])
def test_snapshot_restore_mid_session(key_type):
    steps = _stream(31, 200, 6, 1500, 5)
    if key_type == "STRING":
        steps = [("push", [f"w{int(x)}" for x in s[1]], s[2], s[3]) if s[0] == "push" else s for s in steps]
    ref = SessionWindowReference(5)
    a = _op(5, key_type=key_type, state_capacity=1 << 12)
    b = None
    try:
        _drive(a, ref, steps[:5])                  # stops behind a push: sessions are open
        blob = a.snapshot_state()
        a.close()
        # another superbucket split (precomputed-hash keys may not be split finer than the snapshot's)
        b = _op(5, key_type=key_type, state_capacity=1 << 18 if key_type == "LONG" else 1 << 12)
        b.initialize_state(blob)
        st = b.handle.stats()
        assert st["live_state_entries"] == ref.live_sessions() and st["current_watermark"] == ref.watermark
        fired, dropped = st["num_fired_windows"], st["num_late_records_dropped"]
        for s in steps[5:]:
            if s[0] == "push":
                ref.process(np.asarray(s[1]).tolist(), s[2].tolist(), s[3].tolist())
                b.process_batch(s[1], s[2], s[3])
            else:
                _same(_rows(b.process_watermark(s[1])), _want(ref.process_watermark(s[1])))
        assert b.handle.stats()["live_state_entries"] == 0 and b.handle.stats()["error_flags"] == 0
        assert fired == 0 and dropped == 0         # counters are not part of the blob
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("src,dst", [(1, 2), (2, 1)])
def test_key_group_snapshots_rescale(src, dst):
    steps = _stream(37, 300, 6, 2000, 5)
    ref = SessionWindowReference(5)
    olds = [_op(5, parallelism=src, subtask_index=i) for i in range(src)]
    news = []

    def run(ops, part):
        for s in part:
            if s[0] == "push":
                d = _dest(s[1], len(ops))
                ref.process(s[1].tolist(), s[2].tolist(), s[3].tolist())
                for i, op in enumerate(ops):
                    op.process_batch(s[1][d == i], s[2][d == i], s[3][d == i])
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
        news = [_op(5, parallelism=dst, subtask_index=i) for i in range(dst)]
        for op in news:
            op.handle.restore_key_groups(blobs, [])
            op.handle.initialize_watermark(wm)      # the DataStream operator's watermark comes from the stream
        assert sum(op.handle.stats()["live_state_entries"] for op in news) == ref.live_sessions()
        run(news, steps[5:-1])
        assert all(op.handle.stats()["error_flags"] == 0 for op in news)
        live = {kg: b for kg, b in news[0].handle.snapshot_key_groups()[0].items() if len(b) > 48}      # header: 48 bytes
        assert live
        with pytest.raises(_native.FlinkWinError) as e:      # a key group restored over live state
            news[0].handle.restore_key_group_blob(next(iter(live.values())))
        run(news, steps[-1:])                                # the handle is unharmed
        assert e.value.code == abi.FW_E_STATE
    finally:
        for op in olds + news:
            op.close()


# ---- capacity -------------------------------------------------------------------------------------
def test_output_capacity():
    op = _op(1, output_capacity=16)
    try:
        for i in range(3):      # collected in time: clean
            op.process_batch(_i64(np.arange(10)), np.full(10, 100 * i, np.int64), np.ones(10, np.int64))
            assert len(op.process_watermark(100 * i + 50)["key"]) == 10
        assert op.handle.stats()["error_flags"] == 0
        op.process_batch(_i64(np.arange(40)), np.full(40, 1000, np.int64), np.ones(40, np.int64))
        with pytest.raises(_native.FlinkWinError) as e:
            op.process_watermark(2000)      # 40 fires
        assert e.value.code == abi.FW_E_CAPACITY
        assert op.handle.stats()["error_flags"] & abi.ERRF["OUTPUT"]
    finally:
        op.close()


def test_state_capacity_raises_state_flag():
    op = _op(1, state_capacity=1, max_parallelism=1)      # the smallest state: 2 superbuckets of 1024 sessions
    try:
        op.process_batch(_i64(np.arange(5000)), np.zeros(5000, np.int64), np.ones(5000, np.int64))
        st = op.handle.stats()
        assert st["error_flags"] & abi.ERRF["STATE"] and 0 < st["live_state_entries"] <= 2048
        with pytest.raises(_native.FlinkWinError) as e:
            op.process_watermark(10)
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()


def test_late_capacity_raises_late_flag():
    op = _op(1, late_side_output=True, max_batch_rows=64)      # the side output holds 128 rows
    try:
        op.process_watermark(1000)
        for _ in range(3):
            op.process_batch(_i64(np.arange(64)), np.zeros(64, np.int64), np.ones(64, np.int64))
        st = op.handle.stats()
        assert st["error_flags"] & abi.ERRF["LATE"] and st["num_late_records_dropped"] == 192
        with pytest.raises(_native.FlinkWinError) as e:
            op.late_records()
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()


# ---- refused calls ------------------------------------------------------------------------------------
def test_calls_a_session_handle_refuses():
    import torch
    op, ref = _op(10), SessionWindowReference(10)
    try:
        h, L = op.handle, _native.lib()
        op.process_batch(_i64([1]), _i64([0]), _i64([5]))
        ref.process([1], [0], [5])
        wm = torch.zeros(1, dtype=torch.int64, device="cuda")
        for call in (h.results_async, h.results_ready, h.result_segments, h.first_element_events,
                     lambda: h.device_results_async("cuda"), lambda: h.snapshot_key_group_heap(0),
                     lambda: h.restore_key_group_heap(b"\0" * 16), lambda: h.ds_key_group_windows(0),
                     lambda: h.ds_restore_key_group_windows(0, [], 0), lambda: h.advance_device(wm),
                     lambda: h.set_profiling(True), h.kernel_times):
            with pytest.raises(_native.FlinkWinError, match="not for session windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        assert L.fw_push_device_segments(h._h, 0, 1, None, None, None, None, None, None) == abi.FW_E_INVALID
        assert L.fw_push_device_packed_segments(h._h, 0, 1, None, None, 3) == abi.FW_E_INVALID
        assert L.fw_push_device_key_rows(h._h, 0, None, None, None, None, None) == abi.FW_E_INVALID
        assert L.fw_push_device(h._h, 1, wm.data_ptr(), None, None, None, None) == abi.FW_E_INVALID      # d_ts is required
        with pytest.raises(_native.FlinkWinError) as e:      # no late side output configured
            h.late_records()
        assert e.value.code == abi.FW_E_STATE
        r = abi.fw_result()
        _native.check(L.fw_results(h._h, C.byref(r), 1))
        assert r.n == 0 and not r.first_ord
        # the handle is still usable
        _same(_rows(op.process_watermark(LONG_MAX)), _want(ref.process_watermark(LONG_MAX)))
    finally:
        op.close()
