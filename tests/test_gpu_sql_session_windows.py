"""The SQL SESSION window TVF aggregate on the GPU against the element-by-element checker
(sql_session_reference.py, recalled): the rows of every watermark as a multiset, the late drops and
the live / fired counters.

Integers and NULL masks compare exactly; DOUBLE SUM / AVG at 1e-9 relative, the project's DOUBLE-sum
rule: the device adds tile-session partials, the checker adds in arrival order, and for <= 3000
positive addends per session the two differ by about 3000 * 2^-53 relative.  Shapes are the smallest
that cross every boundary: a tile holds 1024 rows and a coalesce chunk 1024 entries, so the cases
sit at 1023 / 1024 / 1025 rows and a few tiles."""
import ctypes as C

import numpy as np
import pytest
from sql_session_reference import SqlSessionReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MAX = (1 << 63) - 1
REL_TOL = 1e-9

# one layout per kernel instance (accumulator words): (aggs, value types, NULL-able columns)
LAYOUTS = {
    1: ([("SUM", 0, "BIGINT")], ["BIGINT"], ()),
    2: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT")], ["BIGINT"], (0,)),
    4: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT"), ("MIN", 1, "INT"), ("COUNT_STAR", 0, "BIGINT"), ("AVG", 0, "BIGINT")],
        ["BIGINT", "INT"], (0,)),
    8: ([("SUM", 0, "BIGINT"), ("AVG", 1, "DOUBLE"), ("MIN", 2, "INT"), ("MAX", 2, "INT"), ("COUNT", 1, "DOUBLE"),
         ("COUNT_STAR", 0, "BIGINT"), ("SUM", 1, "DOUBLE")], ["BIGINT", "DOUBLE", "INT"], (0, 1, 2)),
}
# three words, rounded up to the four-word instance: the padding word folds as an add of 0
THREE = ([("SUM", 0, "BIGINT"), ("COUNT_STAR", 0, "BIGINT")], ["BIGINT"], (0,))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(gap, layout, **kw):
    from flink_amd.table import SessionWindowAggOperator
    aggs, types, nullable = layout
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return SessionWindowAggOperator(gap, aggs, types, nullable_cols=nullable, **kw).open()


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def _cols(rng, n, layout, p_null=0.3):
    """n rows of random value columns: (values per column, {column: NULL flags})"""
    _, types, nullable = layout
    vals, nulls = [], {}
    for c, t in enumerate(types):
        if t == "DOUBLE":
            vals.append(rng.uniform(0.5, 100.0, n))
        elif t == "INT":
            vals.append(rng.integers(-1000, 1000, n).astype(np.int64))
        else:
            vals.append(rng.integers(-10**12, 10**12, n).astype(np.int64))
        if c in nullable:
            nulls[c] = rng.random(n) < p_null
    return vals, nulls


def _push(k, ts, layout, rng, p_null=0.3):
    vals, nulls = _cols(rng, len(k), layout, p_null)
    return ("push", _i64(k), _i64(ts), vals, nulls)


def _ref_rows(vals, nulls, n):
    cols = [v.tolist() for v in vals]
    flags = {c: f.tolist() for c, f in nulls.items()}
    return [[None if c in flags and flags[c][i] else cols[c][i] for c in range(len(cols))] for i in range(n)]


def _order(rows):
    return sorted(rows, key=lambda r: (r[-1], r[0], r[-2]))


def _same(got, want):
    got, want = _order(got), _order(want)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for x, y in zip(g, w):
            if isinstance(y, float):
                assert x is not None and abs(x - y) <= REL_TOL * abs(y), (g, w)
            else:
                assert x == y and type(x) is type(y), (g, w)


def _slice(step, sel):
    _, k, ts, vals, nulls = step
    return ("push", k[sel], ts[sel], [v[sel] for v in vals], {c: f[sel] for c, f in nulls.items()})


def _feed(op, step, device=False, same_hash=False):
    _, k, ts, vals, nulls = step
    if device:
        import torch
        if len(k):
            op.process_batch_device(torch.tensor(k, device="cuda"), torch.tensor(ts, device="cuda"),
                                    [torch.tensor(v, device="cuda") for v in vals], None,
                                    nulls={c: torch.tensor(f.astype(np.uint8), device="cuda") for c, f in nulls.items()})
    else:  # a HOST_HASHED operator gets one hash for every key: all keys share a superbucket
        op.process_batch(k, ts, vals, np.zeros(len(k), np.int32) if same_hash else None, nulls=nulls)


def _drive(op, ref, steps, device=False, same_hash=False):
    """steps: ("push", keys, ts, value columns, {column: NULL flags}) | ("wm", w).  Every watermark's
    rows, the drop count and the live / fired counters are compared with the checker's."""
    for st in steps:
        if st[0] == "wm":
            _same(op.output_rows(op.process_watermark(st[1])), ref.process_watermark(st[1]))
            continue
        ref.process(st[1].tolist(), st[2].tolist(), _ref_rows(st[3], st[4], len(st[1])))
        _feed(op, st, device, same_hash)
    s = op.handle.stats()
    assert s["num_late_records_dropped"] == ref.late_dropped == op.num_late_records_dropped
    assert s["live_state_entries"] == ref.live_sessions() and s["num_fired_windows"] == ref.fired
    assert s["error_flags"] == 0 and s["pending_rows"] == 0 and s["current_watermark"] == ref.watermark
    return ref.fired


def _run(gap, layout, steps, device=False, **kw):
    op, ref = _op(gap, layout, **kw), SqlSessionReference(gap, layout[0])
    try:
        return _drive(op, ref, steps, device, kw.get("key_type") == "HOST_HASHED")
    finally:
        op.close()


def _stream(seed, layout, n_keys, n_pushes, per, gap):
    rng = np.random.default_rng(seed)
    steps = []
    for p in range(n_pushes):
        k = rng.integers(0, n_keys, per).astype(np.int64) * 31 - 100
        ts = _i64(p * 6 * gap + rng.integers(0, 12 * gap, per))
        ts[rng.random(per) < 1 / 16] -= 8 * gap          # stragglers: behind the watermark from the second push on
        steps.append(_push(k, ts, layout, rng))
        steps.append(("wm", p * 6 * gap + 2 * gap))      # later pushes hold late rows, joining and alone
    steps.append(("wm", LONG_MAX))
    return steps


# ---- one layout per kernel instance ------------------------------------------------------------------
@pytest.mark.parametrize("nw", sorted(LAYOUTS))
def test_layout_per_word_count(nw):
    """~3000 rows over 40 keys in one superbucket, 3 pushes with watermarks between"""
    layout = LAYOUTS[nw]
    op = _op(5, layout, key_type="HOST_HASHED")
    try:
        assert abi.host_sql_session_words(op.cfg) == nw
        ref = SqlSessionReference(5, layout[0])
        assert _drive(op, ref, _stream(100 + nw, layout, 40, 3, 1000, 5), same_hash=True) > 100
        assert ref.late_dropped > 0
    finally:
        op.close()


def test_three_words_round_up_to_four():
    assert _run(5, THREE, _stream(7, THREE, 40, 3, 1000, 5), key_type="HOST_HASHED") > 100


# ---- one hot key ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 3000])
@pytest.mark.parametrize("n_pushes", [1, 4])
def test_hot_key_one_session(n, n_pushes):
    rng = np.random.default_rng(n)
    ts = rng.permutation(n).astype(np.int64) * 3          # one session: neighbours 3 apart, gap 5
    k = np.full(n, 42, np.int64)
    whole = _push(k, ts, LAYOUTS[8], rng)
    cuts = np.linspace(0, n, n_pushes + 1).astype(int)
    steps = [_slice(whole, slice(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    steps += [("wm", 3 * n), ("wm", 3 * n + 1), ("wm", 3 * n + 2)]     # end - 1 = 3 (n - 1) + 4 = 3 n + 1
    assert _run(5, LAYOUTS[8], steps) == 1


# ---- sessions straddling tiles and pushes ---------------------------------------------------------------
@pytest.mark.parametrize("cut", [1023, 1024, 1025])
@pytest.mark.parametrize("split", [False, True])
def test_sessions_straddling_tiles_and_pushes(cut, split):
    """three alternating keys in one superbucket's arrival order; each key's sessions break where its
    row index passes ``cut`` and again 700 rows later"""
    n = 3 * 1100
    i = np.arange(n)
    per = i // 3
    ts = _i64(per * 4 + (per * 3 >= cut) * 1000 + (per * 3 >= cut + 700) * 1000)
    whole = _push(i % 3, ts, LAYOUTS[4], np.random.default_rng(cut))
    steps = [_slice(whole, slice(0, cut)), _slice(whole, slice(cut, n))] if split else [whole]
    steps += [("wm", 500), ("wm", int(ts[cut]) + 100), ("wm", LONG_MAX)]
    assert _run(4, LAYOUTS[4], steps, key_type="HOST_HASHED") == 9


# ---- late candidates ------------------------------------------------------------------------------------------
def _late_orders(order, filler, layout, rng):
    """watermark 104, gap 10: A = (95) is late alone, B = (100) is on time and reaches A.  ``filler`` rows
    of the same key, one far-away session, put the two on either side of a tile boundary."""
    a, b = (9, 95), (9, 100)
    first, second = (a, b) if order == "AB" else (b, a)
    k = [first[0]] + [9] * filler + [second[0]]
    ts = [first[1]] + (1000 + np.arange(filler)).tolist() + [second[1]]
    return [_push([9], [60], layout, rng, 0.0), ("wm", 104), _push(k, ts, layout, rng), ("wm", LONG_MAX)]


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("filler", [0, 1023])
def test_late_candidate_orders(order, filler):
    layout = LAYOUTS[8]
    op, ref = _op(10, layout, max_parallelism=1, state_capacity=1), SqlSessionReference(10, layout[0])
    try:
        _drive(op, ref, _late_orders(order, filler, layout, np.random.default_rng(filler)))
        assert ref.late_dropped == (1 if order == "AB" else 0)
    finally:
        op.close()


def test_backward_chain_of_late_candidates():
    layout, rng = LAYOUTS[4], np.random.default_rng(3)
    steps = [_push([1, 2], [0, 0], layout, rng), ("wm", 104),
             # key 1: anchor then a chain backwards; key 2: the chain without an anchor, farthest first
             _push([1, 2, 1, 2, 1, 2, 1], [100, 70, 90, 80, 80, 90, 70], layout, rng), ("wm", LONG_MAX)]
    op, ref = _op(10, layout), SqlSessionReference(10, layout[0])
    try:
        _drive(op, ref, steps)
        assert ref.late_dropped == 3
    finally:
        op.close()


def test_push_of_late_candidates_only():
    """2048 rows, all late candidates: 32 keys with a live session each; per key 32 rows chain backwards
    from it (accepted) and 32 lie a gap further back, farthest first (dropped)."""
    gap, W, layout, rng = 10, 10_000, LAYOUTS[8], np.random.default_rng(4)
    k, ts = [], []
    for key in range(32):
        for j in range(32):
            k += [key, key]
            ts += [W - 8 - gap * (j + 1), W - 5000 - gap * (32 - j)]    # the chain, nearest first; the unreachable ones
    steps = [_push(np.arange(32), np.full(32, W - 8), layout, rng), ("wm", W), _push(k, ts, layout, rng), ("wm", LONG_MAX)]
    assert len(k) == 2048 and bool(np.all(_i64(ts) + gap - 1 <= W))
    op, ref = _op(gap, layout, max_parallelism=1, state_capacity=1), SqlSessionReference(gap, layout[0])
    try:
        _drive(op, ref, steps)
        assert ref.late_dropped == 1024
    finally:
        op.close()


# ---- NULLs ------------------------------------------------------------------------------------------------------
def test_all_null_session_that_a_non_null_row_joins():
    layout = LAYOUTS[4]
    null = {0: np.array([True])}

    def row(k, ts, v, isnull):
        return ("push", _i64([k]), _i64([ts]), [_i64([v]), _i64([5])], {0: np.array([isnull])})
    steps = [row(1, 0, 111, True), row(1, 5, 222, True), row(2, 0, 333, True),
             ("wm", 3),                                  # nothing is due: the NULL rows opened live sessions
             row(1, 9, 7, False),                        # joins key 1's all-NULL session
             ("wm", LONG_MAX)]
    op, ref = _op(10, layout), SqlSessionReference(10, layout[0])
    try:
        op.process_batch(*row(1, 0, 111, True)[1:4], nulls=null)      # (the same first step, by hand)
        ref.process([1], [0], [[None, 5]])
        assert op.handle.stats()["live_state_entries"] == 1
        _drive(op, ref, steps[1:])
        assert ref.fired == 2
    finally:
        op.close()
    rows = SqlSessionReference(10, layout[0])
    for st in steps:
        if st[0] == "push":
            rows.process(st[1].tolist(), st[2].tolist(), _ref_rows(st[3], st[4], 1))
    out = rows.process_watermark(LONG_MAX)
    # SUM, COUNT(col), MIN(other), COUNT(*), AVG: key 1 took the 7, key 2 stays NULL / 0
    assert out == [(2, None, 0, 5, 1, None, 0, 10), (1, 7, 1, 5, 3, 7, 0, 19)]


# ---- device-resident columns ----------------------------------------------------------------------------------
def test_device_columns_with_null_flags():
    layout = LAYOUTS[8]
    assert _run(5, layout, _stream(21, layout, 30, 3, 1100, 5), device=True) > 100


# ---- sharding --------------------------------------------------------------------------------------------------
def _dest(keys, p):
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_BINROW_BIGINT, 128, p, None,
                                                          d.ctypes.data))
    return d


def _run_sharded(ops, ref, steps):
    for s in steps:
        if s[0] == "push":
            d = _dest(s[1], len(ops))
            ref.process(s[1].tolist(), s[2].tolist(), _ref_rows(s[3], s[4], len(s[1])))
            for i, op in enumerate(ops):
                _feed(op, _slice(s, d == i))
        else:
            parts = [op.output_rows(op.process_watermark(s[1])) for op in ops]
            _same([r for p in parts for r in p], ref.process_watermark(s[1]))
            keys = [{r[0] for r in p} for p in parts]
            assert len(set().union(*keys)) == sum(len(x) for x in keys)      # no key fired by two subtasks


def test_binrow_keys_over_two_subtasks():
    layout = LAYOUTS[4]
    steps = _stream(29, layout, 300, 3, 2000, 5)
    ref = SqlSessionReference(5, layout[0])
    ops = [_op(5, layout, parallelism=2, subtask_index=i) for i in range(2)]
    try:
        _run_sharded(ops, ref, steps)
        assert sum(op.num_late_records_dropped for op in ops) == ref.late_dropped > 0
        assert all(op.handle.stats()["error_flags"] == 0 for op in ops)
        assert all(op.handle.stats()["num_fired_windows"] > 0 for op in ops)
    finally:
        for op in ops:
            op.close()


# ---- checkpoint -------------------------------------------------------------------------------------------------
def test_snapshot_restore_mid_session():
    layout = LAYOUTS[8]
    steps = _stream(31, layout, 200, 5, 1200, 5)
    ref = SqlSessionReference(5, layout[0])
    a, b = _op(5, layout, state_capacity=1 << 12), None
    try:
        _drive(a, ref, steps[:5])                  # stops behind a push: sessions are open
        blob = a.snapshot_state()
        a.close()
        b = _op(5, layout, state_capacity=1 << 18)      # another superbucket split
        b.initialize_state(blob)
        st = b.handle.stats()
        assert st["live_state_entries"] == ref.live_sessions() > 0 and b.current_watermark == ref.watermark
        ref.fired = ref.late_dropped = 0                # counters are not part of the blob
        _drive(b, ref, steps[5:])
        assert b.handle.stats()["live_state_entries"] == 0
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("src,dst", [(1, 2), (2, 1)])
def test_key_group_snapshots_rescale(src, dst):
    layout = LAYOUTS[4]
    steps = _stream(37, layout, 300, 4, 1500, 5)
    ref = SqlSessionReference(5, layout[0])
    olds = [_op(5, layout, parallelism=src, subtask_index=i) for i in range(src)]
    news = []
    try:
        _run_sharded(olds, ref, steps[:5])
        blobs = {}
        for op in olds:
            blobs.update(op.handle.snapshot_key_groups()[0])
        assert len(blobs) == 128
        for op in olds:
            op.close()
        news = [_op(5, layout, parallelism=dst, subtask_index=i) for i in range(dst)]
        for op in news:
            op.handle.restore_key_groups(blobs, [])
            op.handle.initialize_watermark(ref.watermark)
        assert sum(op.handle.stats()["live_state_entries"] for op in news) == ref.live_sessions() > 0
        _run_sharded(news, ref, steps[5:])
        assert all(op.handle.stats()["error_flags"] == 0 and op.handle.stats()["live_state_entries"] == 0 for op in news)
    finally:
        for op in olds + news:
            op.close()


def test_cross_restore_is_refused():
    from flink_amd.datastream import SessionWindowOperator
    layout = LAYOUTS[2]
    a = _op(5, layout)
    others = []
    try:
        _feed(a, _push([1, 2, 3], [0, 1, 2], layout, np.random.default_rng(1)))
        blob = a.snapshot_state()
        # another aggregate list of the same word count, another NULL-able set, another gap
        others = [_op(5, ([("SUM", 0, "BIGINT"), ("COUNT_STAR", 0, "BIGINT")], ["BIGINT"], ())),
                  _op(5, (layout[0], layout[1], ())), _op(6, layout)]
        for o in others:
            with pytest.raises(_native.FlinkWinError, match="different operator configuration") as e:
                o.initialize_state(blob)
            assert e.value.code == abi.FW_E_INVALID
        ds = SessionWindowOperator(5, ("sum", "LONG"), max_batch_rows=1 << 14, output_capacity=1 << 16).open()
        others.append(ds)
        with pytest.raises(_native.FlinkWinError, match="different operator configuration"):
            ds.initialize_state(blob)
        ds.process_batch(_i64([1]), _i64([0]), _i64([5]))
        with pytest.raises(_native.FlinkWinError, match="different operator configuration"):   # and the other way round
            a.initialize_state(ds.snapshot_state())
        b = _op(5, layout)
        others.append(b)
        b.initialize_state(blob)                        # the same configuration takes it
        assert b.handle.stats()["live_state_entries"] == 3
    finally:
        a.close()
        for o in others:
            o.close()


# ---- capacity ---------------------------------------------------------------------------------------------------
def test_output_capacity():
    layout, rng = LAYOUTS[4], np.random.default_rng(5)
    op = _op(1, layout, output_capacity=16)
    try:
        for i in range(3):      # collected in time: clean
            _feed(op, _push(np.arange(10), np.full(10, 100 * i), layout, rng))
            assert len(op.process_watermark(100 * i + 50)["key"]) == 10
        assert op.handle.stats()["error_flags"] == 0
        _feed(op, _push(np.arange(40), np.full(40, 1000), layout, rng))
        with pytest.raises(_native.FlinkWinError) as e:
            op.process_watermark(2000)      # 40 fires
        assert e.value.code == abi.FW_E_CAPACITY
        assert op.handle.stats()["error_flags"] & abi.ERRF["OUTPUT"]
    finally:
        op.close()


def test_state_capacity_leaves_the_state_unchanged():
    """one superbucket of 1024 sessions (HOST_HASHED keys sharing a hash): a tile whose sessions do not
    fit raises FW_ERRF_STATE and is dropped whole; the list is as it was and later pushes fold correctly"""
    layout, rng = LAYOUTS[8], np.random.default_rng(6)
    op = _op(10, layout, key_type="HOST_HASHED", state_capacity=1, max_parallelism=1)
    ref = SqlSessionReference(10, layout[0])
    try:
        first = _push(np.arange(1000), np.zeros(1000), layout, rng)
        ref.process(first[1].tolist(), first[2].tolist(), _ref_rows(first[3], first[4], 1000))
        _feed(op, first, same_hash=True)
        st = op.handle.stats()
        assert st["superbucket_capacity"] == 1024 and st["live_state_entries"] == 1000 and st["error_flags"] == 0
        _feed(op, _push(np.arange(2000, 2100), np.zeros(100), layout, rng), same_hash=True)      # 1100 sessions: dropped
        st = op.handle.stats()
        assert st["error_flags"] & abi.ERRF["STATE"] and st["live_state_entries"] == 1000
        more = _push(np.arange(0, 40) % 20, np.full(40, 8), layout, rng)      # rows that join held sessions still fold
        ref.process(more[1].tolist(), more[2].tolist(), _ref_rows(more[3], more[4], 40))
        _feed(op, more, same_hash=True)
        assert op.handle.stats()["live_state_entries"] == 1000
        held = op.snapshot_state()
        with pytest.raises(_native.FlinkWinError) as e:      # the flag turns the next collection into FW_E_CAPACITY
            op.process_watermark(LONG_MAX)
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()
    # the same pushes without the dropped tile, on a fresh handle: the sessions the first handle held
    # (one superbucket, the same tiles: the entries behind the 48-byte header are the same bytes)
    op = _op(10, layout, key_type="HOST_HASHED", state_capacity=1, max_parallelism=1)
    try:
        _feed(op, first, same_hash=True)
        _feed(op, more, same_hash=True)
        assert op.snapshot_state()[48:] == held[48:] and len(held) == 48 + 1000 * (3 + 8 + 1) * 8
        _same(op.output_rows(op.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
        assert ref.fired == 1000
    finally:
        op.close()


# ---- refused calls -----------------------------------------------------------------------------------------------
def test_calls_a_sql_session_handle_refuses():
    import torch
    layout = LAYOUTS[2]
    op, ref = _op(10, layout), SqlSessionReference(10, layout[0])
    try:
        h, L = op.handle, _native.lib()
        st = _push([1], [0], layout, np.random.default_rng(2), 0.0)
        _feed(op, st)
        ref.process([1], [0], _ref_rows(st[3], st[4], 1))
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
        vals = (C.c_void_p * 8)(wm.data_ptr())
        # a NULL-able column without its null-flag column
        assert L.fw_push_device(h._h, 1, wm.data_ptr(), wm.data_ptr(), None, vals, None) == abi.FW_E_INVALID
        assert "null-flag" in L.fw_last_error().decode()
        with pytest.raises(_native.FlinkWinError):      # SQL has no late side output
            h.late_records()
        r = abi.fw_result()
        _native.check(L.fw_results(h._h, C.byref(r), 1))
        assert r.n == 0 and not r.first_ord
        _same(op.output_rows(op.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))      # still usable
    finally:
        op.close()
