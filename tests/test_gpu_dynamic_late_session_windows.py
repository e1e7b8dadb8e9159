"""Dynamic-gap session windows with an allowed lateness (FW_WIN_SESSION_DYNAMIC_LATENESS) on the GPU
against the element-by-element reference (dynamic_late_session_reference.py).  After every push,
collect() -- the rows late elements fired at once -- and after every watermark the timer rows are
compared as multisets, bit-exact; the drops, the late side output and the counters with them.

A tile holds 1024 rows; the main stream's pushes sit at 1023 / 1024 / 1025 / 3000 / 37 / 2048 rows
(dynamic_late_session_streams.py; test_dynamic_late_session_host.py counts what the stream reaches).

The capacity contract of the folded paths, restated for this kind (tests/folded_capacity_cases.py
states it for the others): a push is cut into tiles of 1024 rows in arrival order per superbucket; a
tile whose merged list would exceed the superbucket's capacity is dropped whole and FW_ERRF_STATE is
raised, the list stays as it was, bit for bit; what the tile's arrival-order walk did before the
decision -- late drops counted, rows fired at once -- stays.  An output row at or past
output_capacity is not written and raises FW_ERRF_OUTPUT; the results call then refuses."""
import struct

import numpy as np
import pytest
from dynamic_late_session_reference import DynamicLateSessionReference
from dynamic_late_session_streams import (HOT_LATENESS, HOT_MAX_GAP, LATENESS, MAX_GAP, N_KEYS, hot_key_stream, main_stream,
                                          value_words)
from test_dynamic_late_session_host import WORKED, WORKED_LATENESS, WORKED_MAX_GAP

import session_exchange_order as order
from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
STATE, OUTPUT, GAPF = abi.ERRF["STATE"], abi.ERRF["OUTPUT"], abi.ERRF["GAP"]
SW_HEADER = 48


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(max_gap, lateness, agg=("sum", "LONG"), **kw):
    from flink_amd.datastream import LateDynamicSessionWindowOperator
    kw.setdefault("max_batch_rows", 4096)
    kw.setdefault("output_capacity", 1 << 14)
    return LateDynamicSessionWindowOperator(max_gap, lateness, agg, **kw).open()


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _wmt(w):
    import torch
    return torch.tensor([w], dtype=torch.int64, device="cuda")


def _rows(res):
    return list(zip([k if isinstance(k, str) else int(k) for k in res["key"]], res["value"].tolist(),
                    res["window_start"].tolist(), res["window_end"].tolist()))


def _same(got, want):
    """rows (key, value, start, end) as multisets, bit-exact"""
    def key(r):
        return (r[3], str(r[0]), r[2], r[1])
    assert sorted(got, key=key) == sorted((tuple(w) for w in want), key=key)


def _push(op, k, ts, v, g, device=False, hashed=False):
    if device:
        op.process_batch_device(_dev(k), _dev(ts), _dev(v), _dev(g))
    else:
        op.process_batch(k, ts, v, g, np.zeros(len(k), np.int32) if hashed else None)


def _drive(op, ref, pushes, agg=("sum", "LONG"), device=False, device_wm=False, side=False, hashed=False, seq=0):
    for k, ts, v, g, wm in pushes:
        late, at_once = ref.process(k.tolist(), ts.tolist(), value_words(v), g.tolist())
        _push(op, k, ts, v, g, device, hashed)
        _same(_rows(op.collect()), at_once)
        if side:
            lr = op.late_records()
            assert sorted(zip(lr["push_seq"].tolist(), lr["row"].tolist())) == [(seq, i) for i in late]
            assert sorted(zip(lr["row"].tolist(), lr["ts"].tolist(), lr["key"].tolist())) == [(i, int(ts[i]), int(k[i])) for i in late]
            if agg[0] != "count":      # (a count reads no value column)
                words = value_words(v)
                assert sorted(zip(lr["row"].tolist(), lr["value"].tolist())) == [(i, words[i]) for i in late]
        seq += 1
        if wm is not None:
            got = op.process_watermark_device(_wmt(wm)) if device_wm else op.process_watermark(wm)
            _same(_rows(got), ref.process_watermark(wm))
    return seq


def _stats(op, ref, flags=0):
    s = op.handle.stats()
    assert (s["live_state_entries"], s["num_fired_windows"], s["num_late_records_dropped"], s["current_watermark"], s["error_flags"]) == \
        (ref.live_sessions(), ref.fired, ref.late_dropped, ref.watermark, flags)
    return s


# ---- the worked case ------------------------------------------------------------------------------
def test_worked_case_with_string_keys_and_a_restore():
    """key 7 as the String "k7", largest gap 100, lateness 50 (test_dynamic_late_session_host.py's
    table); a snapshot after watermark 1310 restored into a second operator: [1300, 1305) comes back
    as a fired session, read off the blob's watermark"""
    ops = [_op(WORKED_MAX_GAP, WORKED_LATENESS, key_type="STRING")]
    ref = DynamicLateSessionReference(WORKED_LATENESS)

    def named(row):
        return ("k7",) + tuple(row[1:])
    try:
        for step in WORKED:
            op = ops[-1]
            if step[0] == "push":
                _, ts, g, v, kept, row = step
                assert ref.add(7, ts, v, g) == (kept, row)
                op.process_batch(["k7"], [ts], [v], [g])
                assert _rows(op.collect()) == ([named(row)] if row else [])
            elif step[0] == "wm":
                assert ref.process_watermark(step[1]) == step[2]
                assert _rows(op.process_watermark(step[1])) == [named(r) for r in step[2]]
                if step[1] == 1310:
                    assert op.handle.stats()["live_state_entries"] == 1      # fired and retained
                    blob = op.snapshot_state()
                    op.close()
                    ops.append(_op(WORKED_MAX_GAP, WORKED_LATENESS, key_type="STRING"))
                    ops[-1].initialize_state(blob)
                    s = ops[-1].handle.stats()
                    assert s["current_watermark"] == 1310 and s["live_state_entries"] == 1
            else:
                assert op.handle.stats()["live_state_entries"] == len(step[1])
        s = ops[-1].handle.stats()   # the second operator: six rows at once and one timer row; one drop
        assert (s["live_state_entries"], s["num_late_records_dropped"], s["num_fired_windows"], s["error_flags"]) == (0, 1, 7, 0)
        assert ref.fired == 9 and ref.late_dropped == 1
    finally:
        for op in ops:
            op.close()


# ---- the main stream ------------------------------------------------------------------------------
def _own_keys(n):
    """n LONG keys of subtask 0's key groups at parallelism 2 of 128"""
    cand = np.arange(1, 40 * n, dtype=np.int64) * 7919 + 13
    own = cand[order.destinations(cand, abi.KEYHASH_LONG, 128, 2) == 0][:n]
    assert len(own) == n
    return own


@pytest.mark.parametrize("form", ["host_wm", "device_wm"])
@pytest.mark.parametrize("agg", [("sum", "LONG"), ("sum", "INT"), ("min", "DOUBLE"), ("count", "LONG")], ids=lambda a: "-".join(a))
def test_main_stream(agg, form):
    """host_wm: k_sw_fold<1, true, false, true> behind host pushes and host watermarks; device_wm: a
    handle of parallelism 2 that holds every key of the stream, device pushes and the watermark of
    record on the device from the start, so every fold is k_sw_fold<1, true, true, true>"""
    pushes = main_stream(ftype=agg[1])
    ref = DynamicLateSessionReference(LATENESS, agg)
    if form == "device_wm":
        own = _own_keys(N_KEYS)
        pushes = [(own[k], ts, v, g, wm) for k, ts, v, g, wm in pushes]
        op = _op(MAX_GAP, LATENESS, agg, late_side_output=True, parallelism=2, subtask_index=0)
    else:
        op = _op(MAX_GAP, LATENESS, agg, late_side_output=True)
    try:
        dev = form == "device_wm"
        if dev:
            assert _rows(op.process_watermark_device(_wmt(LONG_MIN))) == []
        _drive(op, ref, pushes, agg, device=dev, device_wm=dev, side=True)
        assert ref.counts["fired_at_once"] >= 20 and ref.counts["dropped"] >= 20 and ref.counts["cleaned_silent"] >= 20
        _stats(op, ref)
        _same(_rows(op.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
        assert _stats(op, ref)["live_state_entries"] == 0
    finally:
        op.close()


def test_main_stream_in_one_superbucket():
    """HOST_HASHED with one hash for every key: all 40 keys in one list, tiles in arrival order"""
    op, ref = _op(MAX_GAP, LATENESS, key_type="HOST_HASHED", late_side_output=True), DynamicLateSessionReference(LATENESS)
    try:
        _drive(op, ref, main_stream(), side=True, hashed=True)
        _stats(op, ref)
    finally:
        op.close()


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_hot_key_over_three_tiles_pins_the_arrival_order(reverse):
    """several late rows of one batch land in one fired session: every row fires it again with the
    rows before it, so the rows depend on the arrival order (the reversed batch gives other rows:
    test_dynamic_late_session_host.py)"""
    op, ref = _op(HOT_MAX_GAP, HOT_LATENESS, key_type="HOST_HASHED"), DynamicLateSessionReference(HOT_LATENESS)
    try:
        _drive(op, ref, hot_key_stream(reverse), hashed=True)
        assert ref.counts["fired_at_once"] >= 100 and ref.counts["dropped"] >= 20
        _stats(op, ref)
    finally:
        op.close()


# ---- the two lower bounds ---------------------------------------------------------------------------
@pytest.mark.parametrize("device_wm", [False, True], ids=["host_wm", "device_wm"])
def test_short_gap_fire_is_not_skipped(device_wm):
    """One row of gap 5 under a largest gap of 400, pushed as no candidate.  Its timer is at ts + 4; a
    min_fire taken from ts + 400 would let the advance to a watermark between ts + 4 and ts + 399
    return early.  It fires in that advance; a second advance to its cleanup time removes it without a
    row."""
    kw = dict(parallelism=2, subtask_index=0) if device_wm else {}
    op, ref = _op(400, 1000, **kw), DynamicLateSessionReference(1000)
    key = int(_own_keys(1)[0])

    def wm(w):
        got = op.process_watermark_device(_wmt(w)) if device_wm else op.process_watermark(w)
        want = ref.process_watermark(w)
        _same(_rows(got), want)
        return want
    try:
        assert wm(1000) == []
        _drive(op, ref, [(_i64([key]), _i64([2000]), _i64([7]), _i64([5]), None)], device=device_wm)
        assert _stats(op, ref)["live_state_entries"] == 1 and ref.fired == 0
        assert wm(2003) == []
        assert wm(2100) == [(key, 7, 2000, 2005)]          # 2004 <= 2100 < 2399
        assert _stats(op, ref)["live_state_entries"] == 1    # retained
        assert wm(3003) == [] and _stats(op, ref)["live_state_entries"] == 1
        assert wm(3004) == [] and _stats(op, ref)["live_state_entries"] == 0     # 2004 + 1000: removed, no row
        assert ref.counts["cleaned_silent"] == 1 and ref.fired == 1
    finally:
        op.close()


def test_short_window_inside_an_unfired_long_one_keeps_the_bounds_low_enough():
    """a long and a short row of other keys in one superbucket: the short one's timer is the smaller"""
    op, ref = _op(400, 50, key_type="HOST_HASHED"), DynamicLateSessionReference(50)
    try:
        _drive(op, ref, [(_i64([1, 2, 1]), _i64([2000, 2100, 2010]), _i64([1, 2, 4]), _i64([400, 5, 5]), 2104)], hashed=True)
        assert ref.fired == 1 and _stats(op, ref)["live_state_entries"] == 2
        _same(_rows(op.process_watermark(2154)), ref.process_watermark(2154))       # [2100, 2105) is cleaned
        assert _stats(op, ref)["live_state_entries"] == 1
        _same(_rows(op.process_watermark(2399)), ref.process_watermark(2399))
        assert ref.fired == 2
    finally:
        op.close()


# ---- gaps out of range on the device path --------------------------------------------------------------
def test_out_of_range_gaps_on_the_device_path():
    rng = np.random.default_rng(31)
    n = 2100      # three tiles of the one superbucket
    k = _i64(rng.integers(0, 20, n))
    ts = _i64(rng.integers(0, 5000, n))
    v = _i64(rng.integers(-1000, 1000, n))
    g = _i64([3, 20, 60, 400])[rng.integers(0, 4, n)].copy()
    bad = rng.random(n) < 0.05
    g[bad] = _i64([0, -1, 401])[rng.integers(0, 3, int(bad.sum()))]
    g[:3], bad[:3] = [0, 401, -1], True
    ok = ~bad
    ref = DynamicLateSessionReference(300)
    ref.process_watermark(2500)      # half of the rows are late candidates; the oldest are dropped
    late, at_once = ref.process(k[ok].tolist(), ts[ok].tolist(), v[ok].tolist(), g[ok].tolist())
    assert len(late) >= 20 and len(at_once) >= 20
    a, b = _op(400, 300, max_parallelism=1, state_capacity=1), None
    try:
        a.process_watermark(2500)
        with pytest.raises(ValueError, match="0 < gap"):      # the host path checks before it pushes
            a.process_batch(k, ts, v, g)
        assert a.handle.stats()["live_state_entries"] == 0
        a.process_batch_device(_dev(k), _dev(ts), _dev(v), _dev(g))
        _stats(a, ref, GAPF)          # nothing of the bad rows: not held, not dropped, not fired
        with pytest.raises(ValueError, match="0 < gap"):
            a.process_watermark(LONG_MAX)
        # the state holds the valid rows' sessions: a whole restore clears the flags, as after a restart
        blob = a.snapshot_state()
        a.close()
        b = _op(400, 300, max_parallelism=1, state_capacity=1)
        b.initialize_state(blob)
        assert b.handle.stats()["current_watermark"] == 2500
        _same(_rows(b.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- capacity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1], ids=["fills", "one_past"])
def test_retained_sessions_fill_the_list(extra):
    """cap_s = 64 (the smallest; one superbucket).  60 sessions of mixed gaps fire and are retained; a
    tile of 4 + ``extra`` new sessions makes 64 -- fits -- or 65: the tile is dropped, the list as it
    was."""
    op, ref = _op(400, 10**6, key_type="HOST_HASHED", state_capacity=1, output_capacity=64), DynamicLateSessionReference(10**6)
    try:
        assert op.handle.stats()["superbucket_capacity"] == 64
        k, ts, g = _i64(np.arange(60) % 7), _i64(1000 * np.arange(60)), _i64([5, 50, 400])[np.arange(60) % 3]
        _drive(op, ref, [(k, ts, _i64(np.arange(60) + 1), g, 60000)], hashed=True)
        assert _stats(op, ref)["live_state_entries"] == 60 and ref.fired == 60
        held = op.snapshot_state()
        n = 4 + extra
        tile = (_i64(np.arange(n)), _i64(100000 + 1000 * np.arange(n)), _i64(np.ones(n)), _i64(np.full(n, 7)))
        _push(op, *tile, hashed=True)
        if not extra:
            assert _rows(op.collect()) == []
            ref.process(tile[0].tolist(), tile[1].tolist(), tile[2].tolist(), tile[3].tolist())
            assert _stats(op, ref)["live_state_entries"] == 64
            # a late row into a retained session still fires it: the full list takes merges
            _drive(op, ref, [(_i64([3]), _i64([3002]), _i64([7]), _i64([2]), None)], hashed=True)
            assert ref.counts["fired_at_once"] == 1
            _same(_rows(op.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX))
            assert _stats(op, ref)["live_state_entries"] == 0
        else:
            assert _stats(op, ref, STATE)["live_state_entries"] == 60
            assert op.snapshot_state()[SW_HEADER:] == held[SW_HEADER:]      # bit for bit
            with pytest.raises(_native.FlinkWinError) as e:
                op.process_watermark(60001)
            assert e.value.code == abi.FW_E_CAPACITY
            op.initialize_state(held)                                        # a restore clears the flag
            assert _stats(op, ref)["live_state_entries"] == 60
    finally:
        op.close()


@pytest.mark.parametrize("n_late", [4, 5], ids=["exactly", "one_past"])
def test_immediate_fires_at_the_output_capacity(n_late):
    """output_capacity = 64: 60 timer rows uncollected, then 4 or 5 rows fired at once"""
    op, ref = _op(400, 10**6, output_capacity=64), DynamicLateSessionReference(10**6)
    try:
        k, ts, g = _i64(np.arange(60)), _i64(1000 * np.arange(60)), _i64([5, 50, 400])[np.arange(60) % 3]
        ref.process(k.tolist(), ts.tolist(), [1] * 60, g.tolist())
        _push(op, k, ts, _i64(np.ones(60)), g)
        op.handle.advance(60000)                      # 60 rows wait in the result buffer
        want = ref.process_watermark(60000)
        late = (_i64(np.arange(n_late)), _i64(1000 * np.arange(n_late) + 3), _i64(np.full(n_late, 5)), _i64(np.full(n_late, 2)))
        _, at_once = ref.process(late[0].tolist(), late[1].tolist(), late[2].tolist(), late[3].tolist())
        assert len(at_once) == n_late
        _push(op, *late)
        s = op.handle.stats()
        assert s["num_fired_windows"] == ref.fired == 60 + n_late and s["results_available"] == min(64, 60 + n_late)
        if n_late == 4:
            assert s["error_flags"] == 0
            _same(_rows(op.collect()), want + at_once)
        else:
            assert s["error_flags"] == OUTPUT
            with pytest.raises(_native.FlinkWinError) as e:
                op.collect()
            assert e.value.code == abi.FW_E_CAPACITY
        assert s["live_state_entries"] == ref.live_sessions() == 60
    finally:
        op.close()


# ---- key-group snapshots ------------------------------------------------------------------------------
def _dest(keys, p):
    return order.destinations(keys, abi.KEYHASH_LONG, 128, p)


@pytest.mark.parametrize("dst", [1, 3])
def test_key_group_snapshot_with_fired_sessions_rescales(dst):
    pushes = main_stream()
    ref = DynamicLateSessionReference(LATENESS)
    old, news = _op(MAX_GAP, LATENESS), []
    try:
        _drive(old, ref, pushes[:3])
        wm = ref.watermark
        fired = [(s, e) for _, s, e, _ in ref.sessions() if e - 1 <= wm]
        assert len(fired) >= 20                                          # fired and retained at the cut
        assert ref.inside_held >= 100                                    # ... and sessions that contain shorter windows
        blobs = old.handle.snapshot_key_groups()[0]
        assert len(blobs) == 128 and all(struct.unpack_from("<q", b, 16)[0] == wm for b in blobs.values())
        live_blob = next(b for b in blobs.values() if len(b) > SW_HEADER)
        old.close()
        news = [_op(MAX_GAP, LATENESS, parallelism=dst, subtask_index=i) for i in range(dst)]
        # a key group at another watermark is refused: the handle stands at Long.MIN_VALUE, then one past
        for w in (None, wm + 1):
            if w is not None:
                news[0].handle.initialize_watermark(w)
            lo, hi = news[0].handle.key_group_range()
            mine = next(b for kg, b in blobs.items() if lo <= kg <= hi and len(b) > SW_HEADER)
            with pytest.raises(_native.FlinkWinError, match=str(wm)) as e:
                news[0].handle.restore_key_group_blob(mine)
            assert e.value.code == abi.FW_E_STATE and news[0].handle.stats()["live_state_entries"] == 0
        for op in news:
            op.handle.initialize_watermark(wm)
            op.handle.restore_key_groups(blobs, [])
        assert sum(op.handle.stats()["live_state_entries"] for op in news) == ref.live_sessions()
        fired0 = ref.fired
        for k, ts, v, g, w in pushes[3:]:
            d = _dest(k, dst)
            _, at_once = ref.process(k.tolist(), ts.tolist(), v.tolist(), g.tolist())
            got = []
            for i, op in enumerate(news):
                _push(op, k[d == i], ts[d == i], v[d == i], g[d == i])
                got += _rows(op.collect())
            _same(got, at_once)
            _same([r for op in news for r in _rows(op.process_watermark(w))], ref.process_watermark(w))
        _same([r for op in news for r in _rows(op.process_watermark(LONG_MAX))], ref.process_watermark(LONG_MAX))
        st = [op.handle.stats() for op in news]
        assert sum(s["num_fired_windows"] for s in st) == ref.fired - fired0 and all(s["error_flags"] == 0 for s in st)
        assert sum(s["live_state_entries"] for s in st) == 0 and ref.counts["fired_at_once"] >= 20
        # blobs cross neither kinds nor latenesses nor largest gaps
        for other in _others(MAX_GAP, LATENESS):
            try:
                other.handle.initialize_watermark(wm)
                with pytest.raises(_native.FlinkWinError, match="different operator configuration") as e:
                    other.handle.restore_key_group_blob(live_blob)
                assert e.value.code == abi.FW_E_INVALID
            finally:
                other.close()
    finally:
        old.close()
        for op in news:
            op.close()


def _others(max_gap, lateness):
    """handles a FW_WIN_SESSION_DYNAMIC_LATENESS blob of (max_gap, lateness) must not restore into"""
    from flink_amd.datastream import DynamicSessionWindowOperator, LateSessionWindowOperator
    kw = dict(max_batch_rows=4096, output_capacity=1 << 14)
    yield DynamicSessionWindowOperator(max_gap, ("sum", "LONG"), **kw).open()
    yield LateSessionWindowOperator(max_gap, lateness, ("sum", "LONG"), **kw).open()
    yield _op(max_gap, lateness + 1)
    yield _op(max_gap + 1, lateness)


def test_whole_blob_of_another_kind_lateness_or_largest_gap_is_refused():
    a = _op(MAX_GAP, LATENESS)
    try:
        a.process_batch(_i64([1, 2]), _i64([0, 1000]), _i64([1, 1]), _i64([5, 400]))
        blob = a.snapshot_state()
        for other in _others(MAX_GAP, LATENESS):
            try:
                with pytest.raises(_native.FlinkWinError, match="different operator configuration") as e:
                    other.initialize_state(blob)
                assert e.value.code == abi.FW_E_INVALID
                with pytest.raises(_native.FlinkWinError, match="different operator configuration"):      # and the other way
                    a.initialize_state(other.snapshot_state())
            finally:
                other.close()
    finally:
        a.close()
