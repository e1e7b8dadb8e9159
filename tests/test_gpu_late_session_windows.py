"""Session windows with an allowed lateness (FW_WIN_SESSION_LATENESS) on the GPU against the
element-by-element reference (late_session_reference.py).  After every push, collect() -- the rows
late elements fired at once -- and after every watermark the timer rows are compared as multisets;
the drops, the late side output and the counters with them.

Integers and DOUBLE min / max compare exactly, DOUBLE sums at the project's REL_TOL.  A tile holds
1024 rows; the main stream's pushes sit at 1023 / 1024 / 1025 / 3000 / 37 / 2048 rows
(late_session_streams.py; test_late_session_host.py counts what the stream reaches).

The capacity contract of the folded paths, restated for this kind (tests/folded_capacity_cases.py
states it for the others): a push is cut into tiles of 1024 rows in arrival order per superbucket; a
tile whose merged list would exceed the superbucket's capacity is dropped whole and FW_ERRF_STATE is
raised, the list stays as it was, bit for bit; what the tile's arrival-order walk did before the
decision -- late drops counted, rows fired at once -- stays.  An output row at or past
output_capacity is not written and raises FW_ERRF_OUTPUT; the results call then refuses."""
import struct

import numpy as np
import pytest
from late_session_reference import LateSessionReference
from late_session_streams import GAP, HOT_GAP, HOT_LATENESS, LATENESS, hot_key_stream, main_stream, value_words
from parity_common import REL_TOL
from session_window_reference import SessionWindowReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

LONG_MAX = (1 << 63) - 1
STATE, OUTPUT = abi.ERRF["STATE"], abi.ERRF["OUTPUT"]
SW_HEADER = 48


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(gap, lateness, agg=("sum", "LONG"), **kw):
    from flink_amd.datastream import LateSessionWindowOperator
    kw.setdefault("max_batch_rows", 4096)
    kw.setdefault("output_capacity", 1 << 14)
    return LateSessionWindowOperator(gap, lateness, agg, **kw).open()


def _rows(res):
    return list(zip([k if isinstance(k, str) else int(k) for k in res["key"]], res["value"].tolist(),
                    res["window_start"].tolist(), res["window_end"].tolist()))


def _same(got, want, agg=("sum", "LONG")):
    """rows (key, value, start, end) as multisets"""
    def key(r):
        return (r[3], str(r[0]), r[2], r[1])
    if agg == ("sum", "DOUBLE"):
        def key(r):     # noqa: F811 -- values of one session's rows differ by more than the tolerance
            return (r[3], str(r[0]), r[2], np.int64(r[1]).view(np.float64))
    got, want = sorted(got, key=key), sorted((tuple(w) for w in want), key=key)
    assert len(got) == len(want), (len(got), len(want))
    if agg == ("sum", "DOUBLE"):
        assert [(g[0],) + g[2:] for g in got] == [(w[0],) + w[2:] for w in want]
        np.testing.assert_allclose(np.array([g[1] for g in got], np.int64).view(np.float64),
                                   np.array([w[1] for w in want], np.int64).view(np.float64), rtol=REL_TOL, atol=0)
    else:
        assert got == want


def _push(op, k, ts, v, device=False, hashed=False):
    import torch
    if device:
        vv = np.ascontiguousarray(v)
        op.process_batch_device(torch.from_numpy(np.ascontiguousarray(k)).cuda(), torch.from_numpy(np.ascontiguousarray(ts)).cuda(),
                                torch.from_numpy(vv).cuda())
    else:
        op.process_batch(k, ts, v, np.zeros(len(k), np.int32) if hashed else None)


def _drive(op, ref, pushes, agg=("sum", "LONG"), device=False, side=False, hashed=False, seq=0):
    for k, ts, v, wm in pushes:
        late, at_once = ref.process(k.tolist(), ts.tolist(), value_words(v))
        _push(op, k, ts, v, device, hashed)
        _same(_rows(op.collect()), at_once, agg)
        if side:
            lr = op.late_records()
            assert sorted(zip(lr["push_seq"].tolist(), lr["row"].tolist())) == [(seq, i) for i in late]
            assert sorted(zip(lr["row"].tolist(), lr["ts"].tolist())) == [(i, int(ts[i])) for i in late]
            if agg[0] != "count":      # (a count reads no value column)
                words = value_words(v)
                assert sorted(zip(lr["row"].tolist(), lr["value"].tolist())) == [(i, words[i]) for i in late]
        seq += 1
        if wm is not None:
            _same(_rows(op.process_watermark(wm)), ref.process_watermark(wm), agg)
    return seq


def _stats(op, ref, flags=0):
    s = op.handle.stats()
    assert (s["live_state_entries"], s["num_fired_windows"], s["num_late_records_dropped"], s["current_watermark"], s["error_flags"]) == \
        (ref.live_sessions(), ref.fired, ref.late_dropped, ref.watermark, flags)
    return s


# ---- the worked case ------------------------------------------------------------------------------
def test_worked_case_with_string_keys_and_a_restore():
    """key A, gap 3, lateness 5 (the worked case of test_late_session_host.py); a snapshot after wm 4 restored into a second
    operator: [0, 5) comes back as a fired session, read off the blob's watermark"""
    a, b = _op(3, 5, key_type="STRING"), None
    ref = LateSessionReference(3, 5)

    def push(op, ts, v, kept, row):
        assert ref.add("A", ts, v) == (kept, row)
        op.process_batch(["A"], [ts], [v])
        assert _rows(op.collect()) == ([row] if row else [])

    def wm(op, w, rows):
        assert ref.process_watermark(w) == rows
        assert _rows(op.process_watermark(w)) == rows

    try:
        push(a, 0, 1, True, None)
        push(a, 2, 2, True, None)
        wm(a, 4, [("A", 3, 0, 5)])
        assert a.handle.stats()["live_state_entries"] == 1      # fired and retained
        blob = a.snapshot_state()
        a.close()
        b = _op(3, 5, key_type="STRING")
        b.initialize_state(blob)
        assert b.handle.stats()["current_watermark"] == 4 and b.handle.stats()["live_state_entries"] == 1
        push(b, 1, 10, True, ("A", 13, 0, 5))
        push(b, 5, 100, True, None)
        wm(b, 7, [("A", 113, 0, 8)])
        push(b, -10, 7, False, None)
        push(b, 9, 1, True, None)
        wm(b, 12, [("A", 1, 9, 12)])
        assert b.handle.stats()["live_state_entries"] == 1      # [0, 8) was cleaned silently
        push(b, 6, 5, True, ("A", 6, 6, 12))
        push(b, 1, 3, False, None)
        wm(b, 20, [])
        s = b.handle.stats()
        assert (s["live_state_entries"], s["num_late_records_dropped"], s["num_fired_windows"], s["error_flags"]) == (0, 2, 4, 0)
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- the main stream ------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("agg", [("sum", "LONG"), ("sum", "INT"), ("min", "DOUBLE"), ("count", "LONG")], ids=lambda a: "-".join(a))
def test_main_stream(agg, device):
    op, ref = _op(GAP, LATENESS, agg, late_side_output=True), LateSessionReference(GAP, LATENESS, agg)
    try:
        _drive(op, ref, main_stream(ftype=agg[1]), agg, device=device, side=True)
        assert ref.counts["fired_at_once"] >= 20 and ref.counts["dropped"] >= 20 and ref.counts["cleaned_silent"] >= 20
        _stats(op, ref)
        _same(_rows(op.process_watermark(LONG_MAX)), ref.process_watermark(LONG_MAX), agg)
        assert _stats(op, ref)["live_state_entries"] == 0
    finally:
        op.close()


def test_main_stream_in_one_superbucket():
    """HOST_HASHED with one hash for every key: all 40 keys in one list, tiles in arrival order"""
    op, ref = _op(GAP, LATENESS, key_type="HOST_HASHED", late_side_output=True), LateSessionReference(GAP, LATENESS)
    try:
        _drive(op, ref, main_stream(), side=True, hashed=True)
        _stats(op, ref)
    finally:
        op.close()


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_hot_key_over_three_tiles_pins_the_arrival_order(reverse):
    """several late rows of one batch land in one fired session: every row fires it again with the
    rows before it, so the rows depend on the arrival order (the reversed batch gives other rows:
    test_late_session_host.py)"""
    op, ref = _op(HOT_GAP, HOT_LATENESS, key_type="HOST_HASHED"), LateSessionReference(HOT_GAP, HOT_LATENESS)
    try:
        _drive(op, ref, hot_key_stream(reverse), hashed=True)
        assert ref.counts["fired_at_once"] >= 100 and ref.counts["dropped"] >= 20
        _stats(op, ref)
    finally:
        op.close()


def test_lateness_zero_is_the_plain_session_window():
    op, ref = _op(GAP, 0), SessionWindowReference(GAP)
    try:
        fired = 0
        for k, ts, v, wm in main_stream():
            ref.process(k.tolist(), ts.tolist(), v.tolist())
            _push(op, k, ts, v)
            assert _rows(op.collect()) == []
            want = ref.process_watermark(wm)
            fired += len(want)
            _same(_rows(op.process_watermark(wm)), want)
        s = op.handle.stats()
        assert (s["live_state_entries"], s["num_fired_windows"], s["num_late_records_dropped"], s["error_flags"]) == \
            (ref.live_sessions(), fired, ref.late_dropped, 0)
    finally:
        op.close()


# ---- capacity -------------------------------------------------------------------------------------
def _i64(x):
    return np.asarray(x, dtype=np.int64)


@pytest.mark.parametrize("extra", [0, 1], ids=["fills", "one_past"])
def test_retained_sessions_fill_the_list(extra):
    """cap_s = 64 (the smallest; one superbucket).  60 sessions fire and are retained; a tile of 4 +
    ``extra`` new sessions makes 64 -- fits -- or 65: the tile is dropped, the list as it was."""
    op, ref = _op(10, 10**6, key_type="HOST_HASHED", state_capacity=1, output_capacity=64), LateSessionReference(10, 10**6)
    try:
        assert op.handle.stats()["superbucket_capacity"] == 64
        k, ts = _i64(np.arange(60) % 7), _i64(1000 * np.arange(60))
        _drive(op, ref, [(k, ts, _i64(np.arange(60) + 1), 60000)], hashed=True)
        assert _stats(op, ref)["live_state_entries"] == 60 and ref.fired == 60
        held = op.snapshot_state()
        n = 4 + extra
        tile = (_i64(np.arange(n)), _i64(100000 + 1000 * np.arange(n)), _i64(np.ones(n)))
        _push(op, *tile, hashed=True)
        if not extra:
            assert _rows(op.collect()) == []
            ref.process(tile[0].tolist(), tile[1].tolist(), tile[2].tolist())
            assert _stats(op, ref)["live_state_entries"] == 64
            # a late row into a retained session still fires it: the full list takes merges
            _drive(op, ref, [(_i64([3]), _i64([3005]), _i64([7]), None)], hashed=True)
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
    op, ref = _op(10, 10**6, output_capacity=64), LateSessionReference(10, 10**6)
    try:
        k, ts = _i64(np.arange(60)), _i64(1000 * np.arange(60))
        ref.process(k.tolist(), ts.tolist(), [1] * 60)
        _push(op, k, ts, _i64(np.ones(60)))
        op.handle.advance(60000)                      # 60 rows wait in the result buffer
        want = ref.process_watermark(60000)
        late = (_i64(np.arange(n_late)), _i64(1000 * np.arange(n_late) + 3), _i64(np.full(n_late, 5)))
        _, at_once = ref.process(late[0].tolist(), late[1].tolist(), late[2].tolist())
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
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_LONG, 128, p, None, d.ctypes.data))
    return d


@pytest.mark.parametrize("dst", [1, 3])
def test_key_group_snapshot_with_fired_sessions_rescales(dst):
    pushes = main_stream()
    ref = LateSessionReference(GAP, LATENESS)
    old, news, other = _op(GAP, LATENESS), [], None
    try:
        _drive(old, ref, pushes[:3])
        wm = ref.watermark
        assert sum(1 for _, s, e, _ in ref.sessions() if e - 1 <= wm) >= 20      # fired and retained at the cut
        blobs = old.handle.snapshot_key_groups()[0]
        assert len(blobs) == 128 and all(struct.unpack_from("<q", b, 16)[0] == wm for b in blobs.values())
        live_blob = next(b for b in blobs.values() if len(b) > SW_HEADER)
        old.close()
        news = [_op(GAP, LATENESS, parallelism=dst, subtask_index=i) for i in range(dst)]
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
        for k, ts, v, w in pushes[3:]:
            d = _dest(k, dst)
            _, at_once = ref.process(k.tolist(), ts.tolist(), v.tolist())
            got = []
            for i, op in enumerate(news):
                _push(op, k[d == i], ts[d == i], v[d == i])
                got += _rows(op.collect())
            _same(got, at_once)
            _same([r for op in news for r in _rows(op.process_watermark(w))], ref.process_watermark(w))
        _same([r for op in news for r in _rows(op.process_watermark(LONG_MAX))], ref.process_watermark(LONG_MAX))
        st = [op.handle.stats() for op in news]
        assert sum(s["num_fired_windows"] for s in st) == ref.fired - fired0 and all(s["error_flags"] == 0 for s in st)
        assert sum(s["live_state_entries"] for s in st) == 0 and ref.counts["fired_at_once"] >= 20
        # blobs do not cross kinds or latenesses
        from flink_amd.datastream import SessionWindowOperator
        for other in (SessionWindowOperator(GAP, ("sum", "LONG"), max_batch_rows=4096, output_capacity=1 << 14).open(),
                      _op(GAP, LATENESS + 1)):
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


def test_whole_blob_of_another_kind_or_lateness_is_refused():
    from flink_amd.datastream import SessionWindowOperator
    plain = SessionWindowOperator(GAP, ("sum", "LONG"), max_batch_rows=4096, output_capacity=1 << 14).open()
    a, b = _op(GAP, LATENESS), _op(GAP, LATENESS + 1)
    try:
        for op in (plain, a):
            op.process_batch(_i64([1, 2]), _i64([0, 1000]), _i64([1, 1]))
        for src, dst in ((plain, a), (a, plain), (a, b)):
            with pytest.raises(_native.FlinkWinError, match="different operator configuration") as e:
                dst.initialize_state(src.snapshot_state())
            assert e.value.code == abi.FW_E_INVALID
    finally:
        for op in (plain, a, b):
            op.close()
