"""Dynamic-gap session windows with an allowed lateness behind the N > 1 keyBy exchange, one process:
the pattern of test_gpu_session_exchange.py (whose buffers, poison padding and key choice this module
reuses) for FW_WIN_SESSION_DYNAMIC_LATENESS.  Hand-built padded receive buffers -- 3 segments of 1500
rows over launches of 2048 rows and tiles of 1024, so segments straddle both; empty, full, one-row and
over-full segments; spill-shaped pushes of 37 and 1024 rows -- go through fw_push_device_segments
(SoA) and fw_push_device_packed_segments (rows of (key, ts, value, gap) words) into a handle of
parallelism 2, under host watermarks and with the watermark of record on the device
(fw_advance_device).  Every padding row is poison, its gap word (0) included.  A twin handle takes the
compacted rows through fw_push_device and host watermarks; both are compared with the reference
(dynamic_late_session_reference.py) after every push (collect(): the rows fired at once, the late
side output) and every watermark.  Everything is an integer and compares exactly."""
import numpy as np
import pytest
from dynamic_late_session_reference import DynamicLateSessionReference

import test_gpu_session_exchange as ex
from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

MAX_GAP, LATENESS = 400, 300
GAPS, SHARES = np.array([5, 50, 400], dtype=np.int64), (0.45, 0.45, 0.10)
KD = ex.KINDS["dyn"]      # the buffers' shape: two value columns, the padding's gap word 0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _open(**kw):
    from flink_amd.datastream import LateDynamicSessionWindowOperator
    cfg = dict(ex.CFG, state_capacity=1 << 12)      # short gaps merge less: more held sessions per key than the static twin
    cfg.update(kw)
    return LateDynamicSessionWindowOperator(MAX_GAP, LATENESS, ("sum", "LONG"), late_side_output=True, **cfg).open()


def _live_rows(rng, own, b, n):
    """ex._live_rows with a gap per row from GAPS"""
    k = rng.choice(own, n)
    ts = (ex.BASE + b * ex.WM_STEP + rng.integers(-1200, 1000, n)).astype(np.int64)
    vals = [rng.integers(-10**6, 10**6, n).astype(np.int64), rng.choice(GAPS, size=n, p=SHARES).astype(np.int64)]
    return k, ts, vals, {}


def _rows(res):
    return [(int(k), int(v), int(s), int(e)) for k, v, s, e in zip(res["key"], res["value"], res["window_start"], res["window_end"])]


def _same(got, want):
    assert sorted(got) == sorted(tuple(w) for w in want)


@pytest.mark.parametrize("layout", ["soa", "packed"])
@pytest.mark.parametrize("device_wm", [False, True], ids=["host_wm", "device_wm"])
def test_padded_push_equals_compacted_twin_and_reference(layout, device_wm):
    import torch
    own, foreign = ex._keys(KD)
    rng = np.random.default_rng(60 + (layout == "packed") + 2 * device_wm)
    op, twin, ref = _open(), _open(), DynamicLateSessionReference(LATENESS, max_gap=MAX_GAP)
    try:
        for b, (n_segs, seg_len, counts) in enumerate(ex.PUSHES):
            live = _live_rows(rng, own, b, sum(min(c, seg_len) for c in counts))
            cols, pos = ex._padded(KD, rng, foreign, n_segs, seg_len, counts, live)
            assert int((cols[2][1] == 0).sum()) == n_segs * seg_len - len(pos)       # every padding row's gap word is poison
            ex._push_padded(op, KD, layout, counts, cols)
            ex._push_compact(twin, KD, live)
            dropped, at_once = ref.process(live[0].tolist(), live[1].tolist(), live[2][0].tolist(), live[2][1].tolist())
            got = _rows(op.collect())
            _same(got, at_once)
            _same(got, _rows(twin.collect()))
            want_side = [(int(live[0][i]), int(live[1][i]), int(live[2][0][i])) for i in dropped]
            side, rows = ex._side(op)
            side_twin, rows_twin = ex._side(twin)
            assert side == side_twin == want_side
            assert rows == pos[dropped].tolist() and rows_twin == dropped
            wm = ex.BASE + b * ex.WM_STEP
            want = ref.process_watermark(wm)
            if device_wm:
                got = _rows(op.process_watermark_device(torch.tensor([wm], dtype=torch.int64, device="cuda")))
            else:
                got = _rows(op.process_watermark(wm))
            _same(got, want)
            _same(got, _rows(twin.process_watermark(wm)))
            for o in (op, twin):
                s = ex._clean(o)      # no FW_ERRF_KEYGROUP, no FW_ERRF_GAP: no padding row was read
                assert (s["num_late_records_dropped"], s["current_watermark"], s["live_state_entries"], s["num_fired_windows"]) == \
                    (ref.late_dropped, wm, ref.live_sessions(), ref.fired)
        c = ref.counts
        assert min(c["dropped"], c["fired_at_once"], c["candidate_into_unfired"], c["cleaned_silent"]) >= 10, c
        assert ref.own_gap_only >= 100 and ref.inside_held >= 100
        if device_wm:   # a lower device watermark changes nothing; a host watermark above it fires and cleans
            assert _rows(op.process_watermark_device(torch.tensor([wm - 300], dtype=torch.int64, device="cuda"))) == []
            _same(_rows(op.process_watermark(wm + 200)), ref.process_watermark(wm + 200))
            s = ex._clean(op)
            assert (s["current_watermark"], s["live_state_entries"]) == (wm + 200, ref.live_sessions())
        _same(_rows(op.process_watermark(ex.LONG_MAX)), ref.process_watermark(ex.LONG_MAX))
        assert ex._clean(op)["live_state_entries"] == 0
    finally:
        op.close()
        twin.close()


def test_key_group_restore_reads_the_device_watermark():
    """after a device advance the handle's watermark is Ctrl::cur: a key group snapshotted there is
    restored into a handle brought to that watermark from the device, and refused one below it"""
    import torch
    own, _ = ex._keys(KD)
    a, b, ref = _open(), _open(), DynamicLateSessionReference(LATENESS)

    def wmt(w):
        return torch.tensor([w], dtype=torch.int64, device="cuda")
    try:
        k, ts = own[:8], 1000 + 60 * np.arange(8, dtype=np.int64)
        g = np.array([50, 5, 50, 5, 50, 5, 50, 50], dtype=np.int64)      # sessions [1000 + 60 i, + g)
        ref.process(k.tolist(), ts.tolist(), [1] * 8, g.tolist())
        a.process_batch_device(ex._dev(k), ex._dev(ts), ex._dev(np.ones(8, np.int64)), ex._dev(g))
        _same(_rows(a.process_watermark_device(wmt(1480))), ref.process_watermark(1480))      # all fire, the oldest are cleaned
        live = ref.live_sessions()
        assert 0 < live < 8 and ref.fired == 8
        blobs = {kg: blob for kg, blob in a.handle.snapshot_key_groups()[0].items() if len(blob) > 48}
        assert blobs and a.handle.stats()["live_state_entries"] == live
        b.process_watermark_device(wmt(1400))
        with pytest.raises(_native.FlinkWinError, match="1480") as e:
            b.handle.restore_key_group_blob(next(iter(blobs.values())))
        assert e.value.code == abi.FW_E_STATE and "1400" in str(e.value)
        b.process_watermark_device(wmt(1480))
        b.handle.restore_key_groups(blobs, [])
        assert b.handle.stats()["live_state_entries"] == live
        _, at_once = ref.process([int(k[7])], [1425], [41], [3])      # late, inside the fired and retained [1420, 1470)
        assert at_once == [(int(k[7]), 42, 1420, 1470)]
        for o in (a, b):
            o.process_batch_device(ex._dev(k[7:]), ex._dev(np.array([1425], np.int64)), ex._dev(np.array([41], np.int64)),
                                   ex._dev(np.array([3], np.int64)))
            assert _rows(o.collect()) == at_once
            assert _rows(o.process_watermark_device(wmt(1490))) == []      # fired already: no timer row
    finally:
        a.close()
        b.close()


def test_parallelism_1_handle_refuses_the_exchange_calls():
    import torch
    op = _open(parallelism=1)
    try:
        h = op.handle
        cnt = torch.ones(1, dtype=torch.int64, device="cuda")
        col = torch.zeros(4, dtype=torch.int64, device="cuda")
        for call in (lambda: h.advance_device(cnt), lambda: h.push_device_segments(cnt, col[:1], col[:1], [col[:1]] * 2),
                     lambda: h.push_device_packed_segments(cnt, col[:4], 4)):
            with pytest.raises(_native.FlinkWinError, match="not for session windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        assert h.stats()["error_flags"] == 0
    finally:
        op.close()
