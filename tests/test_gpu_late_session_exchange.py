"""Session windows with an allowed lateness behind the N > 1 keyBy exchange, one process: the pattern
of test_gpu_session_exchange.py (whose buffers, poison padding and key choice this module reuses) for
FW_WIN_SESSION_LATENESS.  Hand-built padded receive buffers -- 3 segments of 1500 rows over launches
of 2048 rows and tiles of 1024, so segments straddle both; empty, full, one-row and over-full
segments; spill-shaped pushes of 37 and 1024 rows -- go through fw_push_device_segments (SoA) and
fw_push_device_packed_segments into a handle of parallelism 2, whose watermark of record is on the
device (fw_advance_device).  A twin handle takes the compacted rows through fw_push_device and host
watermarks; both are compared with the reference (late_session_reference.py) after every push
(collect(): the rows fired at once, the late side output) and every watermark.  Everything is an
integer and compares exactly."""
import numpy as np
import pytest
from late_session_reference import LateSessionReference

import test_gpu_session_exchange as ex
from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

GAP, LATENESS = ex.GAP, 300
KD = ex.KINDS["ds"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _open(**kw):
    from flink_amd.datastream import LateSessionWindowOperator
    cfg = dict(ex.CFG)
    cfg.update(kw)
    return LateSessionWindowOperator(GAP, LATENESS, ("sum", "LONG"), late_side_output=True, **cfg).open()


def _rows(res):
    return [(int(k), int(v), int(s), int(e)) for k, v, s, e in zip(res["key"], res["value"], res["window_start"], res["window_end"])]


def _same(got, want):
    assert sorted(got) == sorted(tuple(w) for w in want)


@pytest.mark.parametrize("layout,device_wm", [("soa", False), ("packed", True), ("soa", True)],
                         ids=["soa-host_wm", "packed-device_wm", "soa-device_wm"])
def test_padded_push_equals_compacted_twin_and_reference(layout, device_wm):
    import torch
    own, foreign = ex._keys(KD)
    rng = np.random.default_rng(40 + (layout == "packed") + 2 * device_wm)
    op, twin, ref = _open(), _open(), LateSessionReference(GAP, LATENESS)
    try:
        for b, (n_segs, seg_len, counts) in enumerate(ex.PUSHES):
            live = ex._live_rows(KD, rng, own, b, sum(min(c, seg_len) for c in counts))
            cols, pos = ex._padded(KD, rng, foreign, n_segs, seg_len, counts, live)
            ex._push_padded(op, KD, layout, counts, cols)
            ex._push_compact(twin, KD, live)
            dropped, at_once = ref.process(live[0].tolist(), live[1].tolist(), live[2][0].tolist())
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
                s = ex._clean(o)
                assert (s["num_late_records_dropped"], s["current_watermark"], s["live_state_entries"], s["num_fired_windows"]) == \
                    (ref.late_dropped, wm, ref.live_sessions(), ref.fired)
        c = ref.counts
        assert min(c["dropped"], c["fired_at_once"], c["candidate_into_unfired"], c["cleaned_silent"]) >= 10, c
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
    a, b, ref = _open(), _open(), LateSessionReference(GAP, LATENESS)

    def wmt(w):
        return torch.tensor([w], dtype=torch.int64, device="cuda")
    try:
        k, ts = own[:8], 1000 + 60 * np.arange(8, dtype=np.int64)      # sessions [1000 + 60 i, + 50)
        ref.process(k.tolist(), ts.tolist(), [1] * 8)
        a.process_batch_device(ex._dev(k), ex._dev(ts), ex._dev(np.ones(8, np.int64)))
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
        _, at_once = ref.process([int(k[7])], [1425], [41])      # late, into the fired and retained [1420, 1470)
        assert at_once == [(int(k[7]), 42, 1420, 1475)]
        for o in (a, b):
            o.process_batch_device(ex._dev(k[7:]), ex._dev(np.array([1425], np.int64)), ex._dev(np.array([41], np.int64)))
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
        for call in (lambda: h.advance_device(cnt), lambda: h.push_device_segments(cnt, col[:1], col[:1], [col[:1]]),
                     lambda: h.push_device_packed_segments(cnt, col[:3], 3)):
            with pytest.raises(_native.FlinkWinError, match="not for session windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        assert h.stats()["error_flags"] == 0
    finally:
        op.close()
