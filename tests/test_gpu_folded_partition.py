"""The stable superbucket partition the count and session paths share (fw_folded.hip), through both
operators against their references: pushes on the edges of its 1024-row chunks, a device push that
takes several launches, and rows of another subtask in the middle of full chunks.

Everything is integer sums and compares exactly.  While an error bit is up every reader but stats and
snapshot refuses (test_gpu_folded_capacity_limits), so the rows a push with foreign keys fired cannot
be collected: that push is checked through the counters, and -- after the whole-handle restore that
clears the bit -- through the rows of the pushes and watermarks behind it, whose windows and sessions
hold its elements."""
import numpy as np
import pytest
import test_gpu_count_windows as cw
import test_gpu_session_windows as ds
from count_window_reference import CountWindowReference
from session_window_reference import SessionWindowReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

AGG = ("sum", "LONG")
KEYGROUP = abi.ERRF["KEYGROUP"]
LONG_MAX = (1 << 63) - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _session_rows(seed, n, t0, t1):
    """n rows over 300 keys spread as the count stream's, event times in [t0, t1)"""
    (k, v), = cw._stream(seed, 300, 1, n)
    return k, np.random.default_rng(seed + 1).integers(t0, t1, n).astype(np.int64), v


# ---- chunk edges, count path -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_count_chunk_edges(n):
    pushes = cw._stream(n, 300, 1, n)
    op = cw._op(6, 4, AGG)
    try:
        cw._check(cw._run(op, pushes), cw._reference(6, 4, AGG, pushes), AGG)   # rows and trigger ordinals
        st = op.handle.stats()
        assert st["error_flags"] == 0 and st["live_state_entries"] == len(set(pushes[0][0].tolist()))
    finally:
        op.close()


# ---- one device push of three launches (1024, 1024 and 1 rows) -----------------------------------------------
def test_count_device_push_larger_than_max_batch_rows():
    pushes = cw._stream(5, 300, 1, 2049)
    op = cw._op(6, 4, AGG, max_batch_rows=1024)
    try:
        got = cw._run(op, pushes, device=True)
        want = cw._reference(6, 4, AGG, pushes)      # push_seq 0: the ordinal is the row in the call
        assert max(o for *_, o in want) > 2000 and all(o >> 32 == 0 for *_, o in want)
        cw._check(got, want, AGG)
        assert op.handle.stats()["error_flags"] == 0
    finally:
        op.close()


def test_session_device_push_larger_than_max_batch_rows():
    """300 keys with rows on both sides of every launch boundary: at about 7 rows a key in [0, 2000)
    and a gap of 400 most neighbours merge, whichever launch they came in"""
    k, ts, v = _session_rows(7, 2049, 0, 2000)
    ref = SessionWindowReference(400, AGG)
    first, second = {}, {}                      # keys whose rows of the first two launches touch: many
    for i in range(2048):
        (first if i < 1024 else second).setdefault(int(k[i]), []).append(int(ts[i]))
    assert sum(any(abs(x - y) <= 400 for x in first[key] for y in second[key]) for key in first.keys() & second.keys()) >= 100
    op = ds._op(400, AGG, max_batch_rows=1024)
    try:
        fired = ds._drive(op, ref, [("push", k, ts, v), ("wm", LONG_MAX)], AGG, device=True)
        assert 300 <= fired < 2049
    finally:
        op.close()


# ---- foreign rows inside full chunks -----------------------------------------------------------------------
def _refused(call):
    with pytest.raises(_native.FlinkWinError) as e:
        call()
    assert e.value.code == abi.FW_E_CAPACITY


def test_count_foreign_rows_inside_full_chunks():
    (k, v), = cw._stream(41, 300, 1, 1025)
    own = cw._dest(k, 2) == 0
    assert 400 <= own.sum() <= 625 and own[:1024].any() and not own[:1024].all()
    ref = CountWindowReference(6, 4, AGG)
    first = ref.process(k[own].tolist(), v[own].tolist())
    op = cw._op(6, 4, AGG, parallelism=2, subtask_index=0)
    try:
        op.process_batch(k, v)                       # unfiltered
        st = op.handle.stats()
        assert st["error_flags"] == KEYGROUP
        assert st["live_state_entries"] == len(set(k[own].tolist()))
        assert st["num_fired_windows"] == len(first) > 0
        _refused(op.collect)
        op.initialize_state(op.snapshot_state())     # clears the bit and the uncollected rows; push_seq stays 1
        (k2, v2), = cw._stream(43, 300, 1, 1500)
        own2 = cw._dest(k2, 2) == 0
        k2, v2 = k2[own2], v2[own2]
        op.process_batch(k2, v2)
        want = [(a, b, ws, we, (1 << 32) | (at - int(own.sum()))) for a, b, ws, we, at in ref.process(k2.tolist(), v2.tolist())]
        assert any(ws < we - 1 for _, _, ws, we, _ in want)
        cw._check(cw._rows(op.collect()), want, AGG)     # windows that reach back into the first push
        st = op.handle.stats()
        assert st["error_flags"] == 0 and st["live_state_entries"] == len(set(k[own].tolist()) | set(k2.tolist()))
    finally:
        op.close()


def test_session_foreign_rows_inside_full_chunks():
    k, ts, v = _session_rows(47, 1025, 0, 20000)
    own = cw._dest(k, 2) == 0
    assert 400 <= own.sum() <= 625 and own[:1024].any() and not own[:1024].all()
    ref = SessionWindowReference(50, AGG)
    assert ref.process(k[own].tolist(), ts[own].tolist(), v[own].tolist()) == []
    op = ds._op(50, AGG, parallelism=2, subtask_index=0)
    try:
        op.process_batch(k, ts, v)                   # unfiltered
        st = op.handle.stats()
        assert st["error_flags"] == KEYGROUP
        assert st["live_state_entries"] == ref.live_sessions() > len(set(k[own].tolist()))
        _refused(op.handle.results)
        op.initialize_state(op.snapshot_state())     # clears the bit; the sessions stay
        want = ds._want(ref.process_watermark(10000))
        ds._same(ds._rows(op.process_watermark(10000)), want, AGG)
        assert len(want) > 100 and ref.live_sessions() > 100
        k2, ts2, v2 = _session_rows(53, 1500, 9000, 30000)
        own2 = cw._dest(k2, 2) == 0
        k2, ts2, v2 = k2[own2], ts2[own2], v2[own2]
        late = ref.process(k2.tolist(), ts2.tolist(), v2.tolist())
        op.process_batch(k2, ts2, v2)
        ds._same(ds._rows(op.process_watermark(LONG_MAX)), ds._want(ref.process_watermark(LONG_MAX)), AGG)
        st = op.handle.stats()
        assert st["error_flags"] == 0 and st["live_state_entries"] == 0
        assert st["num_late_records_dropped"] == len(late) > 0
    finally:
        op.close()
