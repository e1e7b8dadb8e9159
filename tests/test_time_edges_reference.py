"""The time arithmetic at its edges, on the CPU: the oracle and the library's host functions against
the plain-Python reference of time_edge_cases.py (Python integers, direct window assignment).

test_gpu_time_edges.py compares the kernels with the oracle on the same origins, outlier sets,
intervals and watermark schedules; this module is what pins the oracle there (rows of every
watermark and the late-drop count), at 6 watermarks of about 2000 rows (3 pushes of 3 chunks of 221
rows + 5), and it compares fw_host_window_start, fw_host_next_trigger_watermark and fw_host_time_op --
the code the kernels run -- with the reference's own arithmetic, not with the oracle's."""
import ctypes as C

import numpy as np
import pytest

import time_edge_cases as E
from flink_amd import _native, abi
from parity_common import _cfg

LAYOUT = dict(chunk=221, n_wm=6, distinct=False)
POOL = np.arange(700, dtype=np.int64) * 7919 - 50000
CONFIGS = dict(list(E.configs().items())[:E.REFERENCE])
INTERVALS = E.interval_cases()


def _oracle_equals_reference(kw, stream, no_late_rows=False):
    cfg = _cfg(kw)
    rows, late, _ = E.oracle_run(cfg, stream)
    want, want_late = E.reference_run(kw, stream.steps)
    for si, (g, w) in enumerate(zip(rows, want)):
        assert g == w, f"watermark {si} ({stream.steps[si][3]}): {len(g)} rows vs reference {len(w)}"
    assert late == want_late
    return E.check_conditions(kw, stream, rows, late, no_late_rows)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("case", E.STREAM_CASES)
def test_oracle_equals_reference(case, config):
    kw = CONFIGS[config]
    _oracle_equals_reference(kw, E.case_stream(case, kw, POOL, **LAYOUT))


@pytest.mark.parametrize("name", sorted(INTERVALS))
def test_oracle_equals_reference_intervals(name):
    kw, shape = INTERVALS[name]
    _oracle_equals_reference(kw, E.interval_stream(name, shape, POOL, **LAYOUT), name in E.NO_LATE_ROWS)


@pytest.mark.parametrize("config", ["max5s", "sql_tumble_int_aggs", "ds_tumble_sum"])
def test_oracle_equals_reference_far_watermarks(config):
    _oracle_equals_reference(CONFIGS[config], E.far_watermark_stream(POOL, **LAYOUT))


# ---------------------------------------------------------------------------------------------------
# the host functions (the code the kernels run) against the reference's arithmetic
# ---------------------------------------------------------------------------------------------------
def _points():
    pts = {0, E.MIN_VALUE, E.MIN_VALUE + 1, E.MAX_VALUE}
    for p in (0, 30, 31, 61, 62):
        for d in ((1,) if p == 0 else (-1, 1)):
            v = ((1 << p) + d) if p else 1
            pts |= {v, -v}
    return sorted(pts)


POINTS = _points()
SIZES = [1, 2, 3, 1000, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 30 * E.DAY]


def test_points_are_the_listed_ones():
    assert len(POINTS) == 3 + 4 * 4 + 3 and (1 << 61) - 1 in POINTS and -(1 << 31) - 1 in POINTS and -1 in POINTS


@pytest.mark.parametrize("size", SIZES)
def test_host_window_start_equals_reference(size):
    L = _native.lib()
    for off in sorted({0, 1, -1, size - 1, -(size - 1)}):
        for ts in POINTS:
            want = E.window_start(ts, off, size)
            assert L.fw_host_window_start(ts, off, size) == want, (ts, off, size)
            x = ts - off
            if E.MIN_VALUE <= x <= E.MAX_VALUE and ts - size >= E.MIN_VALUE:  # nothing wraps: the floor grid point
                assert want == ts - (x % size) and want <= ts < want + size and (want - off) % size == 0


@pytest.mark.parametrize("size", SIZES)
def test_host_next_trigger_watermark_equals_reference(size):
    L = _native.lib()
    for wm in POINTS:
        want = E.next_trigger_watermark(wm, size)
        assert L.fw_host_next_trigger_watermark(wm, size) == want, (wm, size)
        if E.MIN_VALUE + size <= wm <= E.MAX_VALUE - 2 * size:  # nothing wraps: the next grid point - 1 above wm
            assert want > wm and want - wm <= size and (want + 1) % size == 0


TIME_OP_CONFIGS = {
    "hop": dict(window_kind=abi.WIN_HOP, size_ms=6000, slide_ms=2000, offset_ms=1000, count_star_index=0,
                aggs=[(abi.AGG_COUNT_STAR, 0, abi.T_I64)]),
    "cumulate": dict(window_kind=abi.WIN_CUMULATE, size_ms=12000, slide_ms=2000, aggs=[(abi.AGG_SUM, 0, abi.T_I64)]),
}


@pytest.mark.parametrize("name", sorted(TIME_OP_CONFIGS))
def test_host_time_op_equals_reference(name):
    """fw_host_time_op exposes the UTC conversions (0, 1: the identity), the next trigger watermark on
    the slice grid (2), the slice end of a rowtime (3) and the window start of a window end (4); the
    last window end of a slice has no operation code."""
    kw = TIME_OP_CONFIGS[name]
    cfg = _cfg(kw)
    out = C.c_int64()

    def op(what, x):
        _native.check(_native.lib().fw_host_time_op(C.byref(cfg), what, x, C.byref(out)))
        return out.value

    iv = E.slice_interval(kw)
    assert iv == 2000
    for x in POINTS:
        assert op(0, x) == x and op(1, x) == x
        assert op(2, x) == E.next_trigger_watermark(x, iv), x
        assert op(3, x) == E.slice_end(kw, x), x
        assert op(4, x) == E.window_start_of_end(kw, x), x
        se = E.slice_end(kw, x)  # ... and of a window end on the grid
        assert op(4, se) == E.window_start_of_end(kw, se), x
