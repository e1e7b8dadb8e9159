"""The streams of the dynamic-gap late-session tests (test_dynamic_late_session_host.py,
test_gpu_dynamic_late_session_windows.py, test_gpu_dynamic_late_session_exchange.py): built once here
so that the CPU test which counts what the streams reach and the GPU tests which run them read the
same rows.

The main stream has the shape of late_session_streams.main_stream -- 40 keys, six pushes of 1023 /
1024 / 1025 / 3000 / 37 / 2048 rows, the same keys, timestamps, values and watermarks, lateness 300 --
and a gap per row from {5, 50, 400} with shares 0.45 / 0.45 / 0.10; the largest gap is 400.  Most
rows of gap 5 or 50 that are late candidates by their own gap would not be by the largest one, and
the long windows hold many shorter ones inside them.
"""
import numpy as np
from late_session_streams import LATENESS, N_KEYS, SEED, SIZES, T0, value_words  # noqa: F401
from late_session_streams import main_stream as _static_main_stream

GAPS, SHARES, MAX_GAP = (5, 50, 400), (0.45, 0.45, 0.10), 400


def main_stream(seed=SEED, ftype="LONG"):
    """[(keys, ts, values, gaps, watermark after the push)]; values LONG / INT as int64, DOUBLE as float64"""
    rng = np.random.default_rng([seed, 1])   # the gaps' own generator: the other columns are the static stream's
    out = []
    for k, ts, v, wm in _static_main_stream(seed, ftype):
        g = rng.choice(np.array(GAPS, dtype=np.int64), size=len(k), p=SHARES)
        out.append((k, ts, v, g.astype(np.int64), wm))
    return out


HOT_MAX_GAP, HOT_LATENESS = 400, 2000


def hot_key_stream(reverse=False):
    """One hot key over three tiles (3000 rows), mixed gaps: a first push builds sessions, a watermark
    fires them, the second push lands many late rows in fired sessions, so the cumulative rows pin the
    arrival order.  ``reverse``: the second push's rows in reversed order."""
    rng = np.random.default_rng(13)
    k1 = np.full(64, 5, np.int64)
    ts1 = (1000 + 200 * np.arange(64)).astype(np.int64)
    v1 = rng.integers(1, 1000, 64).astype(np.int64)
    g1 = rng.choice(np.array([5, 50, 120], dtype=np.int64), size=64).astype(np.int64)   # sessions [1000 + 200 i, + g)
    n = 3000
    k2 = np.where(rng.random(n) < 0.9, 5, rng.integers(0, 4, n)).astype(np.int64)
    ts2 = (1000 + rng.integers(-300, 64 * 200, n)).astype(np.int64)
    v2 = rng.integers(1, 1000, n).astype(np.int64)
    g2 = rng.choice(np.array([3, 20, 60, 400], dtype=np.int64), size=n, p=(0.4, 0.3, 0.25, 0.05)).astype(np.int64)
    if reverse:
        k2, ts2, v2, g2 = k2[::-1].copy(), ts2[::-1].copy(), v2[::-1].copy(), g2[::-1].copy()
    return [(k1, ts1, v1, g1, 1000 + 40 * 200), (k2, ts2, v2, g2, 1000 + 64 * 200 + 100)]
