"""The streams of the late-session tests (test_late_session_host.py, test_gpu_late_session_windows.py,
test_gpu_late_session_exchange.py): built once here so that the CPU test which counts what the
streams reach and the GPU tests which run them read the same rows.

The main stream: 40 keys, gap 50, lateness 300, six pushes of 1023 / 1024 / 1025 / 3000 / 37 / 2048
rows -- below, at and above one tile, three tiles, a short one, two tiles -- with
ts = 100000 + 400 b + U[-1200, 1000) in push b and the watermark 100000 + 400 b - 400 behind it.
About one row in six is a late candidate (ts + gap - 1 <= watermark); the drops, the immediate fires,
the candidates merged into unfired sessions, the on-time rows merged into fired sessions and the
silent cleanups are each reached at least 20 times (test_late_session_host.py counts them).
With only a few keys everything chains into one session and no class but the timer fire is reached.
"""
import numpy as np

GAP, LATENESS, N_KEYS, SEED = 50, 300, 40, 7
SIZES = (1023, 1024, 1025, 3000, 37, 2048)
T0 = 100000


def main_stream(seed=SEED, ftype="LONG"):
    """[(keys, ts, values, watermark after the push)]; values LONG / INT as int64, DOUBLE as float64"""
    rng = np.random.default_rng(seed)
    out = []
    for b, n in enumerate(SIZES):
        k = rng.integers(0, N_KEYS, n).astype(np.int64)
        ts = (T0 + 400 * b + rng.integers(-1200, 1000, n)).astype(np.int64)
        if ftype == "DOUBLE":
            v = np.round(rng.uniform(-100.0, 100.0, n), 3)
        elif ftype == "INT":
            v = rng.integers(-2**31, 2**31, n).astype(np.int64)   # sums wrap at 32 bits
        else:
            v = rng.integers(-10**9, 10**9, n).astype(np.int64)
        out.append((k, ts, v, T0 + 400 * b - 400))
    return out


def value_words(v):
    """the values as the reference takes them: DOUBLE as bit patterns"""
    v = np.asarray(v)
    return (v.view(np.int64) if v.dtype == np.float64 else v).tolist()


def hot_key_stream(reverse=False):
    """One hot key over three tiles (3000 rows): a first push builds sessions, a watermark fires
    them, the second push lands many late rows in fired sessions, so the cumulative rows pin the
    arrival order.  ``reverse``: the second push's rows in reversed order."""
    rng = np.random.default_rng(11)
    k1 = np.full(64, 5, np.int64)
    ts1 = (1000 + 200 * np.arange(64)).astype(np.int64)         # sessions [1000 + 200 i, +50)
    v1 = rng.integers(1, 1000, 64).astype(np.int64)
    n = 3000
    k2 = np.where(rng.random(n) < 0.9, 5, rng.integers(0, 4, n)).astype(np.int64)
    ts2 = (1000 + rng.integers(-300, 64 * 200, n)).astype(np.int64)
    v2 = rng.integers(1, 1000, n).astype(np.int64)
    if reverse:
        k2, ts2, v2 = k2[::-1].copy(), ts2[::-1].copy(), v2[::-1].copy()
    return [(k1, ts1, v1, 1000 + 40 * 200), (k2, ts2, v2, 1000 + 64 * 200 + 100)]


HOT_GAP, HOT_LATENESS = 50, 2000
