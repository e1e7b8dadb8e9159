"""The padded receive buffers of the count-window exchange tests, in plain numpy: the inputs of
tests/test_gpu_count_exchange.py, checked without a GPU by tests/test_count_exchange_inputs.py.

Geometry: a subtask 0 of parallelism 2 (maxParallelism 128) with max_batch_rows 2048 takes buffers of
3 segments of 1500 rows -- 4500 rows, three launches, the segments straddling the launches at rows
2048 and 4096 and the 1024-row partition chunks.  The count vectors hold a count above the segment
length (clamped to a full segment: the overflow went to the spill), an empty segment, a one-row
segment and partial ones.

Live rows: about 40 % are one hot key the subtask owns, the rest about 300 keys it owns.  Padding rows
are poison: random values under keys of the OTHER subtask's key groups, and -- behind the live rows of
every push's last segment with padding -- the hot key itself, so a fold that reads padding miscounts
the hot key, and one that routes padding raises FW_ERRF_KEYGROUP.
"""
import numpy as np

from flink_amd import _native, abi

MAX_P, PARALLELISM, SUBTASK = 128, 2, 0
MAX_BATCH_ROWS = 2048
TILE = 1024
SEG_LEN, N_SEGS = 1500, 3
COUNTS = [(1577, 0, 1237), (900, 1500, 1), (0, 1499, 1500), (1500, 2000, 640)]
N_KEYS = 300
HOT_SHARE = 0.4
WINDOWS = [(4, None), (5, 3), (250, 150)]
KEY_KINDS = {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT, "HOST_HASHED": abi.KEYHASH_PRECOMPUTED}
VALUE_KINDS = ("LONG", "INT", "DOUBLE", "DOUBLE_SPECIAL")
NAN_BITS = 0x7FF8000000000000


def key_hashes(keys):
    """The routing hash a HOST_HASHED stream carries beside its keys (any int32 function of the key)."""
    k = np.asarray(keys, dtype=np.int64).astype(np.uint64)
    return ((k * np.uint64(2654435761)) >> np.uint64(9)).astype(np.uint32).view(np.int32)


def destinations(keys, key_kind):
    k = np.ascontiguousarray(keys, dtype=np.int64)
    h = np.ascontiguousarray(key_hashes(k)) if key_kind == "HOST_HASHED" else None
    dest = np.empty(len(k), dtype=np.int32)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, h.ctypes.data if h is not None else None, len(k),
                                                          KEY_KINDS[key_kind], MAX_P, PARALLELISM, None, dest.ctypes.data))
    return dest


def keys_of(key_kind):
    """(the hot key, N_KEYS other owned keys, foreign keys); all fit an INT"""
    cand = np.arange(1, 2000, dtype=np.int64) * 7919 + 13
    dest = destinations(cand, key_kind)
    own, foreign = cand[dest == SUBTASK], cand[dest != SUBTASK]
    assert len(own) > N_KEYS and len(foreign) > 100
    return int(own[0]), own[1:N_KEYS + 1], foreign


def values(rng, n, value_kind):
    """n value words (int64): LONG; INT values whose sums wrap at 32 bits; DOUBLE bits for sums;
    DOUBLE bits with -0.0, 0.0 and NaN among negatives for min / max"""
    if value_kind == "LONG":
        return rng.integers(-10**12, 10**12, n).astype(np.int64)
    if value_kind == "INT":
        return rng.integers(-2**31, 2**31, n).astype(np.int64)
    if value_kind == "DOUBLE":
        return rng.uniform(0.5, 100.0, n).view(np.int64)
    assert value_kind == "DOUBLE_SPECIAL"
    v = -rng.uniform(0.5, 100.0, n)
    u = rng.random(n)
    v[u < 0.15] = -0.0
    v[u < 0.05] = 0.0
    v = v.view(np.int64).copy()
    v[u < 0.003] = NAN_BITS
    return v


def live_positions(counts, seg_len=SEG_LEN):
    return np.concatenate([s * seg_len + np.arange(min(c, seg_len)) for s, c in enumerate(counts)]).astype(np.int64)


def build_push(rng, key_kind, value_kind, counts, n_segs=N_SEGS, seg_len=SEG_LEN):
    """One padded buffer: dict(counts, keys, values, hashes (HOST_HASHED, else None) -- the buffer's
    columns --, live_keys, live_values, live_hashes -- the compacted live rows in arrival order --,
    pos -- each live row's buffer position)."""
    hot, own, foreign = keys_of(key_kind)
    n = n_segs * seg_len
    pos = live_positions(counts, seg_len)
    n_live = len(pos)
    lk = rng.choice(own, n_live)
    lk[rng.random(n_live) < HOT_SHARE] = hot
    lv = values(rng, n_live, value_kind)
    pk = rng.choice(foreign, n)
    pv = values(rng, n, value_kind)
    padded = [s for s, c in enumerate(counts) if c < seg_len]
    if padded:  # the hot key in the padding of the last segment that has any
        s = padded[-1]
        pk[s * seg_len + counts[s]:(s + 1) * seg_len] = hot
    pk[pos], pv[pos] = lk, lv
    hashed = key_kind == "HOST_HASHED"
    return dict(counts=tuple(counts), keys=pk, values=pv, hashes=key_hashes(pk) if hashed else None, live_keys=lk,
                live_values=lv, live_hashes=key_hashes(lk) if hashed else None, pos=pos)


def build_case(key_kind, value_kind, seed=1):
    """The case's pushes (COUNTS) and one more compact batch (keys, values, hashes) for the state check."""
    rng = np.random.default_rng(seed)
    pushes = [build_push(rng, key_kind, value_kind, c) for c in COUNTS]
    hot, own, _ = keys_of(key_kind)
    k = rng.choice(own, 1500)
    k[rng.random(1500) < HOT_SHARE] = hot
    extra = (k, values(rng, 1500, value_kind), key_hashes(k) if key_kind == "HOST_HASHED" else None)
    return pushes, extra


def expected_ord(pushes, arrival, first_push_seq=0):
    """push_seq << 32 | buffer position of the live row with the given arrival index over ``pushes``"""
    base = 0
    for b, p in enumerate(pushes):
        if arrival < base + len(p["pos"]):
            return ((first_push_seq + b) << 32) | int(p["pos"][arrival - base])
        base += len(p["pos"])
    raise IndexError(arrival)
