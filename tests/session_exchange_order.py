"""The arrival order a session operator of parallelism p sees behind the packed keyBy exchange, in
pure numpy: the checker of tests/test_gpu_session_multirank.py, itself checked against
KeyByExchange on CPU tensors by tests/test_session_exchange_order.py.

One step moves every sender's batch.  The partition is a stable counting sort by destination: of a
sender's rows for destination d, the first ``cap`` (in input order) travel in its segment for d, the
rest in its spill.  Destination d then sees
    the segments sender by sender, each in the sender's input order,
    then the spills sender by sender,
    then the agreed watermark
(under the device valve the spill lands at the start of the next step, still under the held
watermark, and the agreed watermark follows it: the same sequence).  A session fold depends on the
order of one key's rows only, and a key has one destination, so ONE unsharded reference fed
    every sender's in-segment rows, sender by sender in input order,
    then every sender's spill rows, sender by sender,
    then the agreed watermark
sees every key's rows in the order its destination does.

Destinations come from the library's host routine (fw_host_assign_key_groups), the one
KeyByExchange.partition uses for host batches.
"""
import numpy as np

from flink_amd import _native


def destinations(keys, key_hash_kind, max_parallelism, parallelism):
    """The destination subtask of every key (int32)."""
    k = np.ascontiguousarray(keys, dtype=np.int64)
    dest = np.empty(len(k), dtype=np.int32)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), key_hash_kind, max_parallelism,
                                                          parallelism, None, dest.ctypes.data))
    return dest


def key_groups(keys, key_hash_kind, max_parallelism, parallelism):
    """The key group of every key (int32)."""
    k = np.ascontiguousarray(keys, dtype=np.int64)
    kg = np.empty(len(k), dtype=np.int32)
    dest = np.empty(len(k), dtype=np.int32)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), key_hash_kind, max_parallelism,
                                                          parallelism, kg.ctypes.data, dest.ctypes.data))
    return kg


def in_segment(dest, cap, parallelism):
    """True for the rows that travel in their destination's segment: the first ``cap`` of each
    destination in input order."""
    rank = np.empty(len(dest), dtype=np.int64)
    for d in range(parallelism):
        m = dest == d
        rank[m] = np.arange(int(m.sum()))
    return rank < cap


def destination_sequence(senders, cap, d, key_hash_kind, max_parallelism, parallelism):
    """The rows destination ``d`` receives in one step, in the order it sees them.  ``senders``: per
    sender a tuple of equally long columns, keys first.  Returns the columns."""
    seg, spill = [], []
    for cols in senders:
        dest = destinations(cols[0], key_hash_kind, max_parallelism, parallelism)
        ins = in_segment(dest, cap, parallelism)
        seg.append([c[(dest == d) & ins] for c in cols])
        spill.append([c[(dest == d) & ~ins] for c in cols])
    parts = seg + spill
    return [np.concatenate([p[i] for p in parts]) for i in range(len(senders[0]))]


def reference_order(senders, cap, key_hash_kind, max_parallelism, parallelism):
    """One step's rows of every sender in the order an unsharded reference is fed them (see above).
    Returns (columns, number of spill rows)."""
    seg, spill = [], []
    for cols in senders:
        dest = destinations(cols[0], key_hash_kind, max_parallelism, parallelism)
        ins = in_segment(dest, cap, parallelism)
        seg.append([c[ins] for c in cols])
        spill.append([c[~ins] for c in cols])
    parts = seg + spill
    return ([np.concatenate([p[i] for p in parts]) for i in range(len(senders[0]))],
            sum(len(p[0]) for p in spill))


# ---- the streams of tests/test_gpu_session_multirank.py and their expected results -----------------
# (here so that tests/test_session_exchange_order.py can check, without a GPU, that they exercise the
# order dependence: rows that are late when they arrive, some dropped and some kept)
T0 = 1_600_000_000_000
STEP = 1000
N_BATCHES = 6
N_ROWS = 4000          # per rank per batch
MAX_PARALLELISM = 128
GAP = 150
FINAL_WM = T0 + N_BATCHES * STEP + 120_000

SCENARIOS = {
    "ds_sum": dict(kind="ds", aggregation=("sum", "LONG")),
    "dynamic_gap": dict(kind="dyn", aggregation=("sum", "LONG")),
    "sql_sum_min": dict(kind="sql", aggs=[("SUM", 0, "BIGINT"), ("MIN", 0, "BIGINT")], value_types=["BIGINT"]),
}


def key_hash_kind(sc):
    from flink_amd import abi
    return abi.KEYHASH_BINROW_BIGINT if sc["kind"] == "sql" else abi.KEYHASH_LONG


def stream(sc, rank, batch, n=N_ROWS, own=None):
    """Rank ``rank``'s slice of batch ``batch``: (keys, ts, value columns ...), out-of-order
    timestamps reaching 2.5 steps back, so many rows are late for the valve's watermark when they
    arrive.  ``own`` = (parallelism, subtask): only the keys of that subtask's key groups."""
    rng = np.random.default_rng(104729 * batch + 31 * rank + 11)
    k = rng.integers(0, 500, n).astype(np.int64) * 7919 + 13
    t = (T0 + batch * STEP + rng.integers(-2500, STEP, n)).astype(np.int64)
    v = rng.integers(-10**6, 10**6, n).astype(np.int64)
    cols = [k, t, v]
    if sc["kind"] == "dyn":
        cols.append(rng.integers(1, GAP + 1, n).astype(np.int64))
    if own is not None:
        m = destinations(k, key_hash_kind(sc), MAX_PARALLELISM, own[0]) == own[1]
        cols = [c[m] for c in cols]
    return tuple(cols)


def proposed_wm(batch, rank):
    return T0 + batch * STEP - STEP + 300 * rank   # the valve's minimum is rank 0's


def segment_cap(batch, world, n=N_ROWS):
    """Even steps: the even share plus headroom (KeyByExchange.segment_capacity); odd steps: a quarter
    of the even share, so the overflow round runs."""
    return int(n / max(world, 1) * 1.25) + 1024 if batch % 2 == 0 else n // (4 * world)


def make_reference(sc):
    from dynamic_session_reference import DynamicSessionReference
    from session_window_reference import SessionWindowReference
    from sql_session_reference import SqlSessionReference
    if sc["kind"] == "ds":
        return SessionWindowReference(GAP, sc["aggregation"])
    if sc["kind"] == "dyn":
        return DynamicSessionReference(sc["aggregation"])
    return SqlSessionReference(GAP, sc["aggs"])


def feed(ref, sc, cols, seen):
    """The rows into the reference, in order; counts the rows that were late when they arrived by what
    became of them (seen["late_drop"], seen["late_kept"])."""
    k, t, v = cols[0].tolist(), cols[1].tolist(), cols[2].tolist()
    g = cols[3].tolist() if sc["kind"] == "dyn" else None
    for i in range(len(k)):
        gap = g[i] if g is not None else GAP
        late = t[i] + gap - 1 <= ref.watermark
        if sc["kind"] == "ds":
            kept = ref.add(k[i], t[i], v[i])
        elif sc["kind"] == "dyn":
            kept = ref.add(k[i], t[i], v[i], gap)
        else:
            kept = ref.add(k[i], t[i], [v[i]])
        assert kept or late
        if late:
            seen["late_kept" if kept else "late_drop"] += 1


def expected(name, world, own=None):
    """The fired rows of one unsharded reference over the ``world`` senders' streams in the order
    their destinations see them, its late drops, and what it saw.  Rows: (key, values ..., start, end)."""
    sc = SCENARIOS[name]
    ref = make_reference(sc)
    seen = {"late_drop": 0, "late_kept": 0, "spill_rows": 0}
    rows = []
    for b in range(N_BATCHES):
        senders = [stream(sc, r, b, own=own) for r in range(world)]
        cols, n_spill = reference_order(senders, segment_cap(b, world), key_hash_kind(sc), MAX_PARALLELISM, world)
        seen["spill_rows"] += n_spill
        feed(ref, sc, cols, seen)
        rows += ref.process_watermark(proposed_wm(b, 0))
    rows += ref.process_watermark(FINAL_WM)
    return [tuple(r) for r in rows], ref.late_dropped, seen
