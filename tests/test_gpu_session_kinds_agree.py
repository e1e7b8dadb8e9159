"""The four DataStream session kinds are two flags over one fold: a static handle, a dynamic handle
whose every gap equals the static gap, a lateness handle with lateness 0 and a dynamic-lateness handle
with lateness 0 fold one stream to exactly the same fired rows and late side records, and those are
session_window_reference.py's.  All aggregates are integer sums: no tolerance.  A SQL handle of eight
accumulator words (the NW = 8 kernels) folds a stream of the same shape against
sql_session_reference.py.

One superbucket (every key has one precomputed hash) whose list holds 2048 sessions.  The first push
puts 1100 keys with one row each into it, so the state exceeds one 1024-session coalesce chunk and the
carries between chunks run.  The second push has 1025 rows, one more than a tile: a hot key, rows that
bridge state sessions inside the tile and across the tile boundary, key runs with a late candidate in
both rule-3 orders in the first and in the second chunk of the list, and rows of the keys of the
second chunk.  Then watermarks fire part of the list, more of it, and all of it."""
import numpy as np
import pytest
from dynamic_late_session_reference import DynamicLateSessionReference
from dynamic_session_reference import DynamicSessionReference
from late_session_reference import LateSessionReference
from session_window_reference import SessionWindowReference
from sql_session_reference import SqlSessionReference

from flink_amd import abi

LONG_MAX = (1 << 63) - 1
GAP = 10
W1 = 504                       # the watermark in front of the second push
WATERMARKS = (1009, 1109, 1209, LONG_MAX)
# one superbucket list of 2048 sessions: 2048 superbuckets of 2 * 2^21 / 2048 sessions, one in use
STATE = {"max_parallelism": 1, "state_capacity": 1 << 21, "max_batch_rows": 1 << 12, "output_capacity": 1 << 13}
N_KEYS = 1100


def _key(i):
    return 10 * i + 5          # (the keys 10 * i are free for new keys between them)


def _ts0(i):
    return 1000 + 100 * (i % 4)


def stream():
    """[(keys, timestamps, values)] of the two pushes, int64 arrays in arrival order"""
    rng = np.random.default_rng(20)
    first = rng.permutation(N_KEYS)
    push1 = (np.array([_key(i) for i in first], np.int64), np.array([_ts0(i) for i in first], np.int64),
             np.array([i + 1 for i in first], np.int64))
    rows = []                  # (key, ts): shuffled below
    ordered = {}               # key -> its rows' timestamps in the arrival order the case needs
    rows += [(_key(5), _ts0(5) + 3 * j) for j in range(600)]            # a hot key: one session with the state's
    rows += [(_key(8), 1020), (_key(8), 1010)]                          # [1010, 1030) in the tile reaches the state's [1000, 1010)
    rows += [(_key(12), 1020)]                                          # ... and across the tile boundary: the last row below
    for i, late_first in ((300, True), (700, False), (1090, True), (1080, False)):
        # rule 3 under W1: 495 is late alone, 500 is not and reaches it; keys 1080 / 1090 sit in the second chunk
        ordered[_key(i)] = [495, 500] if late_first else [500, 495]
        rows += [(_key(i), ts) for ts in ordered[_key(i)]]
    ordered[_key(1080)].append(1005)                                    # a late-candidate run that also takes its state session
    rows += [(_key(1080), 1005)]
    rows += [(10 * 50, 400)]                                            # a new key with a late row alone: nothing stays
    rows += [(_key(i), _ts0(i) + 5) for i in range(1030, 1070)]         # rows into sessions of the second chunk
    rows += [(_key(N_KEYS + i), 1300) for i in range(30)]               # new keys behind the list
    rows += [(10 * i, 1200) for i in range(40)]                         # new keys in front: every session moves up
    filler = rng.integers(0, N_KEYS, 1024 - len(rows))                  # second sessions of keys all over the list
    rows += [(_key(int(i)), _ts0(int(i)) + 20) for i in filler]
    assert len(rows) == 1024
    rows = [rows[i] for i in rng.permutation(len(rows))]
    for key, want in ordered.items():                                   # the ordered runs: their slots, in the wanted order
        slots = [i for i, r in enumerate(rows) if r[0] == key and r[1] in want]
        for i, ts in zip(slots, want):
            rows[i] = (key, ts)
    rows.append((_key(12), 1010))                                       # row 1025, alone in the second tile: the bridge
    k, ts = (np.array(c, np.int64) for c in zip(*rows))
    return [push1, (k, ts, np.arange(1, len(k) + 1, dtype=np.int64) * 1000)]


def reference():
    """what every kind must produce: ([late row indices per push], [rows per watermark], late drops)"""
    ref = SessionWindowReference(GAP)
    pushes = stream()
    late = [ref.process(*(c.tolist() for c in pushes[0]))]
    assert ref.process_watermark(W1) == []
    late.append(ref.process(*(c.tolist() for c in pushes[1])))
    fired = [ref.process_watermark(w) for w in WATERMARKS]
    return late, fired, ref.late_dropped


def test_references_agree_on_the_stream():
    """the four references alone, before anything is asked of the GPU; and the stream has the shape"""
    late, fired, dropped = reference()
    pushes = stream()
    assert len(pushes[0][0]) == N_KEYS == len(set(pushes[0][0].tolist())) and len(pushes[1][0]) == 1025
    assert late[0] == [] and dropped == len(late[1]) == 3          # keys 300 and 1090 (late first) and the new key's row
    assert [len(f) > 0 for f in fired] == [True] * 4 and sum(len(f) for f in fired) > N_KEYS + 300
    gaps = [np.full(len(p[0]), GAP).tolist() for p in pushes]
    others = {"dynamic": DynamicSessionReference(), "late": LateSessionReference(GAP, 0),
              "dynamic_late": DynamicLateSessionReference(0, max_gap=GAP)}
    for name, ref in others.items():
        got_late = []
        for p, g in zip(pushes, gaps):
            cols = [c.tolist() for c in p] + ([g] if "dynamic" in name else [])
            out = ref.process(*cols)
            if "late" in name:                                     # (dropped, rows fired at once): none with lateness 0
                assert out[1] == []
                out = out[0]
            got_late.append(out)
            if p is pushes[0]:
                assert ref.process_watermark(W1) == []
        assert got_late == late, name
        assert [ref.process_watermark(w) for w in WATERMARKS] == fired, name
        assert ref.late_dropped == dropped and ref.live_sessions() == 0, name


def _open(kind):
    from flink_amd.datastream import (DynamicSessionWindowOperator, LateDynamicSessionWindowOperator,
                                      LateSessionWindowOperator, SessionWindowOperator)
    kw = dict(key_type="HOST_HASHED", late_side_output=True, **STATE)
    if kind == "static":
        return SessionWindowOperator(GAP, **kw).open()
    if kind == "dynamic":
        return DynamicSessionWindowOperator(GAP, **kw).open()
    if kind == "late":
        return LateSessionWindowOperator(GAP, 0, **kw).open()
    return LateDynamicSessionWindowOperator(GAP, 0, **kw).open()


def _rows(res):
    return sorted(zip(res["key"].tolist(), res["value"].tolist(), res["window_start"].tolist(), res["window_end"].tolist()),
                  key=lambda r: (r[3] - 1, r[0], r[2]))


def _fold(kind):
    """the stream through one handle: ([late (push_seq, row, key, ts, value)], [rows per watermark], counters)"""
    op = _open(kind)
    try:
        late, fired = [], []
        for seq, (k, ts, v) in enumerate(stream()):
            hashes = np.zeros(len(k), np.int32)                    # one hash: one superbucket
            if "dynamic" in kind:
                op.process_batch(k, ts, v, np.full(len(k), GAP, np.int64), hashes)
            else:
                op.process_batch(k, ts, v, hashes)
            if "late" in kind:
                assert len(op.collect()["key"]) == 0               # lateness 0: nothing is held to fire again
            lr = op.late_records()
            late.append(sorted(zip(lr["push_seq"].tolist(), lr["row"].tolist(), lr["key"].tolist(), lr["ts"].tolist(),
                                   lr["value"].tolist())))
            if seq == 0:
                assert op.handle.stats()["live_state_entries"] == N_KEYS
                assert len(op.process_watermark(W1)["key"]) == 0
        for w in WATERMARKS:
            fired.append(_rows(op.process_watermark(w)))
        s = op.handle.stats()
        assert s["error_flags"] == 0 and s["live_state_entries"] == 0
        return late, fired, (s["num_late_records_dropped"], s["num_fired_windows"])
    finally:
        op.close()


@pytest.fixture(scope="module")
def expected():
    late, fired, dropped = reference()
    pushes = stream()
    records = [sorted((seq, i, int(p[0][i]), int(p[1][i]), int(p[2][i])) for i in idx) for seq, (p, idx) in enumerate(zip(pushes, late))]
    return records, fired, (dropped, sum(len(f) for f in fired))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "dynamic", "late", "dynamic_late"])
def test_kind_folds_the_stream_like_the_reference(kind, expected):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert _fold(kind) == expected


# ---- the SQL form, eight accumulator words --------------------------------------------------------
# SUM, COUNT, MIN, MAX, AVG over NULL-able integer columns: integer words only, exact
SQL_AGGS = [("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT"), ("MIN", 1, "INT"), ("MAX", 1, "INT"), ("SUM", 2, "BIGINT"),
            ("COUNT", 2, "BIGINT"), ("COUNT_STAR", 0, "BIGINT"), ("AVG", 0, "BIGINT")]
SQL_TYPES = ["BIGINT", "INT", "BIGINT"]
SQL_NULLABLE = (0, 1, 2)


def _sql_operator():
    from flink_amd.table import SessionWindowAggOperator
    return SessionWindowAggOperator(GAP, SQL_AGGS, SQL_TYPES, key_type="HOST_HASHED", nullable_cols=SQL_NULLABLE, **STATE)


def test_sql_plan_has_eight_words():
    assert abi.host_sql_session_words(_sql_operator().cfg) == 8


def _sql_columns(n, seed):
    rng = np.random.default_rng(seed)
    vals = [rng.integers(-10**12, 10**12, n).astype(np.int64), rng.integers(-1000, 1000, n).astype(np.int64),
            rng.integers(-10**9, 10**9, n).astype(np.int64)]
    return vals, {c: rng.random(n) < 0.3 for c in SQL_NULLABLE}


@pytest.mark.gpu
def test_sql_eight_words_fold_the_stream_like_the_reference():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    op, ref = _sql_operator().open(), SqlSessionReference(GAP, SQL_AGGS)

    def order(rows):
        return sorted(rows, key=lambda r: (r[-1], r[0], r[-2]))
    try:
        for seq, (k, ts, _) in enumerate(stream()):
            vals, nulls = _sql_columns(len(k), 30 + seq)
            ref.process(k.tolist(), ts.tolist(), [[None if nulls[c][i] else int(vals[c][i]) for c in range(3)] for i in range(len(k))])
            op.process_batch(k, ts, vals, np.zeros(len(k), np.int32), nulls=nulls)
            if seq == 0:
                assert op.handle.stats()["live_state_entries"] == N_KEYS
                assert op.output_rows(op.process_watermark(W1)) == ref.process_watermark(W1) == []
        for w in WATERMARKS:
            got, want = order(op.output_rows(op.process_watermark(w))), order(ref.process_watermark(w))
            assert got == want and [type(x) for r in got for x in r] == [type(x) for r in want for x in r]
        s = op.handle.stats()
        assert s["error_flags"] == 0 and s["live_state_entries"] == 0
        assert s["num_late_records_dropped"] == ref.late_dropped == 3 and s["num_fired_windows"] == ref.fired
    finally:
        op.close()
