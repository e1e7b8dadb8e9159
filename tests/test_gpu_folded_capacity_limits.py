"""The session and count paths (fw_session.hip, fw_count.hip) at their capacity limits, against the
plain references under the contract the kernels' comments give (folded_capacity_cases.CappedReference):
a tile whose sessions do not fit is dropped whole, a key that finds no table slot is dropped whole,
rows past a full output or side buffer are lost -- and everything else stays exact.

All keys of a HOST_HASHED operator that is handed one hash share a superbucket, and the partition is
stable, so tile j of a push is its rows [1024 j, 1024 (j + 1)): the inputs (folded_capacity_cases.py,
checked on the CPU by test_folded_capacity_inputs.py) sit exactly on each edge.  Every comparison goes
through the path's own `_same` / `_check` (integers and NULL masks exactly, the one DOUBLE SUM / AVG
layout at 1e-9 relative) and leaves out no row.  While an error bit is up every reader but stats and
snapshot refuses with FW_E_CAPACITY (read_ctrl, fw_api.hip:1036); only a whole-handle restore clears
the bits (fd_restored_ctrl, fw_folded.hip:211-215; n_side in fw_session.hip:1046).  DESIGN section 9 states the contract."""
import numpy as np
import pytest
import test_gpu_count_windows as cw
import test_gpu_dynamic_session_windows as dyn
import test_gpu_session_windows as ds
import test_gpu_sql_session_windows as sql
from folded_capacity_cases import (AGG, CAP_E, COUNT_PAIRS, G, KINDS, LAYOUTS, LONG_MAX, OUT_CAP, CappedReference, case1, case2,
                                   case3, case4, case5, case6, case7, case8, case9, case10, count_reference_rows, layout_of)

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

STATE, OUTPUT, LATE = abi.ERRF["STATE"], abi.ERRF["OUTPUT"], abi.ERRF["LATE"]
SW_HEADER, CW_HEADER = 48, 80      # bytes in front of a session blob's / a count blob's entries


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_layouts_are_the_sql_modules():
    assert all(LAYOUTS[nw] == sql.LAYOUTS[nw] for nw in (2, 4, 8))


# ---- sessions: one operator per kind ---------------------------------------------------------------------
def _open(kind, **kw):
    kw.setdefault("max_batch_rows", 4096)
    kw.setdefault("output_capacity", 1 << 14)
    if kind == "static":
        from flink_amd.datastream import SessionWindowOperator
        return SessionWindowOperator(G, AGG, **kw).open()
    if kind == "dynamic":
        from flink_amd.datastream import DynamicSessionWindowOperator
        return DynamicSessionWindowOperator(G, AGG, **kw).open()
    from flink_amd.table import SessionWindowAggOperator
    aggs, types, nullable = layout_of(kind)
    return SessionWindowAggOperator(G, aggs, types, nullable_cols=nullable, **kw).open()


def _words(kind):
    return int(kind[3:]) if kind.startswith("sql") else 1


def _feed(op, p, shared=True):
    h = np.zeros(len(p), np.int32) if shared else None      # one hash for every key: one superbucket
    if p.kind == "static":
        op.process_batch(p.k, p.ts, p.v, h)
    elif p.kind == "dynamic":
        op.process_batch(p.k, p.ts, p.v, p.g, h)
    else:
        op.process_batch(p.k, p.ts, p.vals, h, nulls=p.nulls)


def _push(op, ref, p, shared=True):
    late = ref.push(p)
    _feed(op, p, shared)
    return late


def _wm(op, ref, w, kind):
    """one watermark: every fired row against the reference's, through the kind's own comparison"""
    res, want = op.process_watermark(w), ref.wm(w)
    if kind == "static":
        ds._same(ds._rows(res), ds._want(want), AGG)
    elif kind == "dynamic":
        dyn._same(dyn._rows(res), dyn._want(want), AGG)
    else:
        sql._same(op.output_rows(res), want)
    return len(want)


def _stats(op, ref, flags):
    s = op.handle.stats()
    assert (s["live_state_entries"], s["num_late_records_dropped"], s["num_fired_windows"], s["error_flags"]) == \
        (ref.live(), ref.late_dropped, ref.fired, flags)
    return s


def _refused(call):
    with pytest.raises(_native.FlinkWinError) as e:
        call()
    assert e.value.code == abi.FW_E_CAPACITY


def _seeded(kind, c, **kw):
    """the operator and the capped reference behind the case's first push"""
    op, ref = _open(kind, key_type="HOST_HASHED", state_capacity=1, **kw), CappedReference(kind, c["cap_s"])
    try:
        assert op.handle.stats()["superbucket_capacity"] == c["cap_s"]
        assert _push(op, ref, c["seed"]) == []
        assert _stats(op, ref, 0)["live_state_entries"] == c["held"]
    except BaseException:
        op.close()
        raise
    return op, ref


def _tight_tile(kind, c, **kw):
    op, ref = _seeded(kind, c, **kw)
    try:
        held, snap = op.snapshot_state(), ref.snapshot()
        assert len(held) == SW_HEADER + c["held"] * (3 + _words(kind) + 1) * 8
        assert _push(op, ref, c["tile"]) == [] and ref.state_bit == c["drops"]
        if c["drops"]:
            assert _stats(op, ref, STATE)["live_state_entries"] == c["held"]
            assert op.snapshot_state()[SW_HEADER:] == held[SW_HEADER:]      # the list is as it was, bit for bit
            _refused(lambda: op.process_watermark(1))                       # (a watermark that fires nothing)
            op.initialize_state(held)
            ref.restore(snap)
        assert _stats(op, ref, 0)["live_state_entries"] == (c["held"] if c["drops"] else c["final"])
        assert _wm(op, ref, LONG_MAX, kind) == (c["held"] if c["drops"] else c["final"])
        _stats(op, ref, 0)
    finally:
        op.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("final", [63, 64, 65])
def test_tight_tile_at_the_small_lists_capacity(kind, final):
    """Case 1.  cap_s = 64, 40 held sessions, one tile after which the list holds 63, 64 or 65:
    `ns + may_add > cap_s` (fw_session.hip:249-250), so the coalesce runs twice (:381), pass 0 counting
    and pass 1 writing with the carries reset between them (:382-390) and sa / sk / sts / se used again.
    63 and 64 fit -- `c_groups == cap_s` is not `> cap_s` (:493) -- and fire what the reference fires;
    65 raises STATE alone and leaves the list's bytes as they were (:496-499).  Every fold instance:
    k_sw_fold<1>, <1, true>, <2>, <4>, <8>."""
    _tight_tile(kind, case1(kind, final))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [24, 25])
def test_tight_tile_over_two_chunks_with_a_group_across_the_boundary(kind, n_new):
    """Case 2.  cap_s = 1024, 1000 held sessions and a full tile: L = 2024 spans two 1024-entry chunks of
    M in both passes (fw_session.hip:392).  Key 500's tile session starts at entry 1000, its dead slots
    cross entry 1023 / 1024 and its held session at entry 1040 joins through the carries c_key / c_max
    (:423-426) and c_acc / c_end, the `hcount == 0` branch (:461-465).  24 new sessions fill the list
    exactly (1024), 25 are one too many (:493)."""
    _tight_tile(kind, case2(kind, n_new), max_parallelism=1)


@pytest.mark.parametrize("kind", KINDS)
def test_tile_dropped_in_the_middle_of_a_push(kind):
    """Case 3.  Three tiles in one push: tile 0 fits (50 sessions), tile 1 does not (80) and is dropped,
    and the loop goes on (`continue`, fw_session.hip:496-499) to tile 2, which joins held sessions, tile
    0's among them.  STATE alone; the next collection raises FW_E_CAPACITY; a restore of the snapshot of
    before the push clears the bit (fw_folded.hip:213), and the push without tile 1's rows then leaves the very
    bytes the three-tile push left, and fires what the plain reference fires."""
    c = case3(kind)
    op, ref = _seeded(kind, c)
    try:
        held, snap = op.snapshot_state(), ref.snapshot()
        assert _push(op, ref, c["push"]) == [] and [(t[0], t[1]) for t in ref.tiles[-3:]] == c["tiles"]
        assert _stats(op, ref, STATE)["live_state_entries"] == 50
        after = op.snapshot_state()
        _refused(lambda: op.process_watermark(1))
        op.initialize_state(held)
        ref.restore(snap)
        assert _stats(op, ref, 0)["live_state_entries"] == 40
        assert _push(op, ref, c["without_tile_1"]) == [] and not ref.state_bit
        _stats(op, ref, 0)
        assert op.snapshot_state()[SW_HEADER:] == after[SW_HEADER:]
        assert _wm(op, ref, LONG_MAX, kind) == 50
        _stats(op, ref, 0)
    finally:
        op.close()


def _late_rows(lr):
    return sorted(zip(lr["push_seq"].tolist(), lr["row"].tolist(), lr["ts"].tolist(), lr["value"].tolist()))


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("over", [False, True])
def test_late_rows_of_a_tile_at_the_list_capacity(kind, over):
    """Case 4.  A tile with late candidates (the serial path, fw_session.hip:330-372) -- 20 anchored and
    kept, 15 unreachable and dropped -- that ends at 64 sessions, or at 65 and is dropped.  The kernel
    counts the 15 and writes their side rows (:346-360) before it decides (:493), so they are counted
    either way.  At 64 late_records() delivers exactly them.  At 65 STATE is up, late_records() refuses
    (sw_late_records reads through read_ctrl, fw_api.hip:2176), and the restore that clears the bit also
    clears n_side (:1046): the 15 stay counted in num_late_records_dropped, which a restore into the
    same handle does not reset, and are never delivered."""
    c = case4(kind, over)
    op, ref = _seeded(kind, c, late_side_output=True)
    try:
        assert _wm(op, ref, c["watermark"], kind) == 0
        held, snap = op.snapshot_state(), ref.snapshot()
        late = _push(op, ref, c["tile"])
        assert late == c["late"] and ref.late_dropped == 15 and ref.state_bit == over
        if over:
            assert _stats(op, ref, STATE)["live_state_entries"] == 40
            assert op.snapshot_state()[SW_HEADER:] == held[SW_HEADER:]
            _refused(op.late_records)
            op.initialize_state(held)
            ref.restore(snap)
            _stats(op, ref, 0)                                              # num_late_records_dropped is still 15
            assert _late_rows(op.late_records()) == []
        else:
            _stats(op, ref, 0)
            t = c["tile"]
            assert _late_rows(op.late_records()) == [(1, i, int(t.ts[i]), int(t.v[i])) for i in late]
        assert _wm(op, ref, LONG_MAX, kind) == (40 if over else 64)
        _stats(op, ref, 0)
    finally:
        op.close()


def test_lists_longer_than_one_tile():
    """Case 5.  cap_s = 2048 (state_capacity 2^21: 2048 superbuckets of 2048 sessions, a few hundred MB
    of state and scratch).  1500 sessions in one superbucket: a joining tile whose L = 2524 spans three
    chunks of M with pass 0 run (fw_session.hip:381, :392); a watermark that fires an interleaved 700,
    so k_sw_advance's chunk loop (:567) runs twice and its stable compaction (:608) moves 256 kept
    sessions of chunk 1 into chunk 0's slots; a full tile on the 800 left (L = 1824); the final
    watermark.  No capacity is exceeded: this is the list-size edge."""
    c = case5()
    op = _open("static", key_type="HOST_HASHED", state_capacity=1 << 21, max_batch_rows=2048)
    ref = CappedReference("static", c["cap_s"])
    try:
        s = op.handle.stats()
        assert (s["num_superbuckets"], s["superbucket_capacity"]) == (2048, 2048)
        fires = []
        for st, live in zip(c["steps"], c["live"]):
            if st[0] == "push":
                assert _push(op, ref, st[1]) == []
            else:
                fires.append(_wm(op, ref, st[1], "static"))
            assert _stats(op, ref, 0)["live_state_entries"] == live
        assert fires == c["fires"]
    finally:
        op.close()


@pytest.mark.parametrize("kind", ["static", "sql4"])
@pytest.mark.parametrize("how", ["snapshot", "key_groups"])
def test_session_output_capacity(kind, how):
    """Case 6.  output_capacity = 64, sessions over many superbuckets, so many workgroups claim rows
    (fw_session.hip:557).  A watermark that fires exactly 64 is clean (`out_base + n_due > out_cap`,
    :560, is false at 64).  One that fires 65 raises OUTPUT alone; fw_get_stats clamps results_available
    to 64 (fw_api.hip:2278), the collection refuses (cw_results, fw_api.hip:1832-1837), and the 65
    sessions are gone from the state (:559, :587): only a restore brings them back -- the whole-handle
    snapshot into the same handle, which clears `error` and `out_count[0]` (fw_folded.hip:213-214), or key-group
    snapshots into a fresh one (sw_restore(key_group) needs an empty key group and clears nothing,
    fw_folded.hip:209-210).  Either way the 65 then come out exactly, read over two watermarks."""
    c = case6(kind)
    op, ref, fresh = _open(kind, output_capacity=OUT_CAP), CappedReference(kind), None
    try:
        for p in c["pushes"]:
            assert _push(op, ref, p, shared=False) == []
        assert _wm(op, ref, c["first"], kind) == OUT_CAP
        assert _stats(op, ref, 0)["live_state_entries"] == 65
        snap = ref.snapshot()
        if how == "snapshot":
            blob = op.snapshot_state()
        else:
            blobs, wm = op.handle.snapshot_key_groups()
        _refused(lambda: op.process_watermark(c["over"]))
        ref.fired += 65
        s = op.handle.stats()
        assert (s["error_flags"], s["results_available"], s["live_state_entries"], s["num_fired_windows"]) == (OUTPUT, OUT_CAP, 0, ref.fired)
        _refused(lambda: op.handle.results(reset=True))
        if how == "snapshot":
            op.initialize_state(blob)
            target = op
        else:
            target = fresh = _open(kind, output_capacity=OUT_CAP)
            fresh.handle.restore_key_groups(blobs, [wm])
            fresh.handle.initialize_watermark(wm)      # (the DataStream operator's watermark comes from the stream)
            ref.fired = 0
        ref.restore(snap)
        s = _stats(target, ref, 0)
        assert (s["results_available"], s["live_state_entries"], s["current_watermark"]) == (0, 65, c["first"])
        assert [_wm(target, ref, w, kind) for w in c["split"]] == c["fires"][2:]
        assert _stats(target, ref, 0)["live_state_entries"] == 0
    finally:
        op.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("n", [2048, 2049])
def test_late_side_capacity(n):
    """Case 7.  max_batch_rows = 1024, so the side output holds 2048 rows (fw_session.hip:791).  2048 late
    rows uncollected are clean (`o < side_cap`, :351) and all come out with their (push_seq, row, ts,
    value).  The 2049th raises LATE alone (:358); n_side goes on counting and the host clamps it
    (fw_api.hip:2178) -- but late_records() refuses while the bit is up, and the restore that clears it
    clears n_side too (:1046).  num_late_records_dropped is 2049 before and after; the handle then works
    again, with the snapshot's push_seq."""
    c = case7(n)
    op, ref = _open("static", late_side_output=True, max_batch_rows=1024), CappedReference("static")
    try:
        assert _wm(op, ref, c["watermark"], "static") == 0
        held, snap = op.snapshot_state(), ref.snapshot()
        want = []
        for seq, p in enumerate(c["pushes"]):
            want += [(seq, i, int(p.ts[i]), int(p.v[i])) for i in _push(op, ref, p, shared=False)]
        assert len(want) == n == ref.late_dropped
        if n == 2048:
            _stats(op, ref, 0)
            assert _late_rows(op.late_records()) == sorted(want)
            seq = len(c["pushes"])
        else:
            _stats(op, ref, LATE)
            _refused(op.late_records)
            op.initialize_state(held)
            ref.restore(snap)
            _stats(op, ref, 0)
            assert _late_rows(op.late_records()) == []
            seq = 0                                        # no push lies before the snapshot
        p = c["after"]
        assert _push(op, ref, p, shared=False) == [0, 1, 2]
        assert _late_rows(op.late_records()) == [(seq, i, int(p.ts[i]), int(p.v[i])) for i in range(3)]
        assert _stats(op, ref, 0)["num_late_records_dropped"] == n + 3
    finally:
        op.close()


# ---- the count table -------------------------------------------------------------------------------------
COUNT_AGGS = [("sum", "LONG"), ("max", "LONG")]


def _cop(size, slide, agg, **kw):
    from flink_amd.datastream import CountWindowOperator
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return CountWindowOperator(size, slide, agg, **kw).open()


def _cfeed(op, push, shared=True):
    k, v = push
    op.process_batch(k, v, np.zeros(len(k), np.int32) if shared else None)


def _cstats(op, live, fired, flags):
    s = op.handle.stats()
    assert (s["live_state_entries"], s["num_fired_windows"], s["error_flags"]) == (live, fired, flags)
    return s


def _entries(blob, size, slide):
    """a count blob's entries (key, count, key group << 32 | sub-bucket, ring[R]) sorted by key"""
    r = size // np.gcd(size, slide)
    e = np.frombuffer(blob[CW_HEADER:], np.int64).reshape(-1, 3 + r)
    return e[np.argsort(e[:, 0])]


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
@pytest.mark.parametrize("agg", COUNT_AGGS, ids=lambda a: a[0])
def test_count_table_full_then_two_more_keys(size, slide, agg):
    """Case 8.  cap_e = 64 and 64 keys in one superbucket: every slot is usable -- the probe runs over
    all cap_e slots (fw_count.hip:92, :108) -- and nothing is raised.  A push with two more keys raises
    STATE alone (:121); the two keys get nothing, the table still holds 64, and the 64 keys' windows of
    that push are fired and counted -- but not delivered: collect() refuses while the bit is up
    (cw_results, fw_api.hip:1832).  The route is restore and replay: the snapshot of before the push,
    and the push without the two keys' rows, deliver the reference's rows of the 64 keys in its order.
    The table the overflowing push left (a snapshot is not refused) holds the very entries the replay
    leaves, and restored it goes on exactly."""
    c = case8(size, slide)
    held = set(c["held"].tolist())
    want = count_reference_rows(size, slide, agg, c["pushes"])
    op = _cop(size, slide, agg, key_type="HOST_HASHED", state_capacity=1)
    try:
        assert op.handle.stats()["superbucket_capacity"] == CAP_E
        fired = 0
        for i in (0, 1):
            _cfeed(op, c["pushes"][i])
            cw._check(cw._rows(op.collect()), want[i], agg)
            fired += len(want[i])
            _cstats(op, CAP_E, fired, 0)
        before = op.snapshot_state()
        _cfeed(op, c["pushes"][2])
        mine = [r for r in want[2] if r[0] in held]
        assert len(mine) < len(want[2])                       # (the two keys' slide + 2 rows would have fired)
        s = _cstats(op, CAP_E, fired + len(mine), STATE)
        assert s["results_available"] == len(mine)
        _refused(op.collect)
        after = op.snapshot_state()
        op.initialize_state(before)
        assert _cstats(op, CAP_E, fired + len(mine), 0)["results_available"] == 0
        k3, v3 = c["pushes"][2]
        sel = np.isin(k3, c["held"])
        replay = c["pushes"][:2] + [(k3[sel], v3[sel])]
        _cfeed(op, replay[2])
        got = cw._rows(op.collect())
        cw._check(got, count_reference_rows(size, slide, agg, replay)[2], agg)
        assert [r[:4] for r in got] == [r[:4] for r in mine]
        _cstats(op, CAP_E, fired + 2 * len(mine), 0)
        assert np.array_equal(_entries(op.snapshot_state(), size, slide), _entries(after, size, slide))
        op.initialize_state(after)                           # the table behind the overflow, the bit cleared
        _cfeed(op, c["pushes"][3])
        cw._check(cw._rows(op.collect()), want[3], agg)
        _cstats(op, CAP_E, fired + 2 * len(mine) + len(want[3]), 0)
    finally:
        op.close()


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
@pytest.mark.parametrize("agg", COUNT_AGGS, ids=lambda a: a[0])
def test_count_table_all_or_nothing_per_key_under_a_race(size, slide, agg):
    """Case 9.  One tile with 54 held keys and 40 new ones for 10 free slots: which 10 win the atomicCAS
    (fw_count.hip:109) is not determined.  The invariant: the table then holds the 54 and a set S of
    exactly 10 new keys, each with all of its rows (its count is its rows so far) -- a key is kept
    whole or dropped whole (:121, `live` at :132) -- the windows fired are the reference's for the 54 and
    S, and the table restored (which clears STATE) goes on exactly for the 54 and S: the rows of the next
    push equal the reference's, whose windows reach back into the race tile."""
    c = case9(size, slide)
    held, new = set(c["held"].tolist()), set(c["new"].tolist())
    p1, race, p3 = c["pushes"]
    op = _cop(size, slide, agg, key_type="HOST_HASHED", state_capacity=1)
    try:
        assert op.handle.stats()["superbucket_capacity"] == CAP_E
        _cfeed(op, p1)
        all_rows = count_reference_rows(size, slide, agg, [p1, race])
        cw._check(cw._rows(op.collect()), all_rows[0], agg)
        _cfeed(op, race)
        blob = op.snapshot_state()
        ent = _entries(blob, size, slide)
        keys = set(ent[:, 0].tolist())
        S = keys - held
        assert len(ent) == CAP_E and keys >= held and S <= new and len(S) == c["room"]
        so_far = np.concatenate([p1[0], race[0]])
        assert ent[:, 1].tolist() == [int((so_far == k).sum()) for k in ent[:, 0]]
        fired = len(all_rows[0]) + sum(r[0] in keys for r in all_rows[1])
        _cstats(op, CAP_E, fired, STATE)
        _refused(op.collect)
        op.initialize_state(blob)
        sel = np.isin(p3[0], ent[:, 0])
        nxt = (p3[0][sel], p3[1][sel])
        assert set(nxt[0].tolist()) == keys
        want = count_reference_rows(size, slide, agg, [p1, race, nxt])[2]
        _cfeed(op, nxt)
        got = cw._rows(op.collect())
        cw._check(got, want, agg)
        assert {r[0] for r in got} == keys                  # every key the table holds fires in this push
        _cstats(op, CAP_E, fired + len(want), 0)
    finally:
        op.close()


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
@pytest.mark.parametrize("agg", COUNT_AGGS, ids=lambda a: a[0])
@pytest.mark.parametrize("how", ["snapshot", "key_groups"])
def test_count_output_capacity(size, slide, agg, how):
    """Case 10.  output_capacity = 64: a push that fires exactly 64 windows is clean (`o < out_cap`,
    fw_count.hip:195); one that fires 65 raises OUTPUT alone (:205), fw_get_stats clamps
    results_available to 64 (fw_api.hip:2262), collect() refuses, and the rings have moved on
    (:211-221).  The whole-handle snapshot of before the push into the same handle (clears `error` and
    `out_count[0]`, fw_folded.hip:213-214), or key-group snapshots into a fresh one, and the push in two parts
    deliver the 65 exactly."""
    c = case10(size, slide)
    (k1, v1), (k2, v2) = c["pushes"]
    cut = c["cut"]
    want = count_reference_rows(size, slide, agg, [(k1, v1), (k2[:cut], v2[:cut]), (k2[cut:], v2[cut:])])
    assert [len(w) for w in want] == [OUT_CAP, 32, 33]
    op, fresh = _cop(size, slide, agg, output_capacity=OUT_CAP), None
    try:
        _cfeed(op, (k1, v1), shared=False)
        cw._check(cw._rows(op.collect()), want[0], agg)
        _cstats(op, 64, 64, 0)
        if how == "snapshot":
            blob = op.snapshot_state()
        else:
            blobs, _ = op.handle.snapshot_key_groups()
        _cfeed(op, (k2, v2), shared=False)
        assert _cstats(op, 65, 64 + 65, OUTPUT)["results_available"] == OUT_CAP
        _refused(op.collect)
        if how == "snapshot":
            op.initialize_state(blob)
            target, fired = op, 64 + 65
        else:
            target = fresh = _cop(size, slide, agg, output_capacity=OUT_CAP)
            fresh.handle.restore_key_groups(blobs, [])
            fired = 0
        assert _cstats(target, 64, fired, 0)["results_available"] == 0
        for i, part in ((1, (k2[:cut], v2[:cut])), (2, (k2[cut:], v2[cut:]))):
            _cfeed(target, part, shared=False)
            cw._check(cw._rows(target.collect()), want[i], agg)
            fired += len(want[i])
        _cstats(target, 65, fired, 0)
    finally:
        op.close()
        if fresh is not None:
            fresh.close()
