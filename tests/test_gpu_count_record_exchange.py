"""Record-shaped count windows behind the N > 1 keyBy exchange: RecordCountWindowOperator(record_types=...)
fed hand-built packed receive buffers (count_record_exchange_cases.py: padded segments, poisoned padding)
through fw_push_device_count_record_packed_segments, its drain running on the record words
fw_count_record_rows gathers on the device.

After every push the operator equals the element-list reference (CountRecordReference over the live
rows in buffer position order) on the records -- bit for bit, record_image --, the emission order,
trigger_ord, record_ord and the set of retained ordinals, and it equals a twin
RecordCountWindowOperator that is fed the compacted live rows as tuples (the twin's ordinals are compact
row indices: they are mapped to buffer positions before comparing).

Everything is bit-exact, DOUBLE sums included: their addends are multiples of 0.5 below 100, so every
partial sum is exact whatever the order of addition (at most 250 * 99.5 < 2^53 * 0.5).
"""
import ctypes as C

import count_exchange_cases as cx
import count_record_exchange_cases as cases
import numpy as np
import pytest
from count_record_reference import CountRecordReference, record_image

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

ROW_WORDS = 2 + cases.F


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(window, aggregation, field=1, types=None, **kw):
    from flink_amd.datastream import RecordCountWindowOperator
    kw.setdefault("parallelism", cx.PARALLELISM)
    kw.setdefault("max_batch_rows", cases.MAX_BATCH_ROWS)
    return RecordCountWindowOperator(window[0], window[1], aggregation, field=field, record_types=types, max_parallelism=cx.MAX_P,
                                     subtask_index=cx.SUBTASK, state_capacity=1 << 12, output_capacity=1 << 16, **kw).open()


def _dev(p):
    import torch
    return (torch.tensor(p["counts"], dtype=torch.int64, device="cuda"), torch.from_numpy(p["rows"]).to("cuda").reshape(-1))


def _push(op, p, row_words=ROW_WORDS):
    counts, rows = _dev(p)
    seq = op.handle.push_seq
    op.process_packed_segments_device(counts, rows, row_words)
    assert op.handle.push_seq == seq + 1   # one call, one push
    return _fired(op)


def _fired(op):
    out = op.collect()
    assert np.all(out["timestamp"] == (1 << 63) - 1)
    return list(zip(out["key"], [record_image(r) for r in out["records"]], out["trigger_ord"].tolist(), out["record_ord"].tolist()))


def _image(rows):
    return [(k, record_image(r), t, o) for k, r, t, o in rows]


def _column(p, ftype):
    return p["live_values"].view(np.float64) if ftype == "DOUBLE" else p["live_values"]


CASES = [(w, a, t, 1) for w in cx.WINDOWS for a in cases.AGGS for t in cases.FTYPES] + \
        [((5, 3), a, t, 3) for a in cases.AGGS for t in cases.FTYPES]


@pytest.mark.parametrize("window,agg,ftype,field", CASES, ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_padded_pushes_equal_reference_and_compacted_twin(window, agg, ftype, field):
    pushes = cases.build_case(agg[0], ftype, field)
    want = cases.reference_run(window, agg, ftype, field)
    aggregation = cases.aggregation(agg, ftype)
    op = _op(window, aggregation, field, cases.record_types(ftype, field))
    twin = _op(window, aggregation, field)   # the host form: any tuples, compacted rows
    try:
        for b, p in enumerate(pushes):
            got = _push(op, p)
            rows, held = want[b]
            assert len(rows) > 0 and got == _image(rows), f"push {b}"
            assert op.retained_ordinals() == held, f"push {b}"
            twin.process_batch(p["live_keys"], _column(p, ftype), p["records"])
            pos = lambda o: (o >> 32 << 32) | int(pushes[o >> 32]["pos"][o & 0xFFFFFFFF])
            assert [(k, r, pos(t), pos(o)) for k, r, t, o in _fired(twin)] == got, f"push {b}"
            assert {pos(o) for o in twin.retained_ordinals()} == op.retained_ordinals()
        st = op.handle.stats()
        assert st["error_flags"] == 0 and st["num_fired_windows"] == sum(len(r) for r, _ in want)
    finally:
        op.close()
        twin.close()


# ---- F = 1 and F = 8 ---------------------------------------------------------------------------------
def _wide_push(rng, b, types, field, counts):
    """a push whose records have len(types) fields: the aggregated one from few values, the others noise"""
    p = cx.build_push(rng, "LONG", "LONG", counts)
    n = cx.N_SEGS * cx.SEG_LEN
    rows = np.empty((n, 2 + len(types)), np.int64)
    rows[:, 0] = p["keys"]
    rows[:, 1] = -1
    for f, t in enumerate(types):
        if f == field:
            rows[:, 2 + f] = cases.field_words(rng, n, "minBy", t)
        elif t == "INT":
            rows[:, 2 + f] = rng.integers(-2**31, 2**31, n)
        elif t == "DOUBLE":
            rows[:, 2 + f] = (rng.integers(-1000, 1000, n) * 0.125).view(np.int64)
        else:
            rows[:, 2 + f] = rng.integers(-2**62, 2**62, n)
    p["rows"] = rows
    p["records"] = cases.words_to_tuples(rows[p["pos"], 2:], types)
    return p


@pytest.mark.parametrize("types,field,agg", [(["LONG"], 0, ("sum", "LONG")), (["LONG"], 0, ("maxBy", "LONG", True)),
                                              (["INT", "DOUBLE", "LONG", "LONG", "DOUBLE", "DOUBLE", "INT", "LONG"], 5, ("minBy", "DOUBLE", False)),
                                              (["LONG", "DOUBLE", "INT", "INT", "INT", "DOUBLE", "LONG", "INT"], 7, ("sum", "INT"))],
                         ids=["F1-sum", "F1-maxBy", "F8-minBy-last-DOUBLE", "F8-sum-INT"])
def test_one_and_eight_fields(types, field, agg):
    rng = np.random.default_rng(11)
    pushes = [_wide_push(rng, b, types, field, c) for b, c in enumerate(cx.COUNTS[:3])]
    ref = CountRecordReference(5, 3, agg, field=field)
    op = _op((5, 3), agg, field, types)
    try:
        for b, p in enumerate(pushes):
            got = _push(op, p, 2 + len(types))
            assert got == _image(ref.process(p["live_keys"].tolist(), p["records"], cases.ordinals(p, b))) and got
            assert op.retained_ordinals() == ref.held()
        assert op.handle.stats()["error_flags"] == 0
    finally:
        op.close()


# ---- a spill push after a segment push ---------------------------------------------------------------------
def test_spill_push_after_a_segment_push():
    """one step of the exchange: the padded segments, then the overflow round's rows as a one-segment
    call of the same entry (a full segment: no padding), each drained on its own"""
    window, agg = (5, 3), ("minBy", "LONG", True)
    rng = np.random.default_rng(3)
    seg = cases.build_record_push(rng, 0, "minBy", "LONG", 1, cx.COUNTS[0])
    spill = cases.build_record_push(rng, 1, "minBy", "LONG", 1, (700,), n_segs=1, seg_len=700)
    again = cases.build_record_push(rng, 2, "minBy", "LONG", 1, cx.COUNTS[1])
    ref = CountRecordReference(window[0], window[1], agg, field=1)
    op = _op(window, agg, 1, cases.record_types("LONG", 1))
    try:
        for b, p in enumerate([seg, spill, again]):
            got = _push(op, p)
            assert got == _image(ref.process(p["live_keys"].tolist(), p["records"], cases.ordinals(p, b))) and got
            assert op.retained_ordinals() == ref.held()
        assert len(spill["pos"]) == 700 and op.handle.push_seq == 3
    finally:
        op.close()


# ---- checkpoint --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agg", [("sum",), ("maxBy", False)], ids=["sum", "maxBy-last"])
def test_snapshot_after_push_two_and_restore(agg):
    window, ftype = (250, 150), "LONG"
    pushes, want = cases.build_case(agg[0], ftype), cases.reference_run(window, agg, ftype)
    a, b = _op(window, cases.aggregation(agg, ftype), 1, cases.record_types(ftype, 1)), None
    try:
        for i in range(2):
            assert _push(a, pushes[i]) == _image(want[i][0])
        blob = a.snapshot_state()
        a.close()
        b = _op(window, cases.aggregation(agg, ftype), 1, cases.record_types(ftype, 1))
        b.initialize_state(blob)
        assert b.retained_ordinals() == want[1][1] and b.handle.push_seq == 2
        for i in range(2, 4):
            assert _push(b, pushes[i]) == _image(want[i][0])
            assert b.retained_ordinals() == want[i][1]
        assert b.handle.stats()["error_flags"] == 0
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- refusals ----------------------------------------------------------------------------------------------
def _refused(rc, *words):
    msg = _native.lib().fw_last_error().decode()
    assert rc == abi.FW_E_INVALID and all(w in msg for w in words), msg


def test_refusals():
    import torch

    from flink_amd.datastream import CountWindowOperator, SessionWindowOperator
    L = _native.lib()
    types = cases.record_types("LONG", 1)
    kw = dict(max_parallelism=cx.MAX_P, parallelism=2, subtask_index=0, state_capacity=1 << 12, max_batch_rows=4096, output_capacity=1 << 14)
    ops = {"record-p1": _op((5, 3), ("sum", "LONG"), 1, types, parallelism=1),
           "count": CountWindowOperator(5, 3, ("sum", "LONG"), **kw).open(),
           "session": SessionWindowOperator(1000, ("sum", "LONG"), **kw).open(),
           "hashed": _op((5, 3), ("sum", "LONG"), 1, types, key_type="HOST_HASHED"),
           "record": _op((5, 3), ("sum", "LONG"), 1, types, max_batch_rows=4096)}
    p = cases.build_record_push(np.random.default_rng(2), 0, "sum", "LONG", 1, (1300, 0, 1000), n_segs=3, seg_len=1300)
    counts, rows = _dev(p)
    out = abi.fw_record_rows()
    try:
        push = lambda name, n_segs=3, seg_len=1300, w=ROW_WORDS: L.fw_push_device_count_record_packed_segments(
            ops[name].handle._h, n_segs, seg_len, counts.data_ptr(), rows.data_ptr(), w)
        gather = lambda name, n_rows=3900, w=ROW_WORDS: L.fw_count_record_rows(ops[name].handle._h, rows.data_ptr(), w, n_rows, C.byref(out))
        for call, fn in ((push, "fw_push_device_count_record_packed_segments"), (gather, "fw_count_record_rows")):
            _refused(call("record-p1"), fn, "parallelism 1")
            _refused(call("count"), fn, "not for count windows")
            _refused(call("session"), fn, "not for session windows")
            _refused(call("record", w=ROW_WORDS + 1), fn, "row_words 7")
        _refused(push("hashed"), "fw_push_device_count_record_packed_segments", "key-hash")
        _refused(push("record", n_segs=4, seg_len=1300), "5200", "4096")   # n_segs * seg_len > max_batch_rows: both numbers
        for name in ops:   # nothing was pushed
            st = ops[name].handle.stats()
            assert st["error_flags"] == 0 and st["live_state_entries"] == 0

        # n_rows below a named position: refused, nothing read out of bounds, nothing consumed
        op, ref = ops["record"], CountRecordReference(5, 3, ("sum", "LONG"), field=1)
        torch.cuda.synchronize()
        assert push("record") == 0
        op.handle.push_seq += 1
        _refused(gather("record", n_rows=1), "fw_count_record_rows", "n_rows is 1")
        op._drain_device(rows, ROW_WORDS)   # the same call with the buffer's n_rows: the events are still there
        assert _fired(op) == _image(ref.process(p["live_keys"].tolist(), p["records"], cases.ordinals(p, 0)))
        assert op.retained_ordinals() == ref.held() and len(ref.held()) > 100
    finally:
        for o in ops.values():
            o.close()


# ---- a live row of a foreign key group -------------------------------------------------------------------
def test_live_foreign_row_is_dropped_and_flagged():
    import torch
    window, agg = (5, 3), ("sum", "LONG")
    types = cases.record_types("LONG", 1)
    hot, own, foreign = cx.keys_of("LONG")
    rng = np.random.default_rng(5)
    counts = (1500, 0, 1237)
    q = cases.build_record_push(rng, 0, "sum", "LONG", 1, counts)
    p = cases.build_record_push(rng, 1, "sum", "LONG", 1, counts)
    extra = cases.build_record_push(rng, 2, "sum", "LONG", 1, (1500, 0, 0))
    bad = 1500 + 500   # a live row of the third segment
    assert p["pos"][bad] == 2 * cx.SEG_LEN + 500
    p["rows"][p["pos"][bad], 0] = foreign[0]
    keep = np.arange(len(p["pos"])) != bad
    op, twin, fresh = _op(window, agg, 1, types), _op(window, agg, 1), None
    ref = CountRecordReference(window[0], window[1], agg, field=1)
    try:
        assert _push(op, q) == _image(ref.process(q["live_keys"].tolist(), q["records"], cases.ordinals(q, 0)))
        twin.process_batch(q["live_keys"], q["live_values"], q["records"])
        twin.collect()
        c, r = _dev(p)
        op.handle.push_device_count_record_packed_segments(c, r, ROW_WORDS)
        kept = [rec for rec, k in zip(p["records"], keep) if k]
        twin.process_batch(p["live_keys"][keep], p["live_values"][keep], kept)
        n1 = len(ref.process(p["live_keys"][keep].tolist(), kept, [o for o, k in zip(cases.ordinals(p, 1), keep) if k]))
        s, st = op.handle.stats(), twin.handle.stats()
        assert s["error_flags"] == abi.ERRF["KEYGROUP"] and st["error_flags"] == 0
        # every other row folded as if the foreign one were absent
        assert s["num_fired_windows"] == st["num_fired_windows"] and s["results_available"] == n1 > 0
        assert s["live_state_entries"] == st["live_state_entries"]
        # the flag is sticky and the reads report it (FW_E_CAPACITY), so the state is read through a
        # checkpoint (a restore starts with clean flags): one more push fires what the reference fires,
        # from the same records
        with pytest.raises(_native.FlinkWinError) as e:
            op.handle.count_record_rows(r, ROW_WORDS)
        assert e.value.code == abi.FW_E_CAPACITY
        fresh = _op(window, agg, 1, types)
        fresh.handle.restore(op.handle.snapshot())
        c, r = _dev(extra)
        fresh.handle.push_device_count_record_packed_segments(c, r, ROW_WORDS)
        g = fresh.handle.count_record_rows(r, ROW_WORDS)
        res = fresh.handle.results()
        order = np.argsort(res["first_ord"], kind="stable")
        want = ref.process(extra["live_keys"].tolist(), extra["records"], cases.ordinals(extra, 2))
        assert len(want) > 0 and fresh.handle.stats()["error_flags"] == 0
        assert list(zip(res["key"][order].tolist(), res["values"][0][order].tolist(), res["first_ord"][order].tolist(),
                        res["values"][1][order].tolist())) == [(k, rec[1], t, o) for k, rec, t, o in want]
        # the gathered words are the records of the rows the results name in this push
        by_ord = dict(zip(cases.ordinals(extra, 2), extra["live_words"].tolist()))
        for j in order.tolist():
            o = int(res["values"][1][j])
            assert bool(g["res_from_push"][j]) == (o >> 32 == 2)
            assert g["res_words"][j].tolist() == (by_ord[o] if o >> 32 == 2 else [0] * cases.F)
        keep_ev = g["ev_is_retain"]
        assert [w.tolist() for w in g["ev_words"][keep_ev]] == [by_ord[o] for o in g["ev_ord"][keep_ev].tolist()]
        assert not g["ev_words"][~keep_ev].any() and (~keep_ev).any() and keep_ev.any()
        torch.cuda.synchronize()
    finally:
        for o in (op, twin, fresh):
            if o is not None:
                o.close()
