"""Count windows behind the N > 1 keyBy exchange, one process: the hand-built padded receive buffers
of tests/count_exchange_cases.py pushed through fw_push_device_count_segments /
fw_push_device_count_packed_segments into a count handle of parallelism 2.

Arrival order is the whole semantics of a count window, and the buffer's position order is the
arrival order: every case is compared, row by row in trigger_ord order, with the count-window
reference (count_window_reference.py) fed the live rows in buffer position order, and bit for bit
with a twin handle that takes the same live rows, compacted, through fw_push_device.  A segmented
call is cut into launches by buffer position (rows 2048 and 4096 here) and a fold tile holds up to
1024 rows of one superbucket of one launch, so the twin is pushed each launch's live rows as a call of
its own: its tiles then hold the same rows in the same order, and DOUBLE sums -- whose last bit
depends on where a tile ends -- are bit-equal too.  Integers and min / max compare bit-exact with the
reference, DOUBLE sums at parity_common.REL_TOL (the reference adds left to right, the device by
count slices).  tests/test_count_exchange_inputs.py checks, without
a GPU, that the cases reach the edges they are built for.
"""
import numpy as np
import pytest
from count_window_reference import CountWindowReference
from parity_common import REL_TOL

import count_exchange_cases as cases
from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

CFG = dict(max_parallelism=cases.MAX_P, parallelism=cases.PARALLELISM, subtask_index=cases.SUBTASK, state_capacity=1 << 12,
           max_batch_rows=cases.MAX_BATCH_ROWS, output_capacity=1 << 14)
# (aggregation, the value kind of count_exchange_cases.values)
AGGS = [(("sum", "LONG"), "LONG"), (("sum", "INT"), "INT"), (("max", "DOUBLE"), "DOUBLE_SPECIAL"), (("sum", "DOUBLE"), "DOUBLE"),
        (("count", "LONG"), "LONG")]
KEY_KINDS = {"packed": ["LONG", "INT"], "soa": ["LONG", "INT", "HOST_HASHED"]}
CASES = [(layout, w, a, KEY_KINDS[layout][(wi + ai) % len(KEY_KINDS[layout])])
         for layout in ("soa", "packed") for wi, w in enumerate(cases.WINDOWS) for ai, a in enumerate(range(len(AGGS)))]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(window, agg=("sum", "LONG"), key_type="LONG", **kw):
    from flink_amd.datastream import CountWindowOperator
    cfg = dict(CFG)
    cfg.update(kw)
    return CountWindowOperator(window[0], window[1], agg, key_type=key_type, **cfg).open()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _push_padded(op, layout, p, values=True):
    sc = _dev(np.asarray(p["counts"], dtype=np.int64))
    if layout == "packed":
        rows = np.stack([p["keys"], np.full(len(p["keys"]), -(1 << 63) + 1, np.int64), p["values"]], axis=1)  # (the ts word is never read)
        op.process_packed_segments_device(sc, _dev(rows.reshape(-1)), 3)
    else:
        op.process_segments_device(sc, _dev(p["keys"]), _dev(p["values"]) if values else None,
                                   _dev(p["hashes"]) if p["hashes"] is not None else None)


def _push_compact(op, k, v, h):
    op.process_batch_device(_dev(k), _dev(v), _dev(h) if h is not None else None)


def _push_compact_by_launch(twin, p):
    """The live rows of a padded buffer into the twin, the live rows of each launch of the segmented
    call (max_batch_rows buffer rows) as a push of its own.  Returns {buffer position: the twin's
    ordinal of that row}."""
    launch = p["pos"] // cases.MAX_BATCH_ROWS
    ords = {}
    for la in np.unique(launch):
        m = launch == la
        seq = twin.handle.push_seq
        _push_compact(twin, p["live_keys"][m], p["live_values"][m], p["live_hashes"][m] if p["live_hashes"] is not None else None)
        assert twin.handle.push_seq == seq + 1
        ords.update({int(pos): (seq << 32) | i for i, pos in enumerate(p["pos"][m])})
    return ords


def _rows(res):
    return list(zip(res["key"].tolist(), res["value"].tolist(), res["window_start"].tolist(), res["window_end"].tolist(),
                    res["trigger_ord"].tolist()))


def _canon(bits):
    return cases.NAN_BITS if np.isnan(np.int64(bits).view(np.float64)) else int(bits)


def _check_reference(got, want, agg):
    """got: device rows in trigger_ord order (key, value, start, end, ord); want: the reference's in
    emission order, the ordinal already push_seq << 32 | buffer position"""
    fn, ftype = agg
    assert len(got) == len(want)
    assert [(g[0],) + g[2:] for g in got] == [(w[0],) + w[2:] for w in want]
    if ftype == "DOUBLE" and fn == "sum":
        gv = np.array([g[1] for g in got], np.int64).view(np.float64)
        wv = np.array([w[1] for w in want], np.int64).view(np.float64)
        np.testing.assert_allclose(gv, wv, rtol=REL_TOL, atol=0)
    elif ftype == "DOUBLE":
        assert [_canon(g[1]) for g in got] == [_canon(w[1]) for w in want]
    else:
        assert [g[1] for g in got] == [w[1] for w in want]


def _reference_rows(ref, pushes, b, first_push_seq=0):
    """the reference's rows of push b, their arrival indices turned into the expected ordinals"""
    p = pushes[b]
    base = ref.arrived
    out = []
    for k, v, ws, we, at in ref.process(p["live_keys"].tolist(), p["live_values"].tolist()):
        out.append((k, v, ws, we, ((first_push_seq + b) << 32) | int(p["pos"][at - base])))
    return out


def _clean(op):
    s = op.handle.stats()
    assert s["error_flags"] == 0, s["error_flags"]   # no FW_ERRF_KEYGROUP: no padding row was routed
    return s


@pytest.mark.parametrize("layout,window,agg_i,key_kind", CASES)
def test_padded_push_equals_compacted_twin_and_reference(layout, window, agg_i, key_kind):
    agg, value_kind = AGGS[agg_i]
    pushes, extra = cases.build_case(key_kind, value_kind)
    op, twin = _op(window, agg, key_kind), _op(window, agg, key_kind)
    ref = CountWindowReference(window[0], window[1], agg)
    try:
        for b, p in enumerate(pushes):
            # a count aggregate's SoA push may leave the value column out
            _push_padded(op, layout, p, values=not (agg[0] == "count" and b % 2))
            twin_ord = _push_compact_by_launch(twin, p)
            got, got_twin = _rows(op.collect()), _rows(twin.collect())
            want = _reference_rows(ref, pushes, b)
            assert len(want) > 0
            _check_reference(got, want, agg)
            # the twin: bit-equal rows, its ordinals those of the compacted rows
            assert [g[:4] for g in got] == [g[:4] for g in got_twin]
            assert [g[4] >> 32 for g in got] == [b] * len(got)
            assert [twin_ord[g[4] & 0xFFFFFFFF] for g in got] == [g[4] for g in got_twin]
            s, st = _clean(op), _clean(twin)
            assert s["live_state_entries"] == st["live_state_entries"] and s["num_fired_windows"] == st["num_fired_windows"]
        # equal state: one more identical compact push fires identical rows
        for o in (op, twin):
            _push_compact(o, *extra)
        got, got_twin = _rows(op.collect()), _rows(twin.collect())
        assert len(got) > 0 and [g[:4] for g in got] == [g[:4] for g in got_twin]
        assert [g[4] - (len(pushes) << 32) for g in got] == [g[4] - ((twin.handle.push_seq - 1) << 32) for g in got_twin]
        _clean(op)
    finally:
        op.close()
        twin.close()


def test_live_foreign_row_is_dropped_and_flagged():
    window, agg = (5, 3), ("sum", "LONG")
    hot, own, foreign = cases.keys_of("LONG")
    rng = np.random.default_rng(5)
    counts = (1500, 0, 1237)
    q = cases.build_push(rng, "LONG", "LONG", counts)   # padding of foreign keys and the hot key: raises nothing
    p = cases.build_push(rng, "LONG", "LONG", counts)
    extra = cases.build_push(rng, "LONG", "LONG", (1500, 0, 0))
    bad = 1500 + 500   # a live row of the third segment inside a full partition chunk: rows 3072 .. 4095, the second launch's
    assert p["pos"][bad] == 2 * cases.SEG_LEN + 500 and 3072 <= p["pos"][bad] < 4096
    p["keys"][p["pos"][bad]] = foreign[0]
    keep = np.arange(len(p["pos"])) != bad
    op, twin, fresh = _op(window, agg), _op(window, agg), None
    ref = CountWindowReference(window[0], window[1], agg)
    try:
        _push_padded(op, "soa", q)
        _push_compact(twin, q["live_keys"], q["live_values"], None)
        got = _rows(op.collect())
        assert len(got) > 0 and [g[:4] for g in got] == [g[:4] for g in _rows(twin.collect())]
        _clean(op)
        n0 = len(ref.process(q["live_keys"].tolist(), q["live_values"].tolist()))
        _push_padded(op, "packed", p)
        _push_compact(twin, p["live_keys"][keep], p["live_values"][keep], None)
        n1 = len(ref.process(p["live_keys"][keep].tolist(), p["live_values"][keep].tolist()))
        s, st = op.handle.stats(), _clean(twin)
        assert s["error_flags"] == abi.ERRF["KEYGROUP"]
        # every other row folded as if the foreign one were absent
        assert s["num_fired_windows"] == st["num_fired_windows"] == n0 + n1
        assert s["results_available"] == st["results_available"] == n1
        assert s["live_state_entries"] == st["live_state_entries"]
        # the flag is sticky and fw_results reports it, so the state is read through a checkpoint (a
        # restore starts with clean flags): one more push fires what the twin and the reference fire
        fresh = _op(window, agg)
        fresh.initialize_state(op.snapshot_state())
        twin.collect()
        _push_padded(fresh, "soa", extra)
        _push_compact(twin, extra["live_keys"], extra["live_values"], None)
        got, want = _rows(fresh.collect()), ref.process(extra["live_keys"].tolist(), extra["live_values"].tolist())
        assert len(got) > 0 and [g[:4] for g in got] == [g[:4] for g in _rows(twin.collect())] == [w[:4] for w in want]
        _clean(fresh)
    finally:
        op.close()
        twin.close()
        if fresh is not None:
            fresh.close()


def test_refusals():
    import torch
    from flink_amd.datastream import CountWindowOperator, SessionWindowOperator, WindowOperator
    from flink_amd.datastream import TumblingEventTimeWindows, EventTimeTrigger
    cnt = torch.ones(1, dtype=torch.int64, device="cuda")
    col = torch.zeros(8, dtype=torch.int64, device="cuda")
    h32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    kw = dict(max_parallelism=cases.MAX_P, subtask_index=0, max_batch_rows=2048, output_capacity=1 << 12)
    p1 = CountWindowOperator(4, None, ("sum", "LONG"), parallelism=1, **kw).open()
    ses = SessionWindowOperator(50, ("sum", "LONG"), parallelism=2, **kw).open()
    tw = WindowOperator(TumblingEventTimeWindows.of(1000), EventTimeTrigger.create(), ("sum", "LONG"), parallelism=2, **kw).open()
    for op, why in ((p1, "parallelism 1"), (ses, "not for session windows"), (tw, "not for time windows")):
        try:
            h = op.handle
            for call in (lambda: h.push_device_count_segments(cnt, col[:1], col[:1]),
                         lambda: h.push_device_count_packed_segments(cnt, col[:3], 3)):
                with pytest.raises(_native.FlinkWinError, match=why) as e:
                    call()
                assert e.value.code == abi.FW_E_INVALID
        finally:
            op.close()
    op = _op((4, None))
    try:
        for words in (2, 4):   # row_words must be 2 + value columns = 3
            with pytest.raises(_native.FlinkWinError, match="row_words") as e:
                op.handle.push_device_count_packed_segments(cnt, col[:words], words)
            assert e.value.code == abi.FW_E_INVALID
        assert _clean(op)["live_state_entries"] == 0
    finally:
        op.close()
    op = _op((4, None), key_type="HOST_HASHED")   # packed rows carry no key hashes
    try:
        with pytest.raises(_native.FlinkWinError, match="key-hash") as e:
            op.process_packed_segments_device(cnt, col[:3], 3)
        assert e.value.code == abi.FW_E_INVALID
        with pytest.raises(_native.FlinkWinError, match="key_hash column required"):
            op.process_segments_device(cnt, col[:1], col[:1], None)
        op.process_segments_device(cnt, col[:1], col[:1], h32[:1])   # (with its hashes it is taken)
    finally:
        op.close()
    op = _op((4, None), key_type="STRING")
    try:
        for call in (lambda: op.process_segments_device(cnt, col[:1], col[:1], h32[:1]),
                     lambda: op.process_packed_segments_device(cnt, col[:3], 3)):
            with pytest.raises(ValueError, match="STRING"):
                call()
    finally:
        op.close()


def test_output_capacity_exact_and_one_more():
    """2000 rows of one owned key under countWindow(4): 500 fires.  output_capacity 500 is filled
    exactly and stays clean; 499 loses one row and raises FW_ERRF_OUTPUT -- on the twin alike."""
    hot, own, foreign = cases.keys_of("LONG")
    rng = np.random.default_rng(3)
    counts = (1500, 0, 500)
    pos = cases.live_positions(counts)
    keys = rng.choice(foreign, cases.N_SEGS * cases.SEG_LEN)
    keys[pos] = hot
    vals = rng.integers(-10**6, 10**6, len(keys)).astype(np.int64)
    p = dict(counts=counts, keys=keys, values=vals, hashes=None)
    for cap, flag in ((500, 0), (499, abi.ERRF["OUTPUT"])):
        op, twin = _op((4, None), output_capacity=cap), _op((4, None), output_capacity=cap)
        try:
            _push_padded(op, "packed", p)
            _push_compact(twin, keys[pos], vals[pos], None)
            s, st = op.handle.stats(), twin.handle.stats()
            assert s["error_flags"] == st["error_flags"] == flag
            assert s["results_available"] == st["results_available"] == cap
            assert s["num_fired_windows"] == st["num_fired_windows"] == 500
        finally:
            op.close()
            twin.close()


def test_snapshot_after_push_2_restores_into_a_fresh_handle():
    window, agg = (250, 150), ("sum", "INT")
    pushes, _ = cases.build_case("LONG", "INT")
    op, fresh = _op(window, agg), None
    ref = CountWindowReference(window[0], window[1], agg)
    try:
        for b in range(2):
            _push_padded(op, "packed" if b else "soa", pushes[b])
            _check_reference(_rows(op.collect()), _reference_rows(ref, pushes, b), agg)
        fresh = _op(window, agg)
        fresh.initialize_state(op.snapshot_state())
        for b in range(2, 4):
            for o in (op, fresh):
                _push_padded(o, "packed" if b % 2 else "soa", pushes[b])
            got = _rows(fresh.collect())
            assert got == _rows(op.collect())                      # the same rows, the same ordinals
            _check_reference(got, _reference_rows(ref, pushes, b), agg)
        assert _clean(fresh)["live_state_entries"] == _clean(op)["live_state_entries"]
    finally:
        op.close()
        if fresh is not None:
            fresh.close()


def test_snapshot_carries_the_device_watermark():
    import torch
    window = (4, None)
    op, fresh, fresh_kg = _op(window), None, None
    try:
        w = 1_600_000_000_123
        op.handle.advance(w - 500)                              # the host mirror, below the device value
        res = op.process_watermark_device(torch.tensor([w], dtype=torch.int64, device="cuda"))
        assert len(res["key"]) == 0 and len(res["trigger_ord"]) == 0   # nothing fires on a watermark
        assert op.handle.stats()["current_watermark"] == w
        fresh = _op(window)
        fresh.initialize_state(op.snapshot_state())
        assert fresh.handle.stats()["current_watermark"] == w
        # never advanced from the device: the host mirror, as before
        fresh_kg = _op(window)
        fresh_kg.handle.advance(77)
        again = _op(window)
        try:
            again.initialize_state(fresh_kg.snapshot_state())
            assert again.handle.stats()["current_watermark"] == 77
        finally:
            again.close()
    finally:
        for o in (op, fresh, fresh_kg):
            if o is not None:
                o.close()
