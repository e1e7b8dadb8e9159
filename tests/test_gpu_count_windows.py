"""Count windows (KeyedStream.countWindow) on the GPU against the element-list reference
(count_window_reference.py): keys, aggregates, window bounds and the emission order, row for row.

Integers and DOUBLE min / max compare exactly (a NaN as the canonical NaN); DOUBLE sums at 1e-9
relative, the project's DOUBLE-sum rule: the device adds count-slice partials, the reference adds
left to right, and for <= 250 addends in [0, 1000) the two differ by about 250 * 2^-53 relative.
Shapes are the smallest that cross every boundary: a tile holds 1024 rows, so 10 000 rows of one key
give many fires per tile, windows that straddle tiles and -- split into pushes -- pushes."""
import ctypes as C
import re

import numpy as np
import pytest
from count_window_reference import CountWindowReference

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

PAIRS = [(250, 150), (3, 5), (5, 1), (6, 4), (4, 2), (1, 1), (7, 7), (16, 1)]
LONG_MAX = (1 << 63) - 1
_CANON_NAN = 0x7FF8000000000000
_SPECIAL = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF00000DEADBEEF,
                     0x8000000000000000, 0, np.float64(1.0).view(np.int64), np.float64(-1.0).view(np.int64)],
                    dtype=np.uint64).view(np.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op(size, slide, agg=("sum", "LONG"), **kw):
    from flink_amd.datastream import CountWindowOperator
    kw.setdefault("max_batch_rows", 1 << 14)
    kw.setdefault("output_capacity", 1 << 16)
    return CountWindowOperator(size, slide, agg, **kw).open()


def _canon(bits):
    return _CANON_NAN if np.isnan(np.int64(bits).view(np.float64)) else int(bits)


def _rows(res):
    return list(zip(res["key"].tolist(), res["value"].tolist(), res["window_start"].tolist(), res["window_end"].tolist(),
                    res["trigger_ord"].tolist()))


def _ords(want, sizes):
    """the reference's arrival indices as push_seq << 32 | row, for pushes of the given sizes (empty
    pushes are not counted: fw_commit / fw_push_device of 0 rows returns at once)"""
    starts = np.cumsum([0] + [s for s in sizes if s > 0])
    out = []
    for k, v, ws, we, at in want:
        p = int(np.searchsorted(starts, at, side="right")) - 1
        out.append((k, v, ws, we, (p << 32) | (at - int(starts[p]))))
    return out


def _check(got, want, agg):
    fn, ftype = agg
    assert len(got) == len(want)
    if ftype == "DOUBLE" and fn in ("min", "max"):
        got = [(k, _canon(v), ws, we, o) for k, v, ws, we, o in got]
        want = [(k, _canon(v), ws, we, o) for k, v, ws, we, o in want]
    if ftype == "DOUBLE" and fn == "sum":
        assert [(g[0],) + g[2:] for g in got] == [(w[0],) + w[2:] for w in want]
        gv = np.array([g[1] for g in got], np.int64).view(np.float64)
        wv = np.array([w[1] for w in want], np.int64).view(np.float64)
        np.testing.assert_allclose(gv, wv, rtol=1e-9, atol=0)
    else:
        assert got == want


def _run(op, pushes, device=False):
    """pushes: [(keys, values)]; returns the rows collected after every push, concatenated"""
    import torch
    got = []
    for k, v in pushes:
        if device:
            if len(k):
                op.process_batch_device(torch.tensor(np.asarray(k, np.int64), device="cuda"),
                                        torch.tensor(np.asarray(v, np.int64), device="cuda"))
        else:
            op.process_batch(k, v)
        got += _rows(op.collect())
    return got


# ---- hot key: many fires per tile, windows straddling tiles and pushes -----------------------------
_HOT_N = 10_000
_hot_cache = {}


def _hot(size, slide):
    if (size, slide) not in _hot_cache:
        vals = np.random.default_rng(size * 1000 + slide).integers(-10**6, 10**6, _HOT_N).astype(np.int64)
        want = CountWindowReference(size, slide, ("sum", "LONG")).process([42] * _HOT_N, vals.tolist())
        _hot_cache[(size, slide)] = (vals, want)
    return _hot_cache[(size, slide)]


@pytest.mark.parametrize("size,slide", PAIRS)
@pytest.mark.parametrize("n_pushes", [1, 10, 100])
def test_hot_key(size, slide, n_pushes):
    vals, want = _hot(size, slide)
    per = _HOT_N // n_pushes
    op = _op(size, slide)
    try:
        keys = np.full(per, 42, np.int64)
        got = _run(op, [(keys, vals[i * per:(i + 1) * per]) for i in range(n_pushes)])
        _check(got, _ords(want, [per] * n_pushes), ("sum", "LONG"))
        st = op.handle.stats()
        assert st["num_fired_windows"] == len(want) == _HOT_N // slide
        assert st["live_state_entries"] == 1 and st["pending_rows"] == 0 and st["error_flags"] == 0
    finally:
        op.close()


def test_hot_key_device_columns_and_null_ts():
    """process_batch_device pushes with d_ts = NULL; a tumbling form (slide None)"""
    vals, _ = _hot(7, 7)
    want = CountWindowReference(7, None, ("sum", "LONG")).process([42] * _HOT_N, vals.tolist())
    op = _op(7, None)
    try:
        got = _run(op, [(np.full(2500, 42, np.int64), vals[i * 2500:(i + 1) * 2500]) for i in range(4)], device=True)
        _check(got, _ords(want, [2500] * 4), ("sum", "LONG"))
    finally:
        op.close()


# ---- many keys / skew -------------------------------------------------------------------------------
def _stream(seed, n_keys, n_pushes, per, zipf=None, lo=-10**6, hi=10**6):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_pushes):
        if zipf:
            k = np.minimum(rng.zipf(zipf, per), n_keys).astype(np.int64) - 1
        else:
            k = rng.integers(0, n_keys, per).astype(np.int64)
        out.append((k * 977 - 3000, rng.integers(lo, hi, per).astype(np.int64)))
    return out


def _reference(size, slide, agg, pushes):
    ref = CountWindowReference(size, slide, agg)
    want = []
    for k, v in pushes:
        want += ref.process(np.asarray(k).tolist(), np.asarray(v).tolist())
    return _ords(want, [len(k) for k, _ in pushes])


@pytest.mark.parametrize("size,slide", [(250, 150), (6, 4)])
def test_many_keys(size, slide):
    pushes = _stream(size, 5000, 20, 3000)
    op = _op(size, slide)
    try:
        _check(_run(op, pushes), _reference(size, slide, ("sum", "LONG"), pushes), ("sum", "LONG"))
        st = op.handle.stats()
        assert st["live_state_entries"] == len({int(x) for k, _ in pushes for x in k}) and st["error_flags"] == 0
    finally:
        op.close()


@pytest.mark.parametrize("size,slide,agg", [(250, 150, ("sum", "LONG")), (5, 1, ("max", "LONG"))])
def test_skew(size, slide, agg):
    pushes = _stream(7, 2000, 8, 4096, zipf=1.1)
    op = _op(size, slide, agg)
    try:
        _check(_run(op, pushes), _reference(size, slide, agg, pushes), agg)
    finally:
        op.close()


# ---- types ----------------------------------------------------------------------------------------
def test_int_sum_wraps_at_32_bits():
    pushes = _stream(3, 40, 4, 2000, lo=(1 << 31) - 5000, hi=1 << 31)
    op = _op(6, 4, ("sum", "INT"))
    try:
        got = _run(op, pushes)
        _check(got, _reference(6, 4, ("sum", "INT"), pushes), ("sum", "INT"))
        assert any(v < 0 for _, v, _, _, _ in got)   # sums of values near 2^31 wrapped
    finally:
        op.close()


@pytest.mark.parametrize("fn", ["min", "max"])
def test_double_min_max_special_values(fn):
    rng = np.random.default_rng(11)
    pushes = []
    for k, _ in _stream(5, 30, 4, 2000):
        dv = (rng.random(len(k)) * 100.0 - 50.0).view(np.int64).copy()
        sp = rng.random(len(k)) < 0.4
        dv[sp] = _SPECIAL[rng.integers(0, len(_SPECIAL), int(sp.sum()))]
        pushes.append((k, dv))
    op = _op(4, 2, (fn, "DOUBLE"))
    try:
        _check(_run(op, pushes), _reference(4, 2, (fn, "DOUBLE"), pushes), (fn, "DOUBLE"))
    finally:
        op.close()


def test_double_sum():
    rng = np.random.default_rng(13)
    pushes = [(k, (rng.random(len(k)) * 1000.0).view(np.int64).copy()) for k, _ in _stream(9, 20, 4, 3000)]
    op = _op(250, 150, ("sum", "DOUBLE"))
    try:
        _check(_run(op, pushes), _reference(250, 150, ("sum", "DOUBLE"), pushes), ("sum", "DOUBLE"))
    finally:
        op.close()


def test_count():
    pushes = _stream(17, 25, 3, 2000)
    op = _op(3, 5, ("count", "LONG"))
    try:
        got = _run(op, pushes)
        _check(got, _reference(3, 5, ("count", "LONG"), pushes), ("count", "LONG"))
        assert {v for _, v, _, _, _ in got} == {3}
    finally:
        op.close()


# ---- degenerate pushes, watermarks -------------------------------------------------------------------
def test_single_row_and_empty_pushes():
    rng = np.random.default_rng(19)
    k = rng.integers(0, 3, 60).astype(np.int64)
    v = rng.integers(-100, 100, 60).astype(np.int64)
    pushes = []
    for i in range(60):
        pushes.append((k[i:i + 1], v[i:i + 1]))
        if i % 7 == 0:
            pushes.append((k[:0], v[:0]))   # an empty push changes nothing, not even the ordinals
    op = _op(4, 2)
    try:
        _check(_run(op, pushes), _reference(4, 2, ("sum", "LONG"), pushes), ("sum", "LONG"))
    finally:
        op.close()


def test_no_fire_on_watermark():
    op = _op(4, 2)
    try:
        op.process_batch(np.array([1, 1, 1, 2], np.int64), np.array([5, 6, 7, 8], np.int64))
        assert [r[:2] for r in _rows(op.collect())] == [(1, 11)]
        fired = op.handle.stats()["num_fired_windows"]
        res = op.process_watermark(LONG_MAX)   # end of input: the partial windows are never emitted
        assert len(res["key"]) == 0 and len(_rows(op.collect())) == 0
        st = op.handle.stats()
        assert st["num_fired_windows"] == fired == 1 and st["current_watermark"] == LONG_MAX
        op.handle.flush()
        assert len(_rows(op.collect())) == 0
    finally:
        op.close()


# ---- WindowWordCount ------------------------------------------------------------------------------
_TEXT = """To be, or not to be,--that is the question:--
Whether 'tis nobler in the mind to suffer
The slings and arrows of outrageous fortune
Or to take arms against a sea of troubles,
And by opposing end them?--To die,--to sleep,--
No more; and by a sleep to say we end
The heartache, and the thousand natural shocks
That flesh is heir to,--'tis a consummation
Devoutly to be wish'd. To die,--to sleep;--
To sleep! perchance to dream:--ay, there's the rub;
For in that sleep of death what dreams may come,
When we have shuffled off this mortal coil,
Must give us pause: there's the respect
That makes calamity of so long life;
For who would bear the whips and scorns of time,
The oppressor's wrong, the proud man's contumely,
The pangs of despis'd love, the law's delay,
The insolence of office, and the spurns
That patient merit of the unworthy takes,
When he himself might his quietus make
With a bare bodkin? who would these fardels bear,
To grunt and sweat under a weary life,
But that the dread of something after death,--
The undiscover'd country, from whose bourn
No traveller returns,--puzzles the will,
And makes us rather bear those ills we have
Than fly to others that we know not of?
Thus conscience does make cowards of us all;
And thus the native hue of resolution
Is sicklied o'er with the pale cast of thought;
And enterprises of great pith and moment,
With this regard, their currents turn awry,
And lose the name of action.--Soft you now!
The fair Ophelia!--Nymph, in thy orisons
Be all my sins remember'd."""


def test_window_word_count():
    """WindowWordCount as shipped: tokenise (lower case, split on \\W+), keyBy(word),
    countWindow(250, 150).sum(1) of ones -- STRING keys, records in the reference's order"""
    words = [w for w in re.split(r"\W+", _TEXT.lower()) if w]
    assert len(set(words)) > 150
    stream = words * 22
    counts = {}
    for w in stream:
        counts[w] = counts.get(w, 0) + 1
    assert sum(c >= 300 for c in counts.values()) >= 2 and sum(150 <= c < 300 for c in counts.values()) >= 2
    ref = CountWindowReference(250, 150, ("sum", "INT"))
    op = _op(250, 150, ("sum", "INT"), key_type="STRING")
    try:
        got, want = [], []
        for o in range(0, len(stream), 1500):
            chunk = stream[o:o + 1500]
            op.process_batch(chunk, np.ones(len(chunk), np.int64))
            got += op.output_records(op.collect())
            want += [(k, v, LONG_MAX) for k, v, _, _, _ in ref.process(chunk, [1] * len(chunk))]
        assert got == want and len(want) >= 6
        assert {v for _, v, _ in got} == {150, 250}
    finally:
        op.close()


# ---- sharding -------------------------------------------------------------------------------------
def _dest(keys, p):
    d = np.empty(len(keys), np.int32)
    k = np.ascontiguousarray(keys, np.int64)
    _native.check(_native.lib().fw_host_assign_key_groups(k.ctypes.data, None, len(k), abi.KEYHASH_LONG, 128, p, None,
                                                          d.ctypes.data))
    return d


def test_sharding_two_subtasks():
    pushes = _stream(23, 300, 6, 3000)
    want = _reference(6, 4, ("sum", "LONG"), pushes)
    ops = [_op(6, 4, parallelism=2, subtask_index=i) for i in range(2)]
    try:
        got = []
        for k, v in pushes:
            d = _dest(k, 2)
            for i, op in enumerate(ops):
                op.process_batch(k[d == i], v[d == i])
                got += _rows(op.collect())
        assert sorted(g[:4] for g in got) == sorted(w[:4] for w in want)
        assert all(op.handle.stats()["error_flags"] == 0 for op in ops)
        # a row pushed to the wrong subtask
        k, _ = pushes[0]
        stray = k[_dest(k, 2) == 1][:1]
        ops[0].process_batch(stray, np.ones(1, np.int64))
        assert ops[0].handle.stats()["error_flags"] & abi.ERRF["KEYGROUP"]
    finally:
        for op in ops:
            op.close()


# ---- checkpoint -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key_type", ["LONG", "STRING"])
def test_snapshot_restore_continues(key_type):
    pushes = _stream(29, 200, 20, 1500)
    if key_type == "STRING":
        pushes = [([f"w{int(x)}" for x in k], v) for k, v in pushes]
    want = _reference(6, 4, ("sum", "LONG"), pushes)
    a = _op(6, 4, key_type=key_type)
    b = None
    try:
        got = []
        for k, v in pushes[:7]:
            a.process_batch(k, v)
            got += _rows(a.collect())
        blob = a.snapshot_state()
        a.close()
        b = _op(6, 4, key_type=key_type)
        b.initialize_state(blob)
        assert b.handle.stats()["live_state_entries"] == len({x for k, _ in pushes[:7] for x in np.asarray(k).tolist()})
        for k, v in pushes[7:]:
            b.process_batch(k, v)
            got += _rows(b.collect())
        _check(got, want, ("sum", "LONG"))   # ordinals continue, Strings map to the same ids
    finally:
        a.close()
        if b is not None:
            b.close()


def test_key_group_snapshots_rescale_1_to_2():
    pushes = _stream(31, 300, 10, 2000)
    want = _reference(250, 150, ("sum", "LONG"), pushes)
    a = _op(250, 150)
    ops = []
    try:
        got = []
        for k, v in pushes[:5]:
            a.process_batch(k, v)
            got += _rows(a.collect())
        blobs, _ = a.handle.snapshot_key_groups()
        assert len(blobs) == 128
        a.close()
        ops = [_op(250, 150, parallelism=2, subtask_index=i) for i in range(2)]
        for op in ops:
            op.handle.restore_key_groups(blobs, [])
        assert sum(op.handle.stats()["live_state_entries"] for op in ops) == len({int(x) for k, _ in pushes[:5] for x in k})
        for k, v in pushes[5:]:
            d = _dest(k, 2)
            for i, op in enumerate(ops):
                op.process_batch(k[d == i], v[d == i])
                got += _rows(op.collect())
        assert sorted(g[:4] for g in got) == sorted(w[:4] for w in want)
        assert all(op.handle.stats()["error_flags"] == 0 for op in ops)
    finally:
        a.close()
        for op in ops:
            op.close()


# ---- capacity, refused calls ------------------------------------------------------------------------
def test_output_capacity():
    op = _op(1, 1, output_capacity=16)
    try:
        for i in range(4):   # collected in time: clean
            op.process_batch(np.full(10, 5, np.int64), np.arange(10, dtype=np.int64))
            assert len(_rows(op.collect())) == 10
        assert op.handle.stats()["error_flags"] == 0
        op.process_batch(np.full(40, 5, np.int64), np.arange(40, dtype=np.int64))   # 40 fires pending
        with pytest.raises(_native.FlinkWinError) as e:
            op.collect()
        assert e.value.code == abi.FW_E_CAPACITY
        assert op.handle.stats()["error_flags"] & abi.ERRF["OUTPUT"]
    finally:
        op.close()


def test_state_capacity_raises_state_flag():
    op = _op(4, 2, state_capacity=1, max_parallelism=1)   # the smallest table: 2 superbuckets of 1024 slots
    try:
        op.process_batch(np.arange(3000, dtype=np.int64), np.ones(3000, np.int64))
        assert op.handle.stats()["error_flags"] & abi.ERRF["STATE"]
        with pytest.raises(_native.FlinkWinError) as e:
            op.collect()
        assert e.value.code == abi.FW_E_CAPACITY
    finally:
        op.close()


def test_calls_a_count_handle_refuses():
    op = _op(4, 2)
    try:
        h, L = op.handle, _native.lib()
        for call in (h.results_async, h.results_ready, h.result_segments, h.late_records, h.first_element_events,
                     lambda: h.device_results_async("cuda"), lambda: h.snapshot_key_group_heap(0),
                     lambda: h.ds_key_group_windows(0)):
            with pytest.raises(_native.FlinkWinError, match="not for count windows") as e:
                call()
            assert e.value.code == abi.FW_E_INVALID
        assert L.fw_push_device_segments(h._h, 0, 1, None, None, None, None, None, None) == abi.FW_E_INVALID
        assert L.fw_push_device_packed_segments(h._h, 0, 1, None, None, 3) == abi.FW_E_INVALID
        assert L.fw_push_device_key_rows(h._h, 0, None, None, None, None, None) == abi.FW_E_INVALID
    finally:
        op.close()
