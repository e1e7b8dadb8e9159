"""The slicing path (k_ingest*, k_merge_fire, k_merge_hopb, the compaction, the key-row table) at the
limits of its fixed-size buffers.

Every case drives exactly one buffer over its capacity and then checks three things:
 (a) fw_stats.error_flags holds that one bit and no other, fw_get_stats itself still works, the calls
     that read the control block (fw_results, fw_snapshot, fw_late_records, fw_first_element_events)
     fail with FW_E_CAPACITY, the structural bounds of the case hold (conditions, not measurements) and
     fw_destroy succeeds;
 (b) what the contract still delivers is a sub-multiset of the oracle's rows without duplicates;
 (c) recovery: a snapshot taken just before the overflowing pushes is restored into the SAME handle
     (the oracle does snapshot_restore at the same point), error_flags is 0 again, the same input is
     fed in portions that fit, and every watermark's rows equal the oracle's; the run ends with
     error_flags == 0 and the oracle's late-record count.  A kernel that damaged state, timers, cursors
     or fill counters on its way into the overflow fails here.

Each case first runs the oracle alone and asserts that its row counts lie on the intended side of the
capacity, before a handle exists: a mis-sized input fails loudly instead of passing vacuously.  That
oracle run is also the reference of parts (b) and (c).  All compared columns are integers or
bit-exact; nothing here takes a tolerance.

FW_ERRF_CHUNKS has no case: its only sites (the chunk-table checks of k_ingest and k_ingest_pack) are
guarded by the host's own flush once FW_MAX_PENDING pushes are pending and cannot be reached through
the API."""
import numpy as np
import pytest

from flink_amd import abi
from flink_amd._native import FlinkWinError
from parity_common import CASES, I64, _cfg, _compare, _double_cols, _rows

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000_000      # a multiple of 2 s, 4 s and 10 s
MBR = 1 << 14               # max_batch_rows of every case but ORDEV; pushes are exactly this long
CAP = max(2 * MBR, 1 << 16)  # treq_cap = lfire_cap = side_cap (fw_api.hip:774: max(2 * max_batch_rows, 65536))
N_OVER = 5                  # overflowing pushes: 81 920 rows against 65 536
OUT_CAP = 4096              # output_capacity of the OUTPUT cases: 128 superbuckets, 64-row slabs
ERRF = abi.ERRF


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- helpers -----------------------------------------------------------------------------------
def _handle(cfg):
    from flink_amd.runtime.handle import WindowAggHandle
    return WindowAggHandle(cfg)


def _oracle(cfg):
    from oracle.oracle import OracleOperator
    return OracleOperator(cfg)


def _push_of(rng, keys, ts):
    """(keys, ts, [int column, double column as bits]) of one push"""
    n = len(keys)
    iv = rng.integers(-1000, 1000, n).astype(np.int64)
    dv = (rng.random(n) * 1000.0).view(np.int64)
    return np.asarray(keys, np.int64), np.asarray(ts, np.int64), [iv, dv]


def _keys(n, base=0):
    return (np.arange(n, dtype=np.int64) + base) * 7919 - 50000


def _capacity_error(fn):
    with pytest.raises(FlinkWinError) as e:
        fn()
    assert e.value.code == abi.FW_E_CAPACITY, e.value


def _overflowed(g, bit, failing):
    """part (a): exactly `bit`, stats keeps working, every call in `failing` raises FW_E_CAPACITY"""
    st = g.stats()
    assert st["error_flags"] == bit, st
    for fn in failing:
        _capacity_error(fn)
    assert g.stats()["error_flags"] == bit
    return st


def _subset_without_duplicates(got, want, ctx):
    """part (b): every row is an oracle row, and no (key, window_end) appears twice"""
    want = set(want)
    assert len({(r[0], r[2]) for r in got}) == len(got), f"{ctx}: a (key, window_end) appears twice"
    for r in got:
        assert r in want, f"{ctx}: {r} is not an oracle row"


class _Ref:
    """The oracle's run of one case, made before any handle exists: rows per watermark of the warm-up
    and of the recovery, in the order the test replays them."""

    def __init__(self, cfg, dc):
        self.cfg, self.dc, self.o = cfg, dc, _oracle(cfg)
        self.rows = []

    def push(self, p):
        self.o.process_batch(*p)

    def advance(self, wm):
        self.o.process_watermark(wm)
        self.rows.append(_rows(self.o.results(clear=True), self.cfg, self.dc))
        return self.rows[-1]

    def take(self):
        """rows emitted without a watermark (DataStream late fires)"""
        self.rows.append(_rows(self.o.results(clear=True), self.cfg, self.dc))
        return self.rows[-1]


class _Replay:
    """The handle's side of a _Ref: the same calls, each compared with the reference's rows."""

    def __init__(self, g, ref):
        self.g, self.ref, self.i = g, ref, 0

    def check(self, res, ctx):
        _compare(_rows(res, self.ref.cfg, self.ref.dc), self.ref.rows[self.i], self.ref.dc, ctx)
        self.i += 1

    def advance(self, wm, ctx):
        self.g.advance(wm)
        self.check(self.g.results(reset=True), ctx)

    def done(self):
        assert self.i == len(self.ref.rows)
        st = self.g.stats()
        assert st["error_flags"] == 0, st
        assert st["num_late_records_dropped"] == self.ref.o.late_dropped
        return st


def _restore_same_handle(g, blob):
    g.restore(blob)
    assert g.stats()["error_flags"] == 0


# ---- 1. OUTPUT, slabs and overflow region exhausted ---------------------------------------------
def _tumble_windows(rng, n_win, n_keys, first=1, size=10_000):
    """one push per window: n_keys distinct keys, all on time"""
    return [_push_of(rng, _keys(n_keys, 100_000 * w), T0 + w * size + rng.integers(0, size, n_keys))
            for w in range(first, first + n_win)]


def test_output_capacity_region_exhausted():
    kw = CASES["sql_tumble_int_aggs"]
    cfg = _cfg(kw, output_capacity=OUT_CAP, max_batch_rows=MBR)
    rng = np.random.default_rng(1)
    warm = _push_of(rng, _keys(1000), T0 + rng.integers(0, 10_000, 1000))
    wins = _tumble_windows(rng, 5, 4000)
    ref = _Ref(cfg, set())
    ref.push(warm)
    ref.advance(T0 + 9_999)
    ref.o.snapshot_restore()
    per_win = []
    for w, p in enumerate(wins):
        ref.push(p)
        per_win.append(ref.advance(T0 + (w + 2) * 10_000 - 1))
    all_rows = [r for rows in per_win for r in rows]
    n_sb, slab = 128, 64   # (2 * 4096 + 127) / 128 = 64 rows per slab
    assert all(len(r) == 4000 for r in per_win) and 4000 <= OUT_CAP
    assert len(all_rows) == 20_000 > n_sb * slab + OUT_CAP

    def overflow(g):
        g.push_host(*warm)
        g.advance(T0 + 9_999)
        rp = _Replay(g, ref)
        rp.check(g.results(reset=True), "warm-up")
        blob = g.snapshot()
        for p in wins:
            g.push_host(*p)
        g.advance(T0 + 6 * 10_000 - 1)
        return rp, blob

    # (a) + (c)
    g = _handle(cfg)
    try:
        assert g.stats()["num_superbuckets"] == n_sb
        rp, blob = overflow(g)
        _overflowed(g, ERRF["OUTPUT"], [g.results, g.snapshot])
        _restore_same_handle(g, blob)
        for w, p in enumerate(wins):
            g.push_host(*p)
            rp.advance(T0 + (w + 2) * 10_000 - 1, f"recovery window {w}")
        rp.done()
    finally:
        g.close()
    # (b) the segments do not go through the control block's error: the rows that fit are delivered
    from flink_amd.runtime.handle import _np_view
    g = _handle(cfg)
    try:
        overflow(g)
        seg = g.result_segments()
        res = g.segments_to_host(seg)  # (synchronises)
        counts = _np_view(seg.counts, int(seg.n_segments), np.int32).copy()
        assert int(seg.n_segments) == n_sb + 1 and int(seg.seg_cap) == slab
        assert counts[-1] == OUT_CAP, counts[-1]
        assert (counts[:-1] <= slab).all() and (counts >= 0).all()
        got = _rows(res, cfg, set())
        assert len(got) == int(counts.sum())
        _subset_without_duplicates(got, all_rows, "segments")
        assert g.stats()["error_flags"] == ERRF["OUTPUT"]
    finally:
        g.close()


# ---- 2. OUTPUT, the slabs absorb what the result columns cannot hold -----------------------------
def _one_window_6000(cfg, dc):
    """6000 distinct keys in one window; the recovery feeds the same keys as two windows of 3000 (one
    firing emits all rows of its window: 6000 rows of one window never fit 4096)"""
    rng = np.random.default_rng(2)
    k = _keys(6000)
    big = _push_of(rng, k, T0 + 10_000 + rng.integers(0, 10_000, 6000))
    halves = [(big[0][h::2], big[1][h::2] + h * 10_000, [v[h::2] for v in big[2]]) for h in (0, 1)]
    ref = _Ref(cfg, dc)
    ref.push(big)
    rows = ref.advance(T0 + 19_999)
    assert OUT_CAP < len(rows) == 6000 <= 128 * 64 + OUT_CAP  # no firing-time error: slabs + region hold them
    ref2 = _Ref(cfg, dc)
    for h in (0, 1):
        ref2.push(halves[h])
        assert len(ref2.advance(T0 + (2 + h) * 10_000 - 1)) == 3000 <= OUT_CAP
    return big, halves, rows, ref2


def test_output_capacity_at_the_collection_results():
    """fw_results: FW_E_CAPACITY, the bit, and recovery."""
    cfg = _cfg(CASES["sql_tumble_int_aggs"], output_capacity=OUT_CAP, max_batch_rows=MBR)
    big, halves, _, ref2 = _one_window_6000(cfg, set())
    g = _handle(cfg)
    try:
        blob = g.snapshot()
        g.push_host(*big)
        g.advance(T0 + 19_999)
        assert g.stats()["error_flags"] == 0  # the firing itself fits slabs + region
        _capacity_error(g.results)
        _overflowed(g, ERRF["OUTPUT"], [g.results, g.snapshot])
        _restore_same_handle(g, blob)
        rp = _Replay(g, ref2)
        for h in (0, 1):
            g.push_host(*halves[h])
            rp.advance(T0 + (2 + h) * 10_000 - 1, f"recovery half {h}")
        rp.done()
    finally:
        g.close()


def test_output_capacity_at_the_collection_results_async():
    """fw_results_async + fw_results_ready: FW_E_CAPACITY."""
    cfg = _cfg(CASES["sql_tumble_int_aggs"], output_capacity=OUT_CAP, max_batch_rows=MBR)
    big, _, _, _ = _one_window_6000(cfg, set())
    g = _handle(cfg)
    try:
        g.push_host(*big)
        g.advance(T0 + 19_999)
        g.results_async()
        _capacity_error(g.results_ready)
        assert g.stats()["error_flags"] == ERRF["OUTPUT"]
    finally:
        g.close()


@pytest.mark.parametrize("phase", ["one", "local"])
def test_output_capacity_at_the_collection_results_device(phase):
    """fw_results_device does not wait and cannot fail: *d_n is the number of rows it copied, and the
    bit tells that rows were dropped.  "local": emit_partial of the LOCAL phase, the collection the
    two-phase device step uses."""
    import torch
    extra = dict(agg_phase=abi.PHASE_LOCAL) if phase == "local" else {}
    cfg = _cfg(CASES["sql_tumble_int_aggs"], output_capacity=OUT_CAP, max_batch_rows=MBR, **extra)
    big, _, rows, _ = _one_window_6000(cfg, set())
    g = _handle(cfg)
    try:
        g.push_host(*big)
        g.advance(T0 + 19_999)
        dev = torch.device("cuda", 0)
        n, key, ws, we, vals, nm = g.device_results_async(dev)
        n = int(n)  # (synchronises the caller's stream, which waits for the collection)
        assert 0 < n <= OUT_CAP, n
        res = {"key": key[:n].cpu().numpy(), "window_start": ws[:n].cpu().numpy(), "window_end": we[:n].cpu().numpy(),
               "values": [v[:n].cpu().numpy() for v in vals], "null_mask": nm[:n].cpu().numpy()}
        _subset_without_duplicates(_rows(res, cfg, set()), rows, f"fw_results_device {phase}")
        _capacity_error(g.sync)  # fw_sync reads the control block: the bit fails it
        assert g.stats()["error_flags"] == ERRF["OUTPUT"]
    finally:
        g.close()


# ---- 3. TREQ --------------------------------------------------------------------------------------
# (start of the on-time rows, W + 1, [lo, hi) of the late timestamps).  W + 1 is a window end; the late
# rows' slices have fired at W and a later window of theirs has not.
def _treq_times(name):
    kw = CASES[name]
    size, slide, off = kw["size_ms"], kw["slide_ms"], kw.get("offset_ms", 0)
    if kw["window_kind"] == abi.WIN_HOP:
        end = T0 - (T0 - off) % slide + slide + 2 * size  # a slice boundary + 2 sizes
        start = end - size
        lo, hi = (6000, 2000) if size >= 4 * slide else (slide, 0)  # 10 s / 2 s: 2-6 s below W + 1
    else:  # CUMULATE: the window of 4 steps of the cycle that starts at `start`
        start = T0 - (T0 - off) % size + size
        end = start + 4 * slide
        lo, hi = 6000, 2000
    return start, end, end - lo, end - hi


HB_R = 8  # slices per HOP block entry (fw_internal.h)


def _treq_entries_per_key(kw, ts, block_state):
    """The state entries one key can hold for rows at the timestamps `ts`, from the window alone: one
    per distinct slice end the rows map to (a late CUMULATE row: its cycle's first slice, the merge
    target) plus one per window end that holds one of these slices (the windows' timers).  With HOP block
    state an entry is a block of HB_R slices and the timers are arithmetic: the distinct blocks."""
    size, slide, off = kw["size_ms"], kw["slide_ms"], kw.get("offset_ms", 0)
    se = np.unique(ts - (ts - off) % slide + slide)
    if block_state:
        return len(np.unique((se - 1) - (se - 1 - off) % (HB_R * slide)))
    if kw["window_kind"] == abi.WIN_HOP:
        slices = set(se.tolist())
        timers = {int(e) + k * slide for e in se for k in range(size // slide)}
    else:
        cyc = (se - 1) - (se - 1 - off) % size  # the cycle's start
        slices = set(se.tolist()) | set((cyc + slide).tolist())
        timers = {e for e0, c in zip(se.tolist(), cyc.tolist()) for e in range(e0, c + size + 1, slide)}
    return len(slices) + len(timers)


@pytest.mark.parametrize("name,runs,per_key", [("sql_hop", "0", 5 + 9), ("sql_hop", "1", 5 + 9),
                                               ("sql_cumulate_countstar", None, 4 + 6), ("sql_hop_offset", None, 1)])
def test_timer_request_capacity(name, runs, per_key, monkeypatch):
    """sql_hop_offset (two accumulator words: HOP block state, k_merge_hopb) is beyond the issue's list.
    per_key: what _treq_entries_per_key must give for the case (slices + timers, or blocks)."""
    if runs is not None:
        monkeypatch.setenv("FW_RUNS", runs)
    kw = CASES[name]
    cfg, dc = _cfg(kw, max_batch_rows=MBR), _double_cols(kw)
    start, end, lo, hi = _treq_times(name)
    W, slide = end - 1, kw["slide_ms"]
    rng = np.random.default_rng(3)
    warm = _push_of(rng, _keys(64)[rng.integers(0, 64, MBR)], rng.integers(start, end, MBR))
    late = [_push_of(rng, _keys(64)[rng.integers(0, 64, MBR)], rng.integers(lo, hi, MBR)) for _ in range(N_OVER)]
    ref = _Ref(cfg, dc)
    ref.push(warm)
    assert len(ref.advance(W)) > 0
    ref.o.snapshot_restore()
    dropped = ref.o.late_dropped
    for p in late:
        ref.push(p)
    assert ref.o.late_dropped == dropped      # every late row merges: one timer request each
    assert N_OVER * MBR > CAP >= MBR
    assert len(ref.advance(W + slide)) > 0
    pushed = np.concatenate([warm[1]] + [p[1] for p in late])
    assert _treq_entries_per_key(kw, pushed, name == "sql_hop_offset") == per_key

    g = _handle(cfg)
    try:
        rp = _Replay(g, ref)
        g.push_host(*warm)
        rp.advance(W, "warm-up")
        blob = g.snapshot()
        before = g.stats()
        for p in late:
            g.push_host(*p)
        # what a stray request triple would break: an entry under a key or a window end nobody pushed.
        # Checked when the merge has read the requests (the flush) and again after the firing, which
        # may leave nothing live (sql_hop_offset: W + slide fires the last window of every slice).
        g.flush()
        assert 0 < g.stats()["live_state_entries"] <= 64 * per_key, (g.stats()["live_state_entries"], per_key)
        g.advance(W + slide)
        st = _overflowed(g, ERRF["TREQ"], [g.results, g.snapshot])
        assert st["num_late_records_dropped"] == before["num_late_records_dropped"]
        assert st["live_state_entries"] <= 64 * per_key, (st["live_state_entries"], per_key)
        _restore_same_handle(g, blob)
        for p in late:
            g.push_host(*p)
            g.flush()
        rp.advance(W + slide, "recovery")
        rp.done()
    finally:
        g.close()


# ---- 4. LATE, late-fire rows -------------------------------------------------------------------------
def test_late_fire_row_capacity():
    kw = CASES["ds_tumble_lateness"]  # 4 s windows, 3 s lateness
    cfg = _cfg(kw, max_batch_rows=MBR, output_capacity=1 << 18)
    rng = np.random.default_rng(4)
    nk = 1000
    warm = _push_of(rng, _keys(nk)[rng.integers(0, nk, MBR)], T0 + rng.integers(0, 4000, MBR))
    late = [_push_of(rng, _keys(nk)[rng.integers(0, nk, MBR)], T0 + rng.integers(0, 4000, MBR)) for _ in range(N_OVER)]
    W = T0 + 4000  # the window has fired; it is cleaned at T0 + 3999 + 3000
    ref = _Ref(cfg, set())
    ref.push(warm)
    assert len(ref.advance(W)) == nk
    ref.o.snapshot_restore()
    assert len(ref.advance(W)) == 0  # a restored WindowOperator's timer service starts at Long.MIN_VALUE again
    for p in late:
        ref.push(p)
        assert len(ref.take()) == MBR  # every late element fires its window again
    assert N_OVER * MBR > CAP >= MBR and N_OVER * MBR <= 1 << 18
    ref.advance(W + 500)

    g = _handle(cfg)
    try:
        rp = _Replay(g, ref)
        g.push_host(*warm)
        rp.advance(W, "warm-up")
        blob = g.snapshot()
        for p in late:
            g.push_host(*p)
        g.advance(W + 500)  # the merge walks the late-fire rows it has
        _overflowed(g, ERRF["LATE"], [g.results, g.snapshot])
        _restore_same_handle(g, blob)
        rp.advance(W, "the watermark again")
        for i, p in enumerate(late):
            g.push_host(*p)
            g.flush()
            rp.check(g.results(reset=True), f"recovery push {i}")
        rp.advance(W + 500, "recovery")
        rp.done()
    finally:
        g.close()


# ---- 5. LATE, side output ----------------------------------------------------------------------------
def _side_rows(d, used):
    return sorted(zip(d["key"].tolist(), d["ts"].tolist(), *[d["values"][c].tolist() for c in used]))


def test_late_side_output_capacity():
    kw = CASES["ds_sliding_side_output"]  # 4 s / 1 s, no lateness
    cfg = _cfg(kw, max_batch_rows=MBR)
    used = sorted({cfg.aggs[a].input_col for a in range(cfg.n_aggs) if cfg.aggs[a].kind != abi.AGG_COUNT_STAR})
    rng = np.random.default_rng(5)
    nk = 500
    W = T0 + 10_000
    warm = _push_of(rng, _keys(nk)[rng.integers(0, nk, MBR)], T0 + 6000 + rng.integers(0, 4000, MBR))
    late = [_push_of(rng, _keys(nk)[rng.integers(0, nk, MBR)], T0 + rng.integers(0, 3000, MBR)) for _ in range(N_OVER)]
    ref = _Ref(cfg, set())
    ref.push(warm)
    assert len(ref.advance(W)) > 0
    assert len(ref.o.side_output()["key"]) == 0
    ref.o.snapshot_restore()
    assert len(ref.advance(W)) == 0  # (the restored timer service starts at Long.MIN_VALUE again)
    want_side = []
    for p in late:
        ref.push(p)
        want_side.append(_side_rows(ref.o.side_output(), used))
        assert len(want_side[-1]) == MBR  # wholly behind the watermark
    assert N_OVER * MBR > CAP >= MBR
    ref.advance(W + 1000)

    g = _handle(cfg)
    try:
        rp = _Replay(g, ref)
        g.push_host(*warm)
        rp.advance(W, "warm-up")
        assert len(g.late_records()["key"]) == 0
        blob = g.snapshot()
        for p in late:
            g.push_host(*p)
        _overflowed(g, ERRF["LATE"], [g.late_records, g.results, g.snapshot])
        _restore_same_handle(g, blob)
        rp.advance(W, "the watermark again")
        for i, p in enumerate(late):
            g.push_host(*p)
            assert _side_rows(g.late_records(), used) == want_side[i], f"recovery push {i}: late side output differs"
        rp.advance(W + 1000, "recovery")
        rp.done()
    finally:
        g.close()


# ---- 6. ORDEV -----------------------------------------------------------------------------------------
def test_first_element_event_capacity():
    mbr, scap, size = 1 << 12, 1 << 12, 4000
    kw = dict(api=abi.API_DATASTREAM, window_kind=abi.WIN_TUMBLE, size_ms=size, aggs=[(abi.AGG_SUM, 0, I64)])
    cfg = _cfg(kw, ds_first_ordinals=True, max_batch_rows=mbr, state_capacity=scap)
    # fw_api.hip:781-782: ordev_cap = (FW_MAX_PENDING * cap_rows + state_capacity) * n_win + 65536, with
    # cap_rows = max_batch_rows rounded up to ingest chunks of 4096 rows and one window per element
    ordev_cap = (8 * mbr + scap) * 1 + (1 << 16)
    n_steps = ordev_cap // (2 * mbr) + 1  # every step leaves 4096 retains and 4096 releases
    rng = np.random.default_rng(6)
    pushes = [_push_of(rng, np.arange(mbr, dtype=np.int64) + s * mbr, T0 + s * size + rng.integers(0, size, mbr))
              for s in range(n_steps + 1)]
    wm = lambda s: T0 + s * size - 1   # fires window s - 1
    ref = _Ref(cfg, set())
    first = []  # first-element ordinals of the rows each advance fires
    for s, p in enumerate(pushes):
        ref.push(p)
        if s == 0:
            ref.advance(wm(0))
            ref.o.snapshot_restore()
            first.append([])
            continue
        ref.o.process_watermark(wm(s))
        res = ref.o.results(clear=True)
        first.append(sorted(res["first_ord"].tolist()))
        ref.rows.append(_rows(res, cfg, set()))
        assert len(first[-1]) == mbr
    ref.o.process_watermark(wm(len(pushes)))
    res = ref.o.results(clear=True)
    first.append(sorted(res["first_ord"].tolist()))
    ref.rows.append(_rows(res, cfg, set()))
    assert 2 * mbr * n_steps > ordev_cap >= 4 * mbr and n_steps == 13

    g = _handle(cfg)
    try:
        rp = _Replay(g, ref)
        seq = {}  # the handle's push number -> the oracle's (the handle keeps counting through a restore)
        seq[g.push_seq] = 0
        g.push_host(*pushes[0])
        rp.advance(wm(0), "warm-up")
        retain, release = g.first_element_events()
        assert len(release) == 0
        warm_retain = sorted(retain.tolist())
        blob = g.snapshot()
        for s in range(1, n_steps + 1):
            g.push_host(*pushes[s])
            g.advance(wm(s))
        _overflowed(g, ERRF["ORDEV"], [g.first_element_events, g.results, g.snapshot])
        _restore_same_handle(g, blob)
        norm = lambda a: sorted(((seq[x >> 32] << 32) | (x & 0xffffffff)) for x in a.tolist())
        got_retain, got_release = [warm_retain], [[]]
        for s in range(1, len(pushes)):
            seq[g.push_seq] = s
            g.push_host(*pushes[s])
            g.advance(wm(s))
            res = g.results(reset=True)
            assert norm(res["first_ord"]) == first[s], f"recovery step {s}: first elements of the fired rows"
            rp.check(res, f"recovery step {s}")
            retain, release = g.first_element_events()
            got_retain.append(norm(retain))
            got_release.append(norm(release))
        g.advance(wm(len(pushes)))
        res = g.results(reset=True)
        rp.check(res, "last window")
        retain, release = g.first_element_events()
        assert len(retain) == 0
        got_release.append(norm(release))
        # a window's first element is retained at the flush that creates its state and released when the
        # window is cleaned, which for these windows (no lateness) is the advance that fires it
        for s in range(len(pushes)):
            assert got_retain[s] == first[s + 1], f"retains of step {s}"
            assert got_release[s + 1] == first[s + 1], f"releases of step {s + 1}"
        st = rp.done()
        assert st["live_state_entries"] == 0
    finally:
        g.close()


# ---- 7. STATE on HOP and CUMULATE ---------------------------------------------------------------------
TWO = dict(max_parallelism=2, state_capacity=1024)  # two superbuckets (test_gpu_merge_tag.py's recipe)


@pytest.mark.parametrize("name", ["sql_hop", "sql_cumulate_countstar", "sql_hop_offset"])
def test_state_capacity_hop_and_cumulate(name):
    """sql_hop_offset (HOP block state, k_merge_hopb's own site) is beyond the issue's list."""
    kw = CASES[name]
    cfg, dc = _cfg(kw, max_batch_rows=MBR, **TWO), _double_cols(kw)
    slide = kw["slide_ms"]
    rng = np.random.default_rng(7)
    # Step 0 brings all 500 keys, step b > 0 the keys with key index % 4 == b % 4: over four steps all 500
    # again, each with data in at most two live slices.  With its window timer that is three entries per
    # key, 750 of a superbucket's 250 keys against the smallest table here (sql_hop: 8 words, 1024 entries).
    def small(b):
        pool = _keys(500) if b == 0 else _keys(500)[b % 4::4]
        return _push_of(rng, pool[rng.integers(0, len(pool), 4000)], T0 + b * slide + rng.integers(0, slide, 4000))
    steps = [small(b) for b in range(8)]
    big = _push_of(rng, _keys(8000, 1000)[rng.integers(0, 8000, MBR)], T0 + slide + rng.integers(0, 2 * slide, MBR))
    ref = _Ref(cfg, dc)
    ref.push(steps[0])
    ref.advance(T0 + slide - 1)
    assert ref.o.state_size >= 500  # 500 keys are live at the snapshot
    ref.o.snapshot_restore()
    for b in range(1, 8):
        ref.push(steps[b])
        ref.advance(T0 + (b + 1) * slide - 1)
    assert sum(len(r) for r in ref.rows) > 0
    # distinct (key, slice) pairs against two tables of at most 4096 entries
    assert len(set(zip(big[0].tolist(), (big[1] // slide).tolist()))) > 2 * 4096 + 1000

    g = _handle(cfg)
    try:
        rp = _Replay(g, ref)
        g.push_host(*steps[0])
        rp.advance(T0 + slide - 1, "warm-up")
        blob = g.snapshot()
        g.push_host(*big)
        g.advance(T0 + 2 * slide - 1)
        st = _overflowed(g, ERRF["STATE"], [g.results, g.snapshot])
        assert st["num_superbuckets"] == 2
        assert st["live_state_entries"] <= st["num_superbuckets"] * st["superbucket_capacity"], st
        assert st["peak_superbucket_entries"] > st["superbucket_capacity"], st
        _restore_same_handle(g, blob)
        for b in range(1, 8):
            g.push_host(*steps[b])
            rp.advance(T0 + (b + 1) * slide - 1, f"recovery step {b}")
        rp.done()
    finally:
        g.close()


# ---- 8. KEYROW ----------------------------------------------------------------------------------------
KR_MAX = 32
KR_KW = dict(window_kind=abi.WIN_TUMBLE, size_ms=2000, count_star_index=0,
             aggs=[(abi.AGG_COUNT_STAR, 0, I64), (abi.AGG_MAX, 0, I64)])


def _kr_images(ids, long_at=None):
    """BinaryRowData images of one-field BIGINT key rows (8 B null bits + header, 8 B field); the row at
    long_at is 8 bytes longer than key_row_max_bytes"""
    off, img = [0], []
    for i, k in enumerate(ids):
        row = bytes(8) + int(k).to_bytes(8, "little", signed=True)
        if i == long_at:
            row += bytes(KR_MAX + 8 - len(row))
        img.append(row)
        off.append(off[-1] + len(row))
    return np.array(off, np.int64), np.frombuffer(b"".join(img), np.uint8)


class _KeyRowReplay(_Replay):
    def check(self, res, ctx):
        res = dict(res)
        res["key"] = np.array([int.from_bytes(b[8:16], "little", signed=True) for b in res["key_rows"]], np.int64)
        assert all(len(b) == 16 for b in res["key_rows"])
        super().check(res, ctx)


def _kr_push(g, p, long_at=None):
    off, img = _kr_images(p[0], long_at)
    g.push_host_key_rows(off, img, p[1], p[2])


def _kr_cfgs(mbr):
    cfg = _cfg(KR_KW, key_hash=abi.KEYHASH_KEYROW, key_row_max_bytes=KR_MAX, state_capacity=1024, max_batch_rows=mbr,
               output_capacity=1 << 14)
    return cfg, _cfg(KR_KW, key_hash=abi.KEYHASH_PRECOMPUTED, state_capacity=1024, max_batch_rows=mbr, output_capacity=1 << 14)


def test_key_row_over_the_length_limit():
    cfg, ocfg = _kr_cfgs(256)
    rng = np.random.default_rng(8)
    warm = _push_of(rng, np.arange(100, dtype=np.int64) + 10_000, T0 + 20_000 + rng.integers(0, 2000, 100))  # stays live
    push = _push_of(rng, np.arange(100, dtype=np.int64), T0 + rng.integers(0, 2000, 100))
    ref = _Ref(ocfg, set())
    ref.push(warm)
    assert len(ref.advance(T0 - 1)) == 0
    ref.o.snapshot_restore()
    ref.push(push)
    assert len(ref.advance(T0 + 1999)) == 100
    assert len(ref.advance(T0 + 21_999)) == 100

    g = _handle(cfg)
    try:
        rp = _KeyRowReplay(g, ref)
        _kr_push(g, warm)
        rp.advance(T0 - 1, "warm-up")
        blob = g.snapshot()
        longer = (np.append(push[0], 777), np.append(push[1], T0 + 5), [np.append(v, 1) for v in push[2]])
        _kr_push(g, longer, long_at=100)
        _overflowed(g, ERRF["KEYROW"], [g.results, g.snapshot])
        # a blob that fails its check changes nothing: the table, the state and the error bit stay
        with pytest.raises(FlinkWinError) as bad:
            g.restore(blob[:-8])  # the last key row's image is cut short
        assert bad.value.code == abi.FW_E_INVALID
        st = g.stats()
        assert st["error_flags"] == ERRF["KEYROW"] and st["key_rows"] >= 200, st
        _restore_same_handle(g, blob)
        assert g.stats()["key_rows"] == 100  # the table was restarted with the blob's key rows
        _kr_push(g, push)
        rp.advance(T0 + 1999, "recovery")
        rp.advance(T0 + 21_999, "recovery, the window of the snapshot")
        rp.done()
    finally:
        g.close()


def test_key_row_table_full():
    """cap_ids + more distinct live key rows: the state tables (128 superbuckets of 2048 entries) hold
    them easily, so FW_ERRF_STATE stays clear and KEYROW is the only bit.  The advance that fires them
    runs the collection with the id counter past cap_ids."""
    mbr = 256
    cfg, ocfg = _kr_cfgs(mbr)
    cap_ids = max(1024, 1024 + 8 * mbr)  # fw_api.hip:789: max(1024, state_capacity + FW_MAX_PENDING * max_batch_rows)
    rng = np.random.default_rng(9)
    warm = _push_of(rng, np.arange(100, dtype=np.int64) + 100_000, T0 + 20_000 + rng.integers(0, 2000, 100))
    wins = [_push_of(rng, np.arange(1100, dtype=np.int64) + 2000 * w, T0 + 2000 * w + rng.integers(0, 2000, 1100))
            for w in range(3)]
    ref = _Ref(ocfg, set())
    ref.push(warm)
    assert len(ref.advance(T0 - 1)) == 0
    ref.o.snapshot_restore()
    for w, p in enumerate(wins):
        ref.push(p)
        assert len(ref.advance(T0 + 2000 * (w + 1) - 1)) == 1100
    assert len(ref.advance(T0 + 21_999)) == 100
    # all at once they do not fit the table; window by window they do, but only with collections
    assert 100 + 3 * 1100 > cap_ids > 100 + 2 * 1100 and 100 + 3 * 1100 <= 1 << 14

    g = _handle(cfg)
    try:
        rp = _KeyRowReplay(g, ref)
        _kr_push(g, warm)
        rp.advance(T0 - 1, "warm-up")
        blob = g.snapshot()
        for p in wins:
            _kr_push(g, p)
        g.advance(T0 + 5999)
        st = _overflowed(g, ERRF["KEYROW"], [g.results, g.snapshot])
        assert 0 < st["key_rows"] <= cap_ids, st
        _restore_same_handle(g, blob)
        for w, p in enumerate(wins):
            _kr_push(g, p)
            rp.advance(T0 + 2000 * (w + 1) - 1, f"recovery window {w}")
            assert g.stats()["key_rows"] <= cap_ids
        rp.advance(T0 + 21_999, "recovery, the window of the snapshot")
        st = rp.done()
        assert st["key_row_collections"] > 0, st
    finally:
        g.close()


# ---- 9. restore with uncollected rows ------------------------------------------------------------------
@pytest.mark.parametrize("how", ["snapshot", "key_groups"])
def test_restore_drops_uncollected_rows(how):
    """The reference restores into a fresh operator, where nothing emitted and unread survives."""
    cfg = _cfg(CASES["sql_tumble_int_aggs"], output_capacity=OUT_CAP, max_batch_rows=MBR)
    rng = np.random.default_rng(10)
    first = _push_of(rng, _keys(6000), T0 + rng.integers(0, 10_000, 6000))
    second = _push_of(rng, _keys(3000, 3000), T0 + 10_000 + rng.integers(0, 10_000, 3000))
    o = _oracle(cfg)
    o.process_batch(*first)
    o.process_watermark(T0 + 9_999)
    assert len(o.results(clear=True)["key"]) == 6000  # some slabs of 64 overflow into the region
    o.snapshot_restore()
    ref = _Ref(cfg, set())
    ref.o = o
    ref.push(second)
    assert len(ref.advance(T0 + 19_999)) == 3000 <= OUT_CAP

    g = _handle(cfg)
    try:
        g.push_host(*first)
        g.advance(T0 + 9_999)
        assert g.stats()["results_available"] == 6000
        if how == "snapshot":
            g.restore(g.snapshot())
        else:
            blobs, wm = g.snapshot_key_groups()
            g.restore_key_groups(blobs, [wm])
        assert g.stats()["results_available"] == 0
        assert len(g.results(reset=True)["key"]) == 0, "rows of before the restore came out after it"
        rp = _Replay(g, ref)
        g.push_host(*second)
        rp.advance(T0 + 19_999, "the second window")
        rp.done()
    finally:
        g.close()
