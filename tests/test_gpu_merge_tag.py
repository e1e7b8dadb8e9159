"""GPU parity of the merge kernel's tag path (fw_merge_impl.h, GF_TAG).

SQL TUMBLE handles with one NOT NULL integer MAX / MIN / SUM buffer PF_PACK run rows.  A flush whose
pending pushes are all PF_PACK, whose key and rank fields fit 31 bits and whose live state converts is
merged through a tag-addressed LDS table, superbucket by superbucket; everything else keeps the entry
table in the same launch.  Every case runs with FW_MG_TAG=1 and FW_MG_TAG=0 in fresh operators: each
watermark's rows are bit-exact against the oracle in both, and the late / partial / fired / live
counters agree between the two.  fw_merge_path_superbuckets tells which path served the superbuckets.

Pushes are 3 chunks + 5 rows, 3 pushes per watermark, 6 watermarks, max_batch_rows = 1 << 14.  Keys come
from a pool that spans 19 bits, so the key and rank fields take 20 + 8 bits.

Superbuckets.  A chunk's rows of one superbucket go to a sub-run of 5/4 of a uniform share + 16 rows
(rounded up to 16), and a push of four chunks uses four of a superbucket's eight sub-runs, one chunk each.
With the 128 superbuckets of the common test capacity a chunk brings 32 +- 6 rows against 48, so now and
then a superbucket sees an overflow flag and keeps the entry table; the cases that assert the path of
every superbucket run 1024 (state_capacity = 2 000 000: 4 rows against 32).  With one or two superbuckets
a 4096-row chunk always overruns its sub-run (2048 rows against 1296), and so does any chunk with a hot
key: under the module's pushes the crowded table and the hot key are served by the entry table, so
those two cases also run with one push of at most 2500 rows per chunk, which the tag path serves."""
import numpy as np
import pytest

from flink_amd import _native, abi
from parity_common import I64, _cfg, _compare, _rows, _run_both

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000_000
CH = 4096
PUSH = 3 * CH + 5          # rows per push
SPLIT = 3                  # pushes per watermark
N_WM = 6
SIZE = 5000                # TUMBLE size = slice (ms): every watermark fires a window and flushes
LONG = 15000               # TUMBLE size of three watermark steps: state lives across flushes
STEP, OOO = 5000, 4000
BIG = dict(state_capacity=2_000_000)   # 1024 superbuckets (module docstring)
POOL = np.arange(40000, dtype=np.int64) * 7 + 11

AGGS = {
    "max": [(abi.AGG_MAX, 0, I64)],
    "min": [(abi.AGG_MIN, 0, I64)],
    "sum": [(abi.AGG_SUM, 0, I64)],
}
COUNTERS = ("num_late_records_dropped", "partials_emitted", "num_fired_windows", "live_state_entries")


def _kw(name, size=SIZE):
    return dict(window_kind=abi.WIN_TUMBLE, size_ms=size, aggs=AGGS[name])


def _stream(seed, pool=POOL, n_wm=N_WM, push=PUSH, vbase=0):
    """On-time batches of SPLIT pushes; keys distinct within a push when the pool allows it."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_wm):
        base = T0 + b * STEP
        n = SPLIT * push
        ts = base + rng.integers(0, STEP, n) - rng.integers(0, OOO, n)
        if len(pool) >= n:
            keys = rng.permutation(pool)[:n]
        elif len(pool) >= push:
            keys = np.concatenate([rng.permutation(pool)[:push] for _ in range(SPLIT)])
        else:
            keys = pool[rng.integers(0, len(pool), n)]
        iv = (vbase + rng.integers(-10**6, 10**6, n)).astype(np.int64)
        out.append((keys.astype(np.int64), ts.astype(np.int64), iv, np.zeros(n), base + STEP - OOO - 1))
    return out


def _paths():
    """(entry-table path, tag path) superbuckets of the handles destroyed so far."""
    L = _native.lib()
    return int(L.fw_merge_path_superbuckets(None, 0)), int(L.fw_merge_path_superbuckets(None, 1))


def _both_modes(monkeypatch, kw, batches, cfg_extra=None, snapshot_at=None):
    """{mode: (stats, entry-table superbuckets, tag superbuckets)} of FW_MG_TAG=1 and =0 through
    parity_common._run_both (every watermark's rows against the oracle)."""
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FW_MG_TAG", mode)
        st, (o0, t0) = {}, _paths()
        _run_both(_cfg(kw, max_batch_rows=1 << 14, **(cfg_extra or {})), batches, set(), split=SPLIT, stats=st,
                  snapshot_at=snapshot_at)
        o1, t1 = _paths()  # (_run_both's handle went with its frame)
        out[mode] = (st, o1 - o0, t1 - t0)
    for c in COUNTERS:
        assert out["1"][0][c] == out["0"][0][c], (c, out["1"][0], out["0"][0])
    assert out["0"][1:] == (0, 0), out["0"][1:]  # FW_MG_TAG=0 launches the plain variant: nothing counted
    return out


def _run_steps(cfg, batches, expect_error=0):
    """parity_common._run_both's loop with the path counters after every watermark: returns the
    final stats and per watermark the (entry-table, tag) superbuckets of its launches.  expect_error:
    rows are not compared, and the error bit must be raised."""
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    o, g = OracleOperator(cfg), WindowAggHandle(cfg)
    per_wm, last = [], (0, 0)
    try:
        for bi, (k, t, iv, dv, wm) in enumerate(batches):
            vals = [iv, dv.view(np.int64)]
            if not expect_error:
                o.process_batch(k, t, vals, None)
                o.process_watermark(wm)
            try:
                for part in np.array_split(np.arange(len(k)), SPLIT):
                    g.push_host(k[part], t[part], [v[part] for v in vals])
                g.advance(wm)
                got = g.results(reset=True)
            except _native.FlinkWinError:
                assert expect_error
                break
            if not expect_error:
                _compare(_rows(got, cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"batch {bi}")
            now = g.merge_path_superbuckets()
            per_wm.append((now[0] - last[0], now[1] - last[1]))
            last = now
        st = g.stats()
        if expect_error:
            assert st["error_flags"] & expect_error, st
        else:
            assert st["num_late_records_dropped"] == o.late_dropped and st["error_flags"] == 0
    finally:
        g.close()
    return st, per_wm


def _steps_both_modes(monkeypatch, kw, batches, cfg_extra=None):
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FW_MG_TAG", mode)
        out[mode] = _run_steps(_cfg(kw, max_batch_rows=1 << 14, **(cfg_extra or {})), batches)
    for c in COUNTERS:
        assert out["1"][0][c] == out["0"][0][c], (c, out["1"][0], out["0"][0])
    assert all(p == (0, 0) for p in out["0"][1]), out["0"][1]
    return out["1"]


@pytest.mark.parametrize("name", sorted(AGGS))
def test_packed_flushes_take_the_tag_path(monkeypatch, name):
    """Case 1.  The first flush epoch has no PF_PACK fields (PF_WIDE rows: entry table); from the second
    on every superbucket -- each has work in every launch -- is served by the tag path."""
    out = _both_modes(monkeypatch, _kw(name), _stream(1), cfg_extra=BIG)
    st, old, tag = out["1"]
    n_sb = st["num_superbuckets"]
    assert n_sb == 1024
    assert (old, tag) == (n_sb, (N_WM - 1) * n_sb), (old, tag)
    assert st["num_late_records_dropped"] == 0


@pytest.mark.parametrize("name", ["max", "sum"])
def test_state_lives_across_flushes(monkeypatch, name):
    """Case 2.  Windows of three watermark steps: a flush (a fired window, or eight pending pushes)
    loads entries earlier flushes wrote, extends them, writes them back, and a later one fires them.
    Values are negative (max) or near 2^62 (sum: a key's second row in a window crosses 2^63 and
    wraps, as Java's long does)."""
    batches = _stream(2, vbase=(1 << 62) if name == "sum" else -(10**7))
    out = _both_modes(monkeypatch, _kw(name, LONG), batches, cfg_extra=BIG)
    st, old, tag = out["1"]
    assert tag > 0 and st["live_state_entries"] > 0, (old, tag, st)


def _with_hot_key(batches, push, at, pool=POOL):
    """1500 rows of one (key, slice), a key no earlier push held, in the middle push of every watermark
    after the first"""
    for b, (k, t, iv, dv, wm) in enumerate(batches):
        if b == 0:
            continue
        o = push + at
        k[o:o + 1500] = pool[-1] + 7 * (b + 1)  # (inside the key field: its headroom is the pool's span)
        t[o:o + 1500] = T0 + b * STEP + 100
    return batches


def test_one_hot_key(monkeypatch):
    """Case 3.  The hot rows reach the merge unfolded (FW_IG_PACK=2: the packing ingest on every push).
    They overrun their superbucket's sub-run, so that superbucket keeps the entry table and the others
    take the tag path."""
    monkeypatch.setenv("FW_IG_PACK", "2")
    st, per_wm = _steps_both_modes(monkeypatch, _kw("sum"), _with_hot_key(_stream(3), PUSH, 700), cfg_extra=BIG)
    n_sb = st["num_superbuckets"]
    assert per_wm[1:] == [(1, n_sb - 1)] * (N_WM - 1), per_wm


def test_one_hot_key_on_the_tag_path(monkeypatch):
    """Case 3 where the tag path takes the hot rows: one superbucket, pushes of 2500 rows (its sub-runs
    hold 2576), 1200 keys.  1500 lanes race one compare-and-swap for the hot group's slot; the losers
    see its tag and fold into the same accumulator."""
    monkeypatch.setenv("FW_IG_PACK", "2")
    pool = POOL[:1200]
    batches = _with_hot_key(_stream(11, pool=pool, push=2500), 2500, 400, pool)
    st, per_wm = _steps_both_modes(monkeypatch, _kw("sum"), batches, cfg_extra=dict(max_parallelism=1, state_capacity=1024))
    assert st["num_superbuckets"] == 1
    assert per_wm == [(1, 0)] + [(0, 1)] * (N_WM - 1), per_wm


TWO = dict(max_parallelism=2, state_capacity=1024)  # two superbuckets


def test_crowded_table(monkeypatch):
    """Case 4.  Two superbuckets, 3000 keys and two live slices: about 2300 groups each in a table of
    8192 slots, so probe chains form.  With the module's pushes every chunk overruns its sub-run and the
    entry table serves the flushes; with pushes of 2200 rows the tag path does, from the second epoch on."""
    pool = np.arange(3000, dtype=np.int64) * 7 + 11
    st, per_wm = _steps_both_modes(monkeypatch, _kw("max"), _stream(4, pool=pool), cfg_extra=TWO)
    assert st["num_superbuckets"] == 2 and st["peak_superbucket_entries"] > 2000, st
    st, per_wm = _steps_both_modes(monkeypatch, _kw("max"), _stream(5, pool=pool, push=2200), cfg_extra=TWO)
    assert st["peak_superbucket_entries"] > 2000, st
    assert per_wm[0] == (2, 0) and all(p == (0, 2) for p in per_wm[1:]), per_wm


@pytest.mark.parametrize("push", [PUSH, 2200])
def test_state_overflow_is_reported(monkeypatch, push):
    """Case 4, beyond cap_e: 8000 keys on two superbuckets are more than 3072 groups each;
    FW_ERRF_STATE is raised in both modes (rows not compared).  While the bit is up the tables stay
    within their bounds, and the handle recovers: a snapshot taken while 500 keys were live, restored
    into the same handle after the overflow, continues with 500 keys bit-exactly against the oracle."""
    pool = np.arange(8000, dtype=np.int64) * 7 + 11
    for mode in ("1", "0"):
        monkeypatch.setenv("FW_MG_TAG", mode)
        cfg = _cfg(_kw("sum"), max_batch_rows=1 << 14, **TWO)
        st, _ = _run_steps(cfg, _stream(6, pool=pool, push=push), expect_error=abi.ERRF["STATE"])
        assert st["live_state_entries"] <= st["num_superbuckets"] * st["superbucket_capacity"], st
        assert st["peak_superbucket_entries"] > st["superbucket_capacity"], st
        _overflow_then_recover(cfg, _stream(12, pool=pool[:500], push=push), _stream(6, pool=pool, push=push))


def _overflow_then_recover(cfg, small, big):
    """`small` fits the state tables, `big` does not.  Batch 0 of `small`, a snapshot, `big` until the
    handle reports FW_ERRF_STATE, the snapshot restored into the same handle (the oracle restarts at the
    same cut), then the rest of `small`, every watermark's rows against the oracle."""
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    o, g = OracleOperator(cfg), WindowAggHandle(cfg)

    def step(bi):
        k, t, iv, dv, wm = small[bi]
        vals = [iv, dv.view(np.int64)]
        o.process_batch(k, t, vals, None)
        o.process_watermark(wm)
        for part in np.array_split(np.arange(len(k)), SPLIT):
            g.push_host(k[part], t[part], [v[part] for v in vals])
        g.advance(wm)
        _compare(_rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"batch {bi}")

    try:
        step(0)
        assert g.stats()["live_state_entries"] > 0
        blob = g.snapshot()
        o.snapshot_restore()
        with pytest.raises(_native.FlinkWinError) as err:
            for k, t, iv, dv, wm in big:
                for part in np.array_split(np.arange(len(k)), SPLIT):
                    g.push_host(k[part], t[part], [iv[part], dv.view(np.int64)[part]])
                g.advance(wm)
                g.results(reset=True)
        assert err.value.code == abi.FW_E_CAPACITY
        assert g.stats()["error_flags"] == abi.ERRF["STATE"]
        g.restore(blob)
        assert g.stats()["error_flags"] == 0
        for bi in range(1, len(small)):
            step(bi)
        st = g.stats()
        assert st["num_late_records_dropped"] == o.late_dropped and st["error_flags"] == 0, st
    finally:
        g.close()


def _key_group(keys):
    kg = np.zeros(len(keys), dtype=np.int32)
    rc = _native.lib().fw_host_assign_key_groups(keys.ctypes.data, None, len(keys), abi.KEYHASH_LONG, 128, 1,
                                                 kg.ctypes.data, None)
    assert rc == 0
    return kg


@pytest.mark.parametrize("what", ["wide_key", "far_slice", "sub_run_overflow"])
def test_fallbacks_inside_one_launch(monkeypatch, what):
    """Case 5.  In the middle push of every watermark after the first, one chunk keeps rows in its own
    region: a key 2^40 above the key field or a row 300 slices ahead (the chunk writes PF_WIDE rows), or
    300 keys of one key group (about 40 rows per superbucket against a sub-run of 32).  The superbuckets that
    chunk touches take the entry table, the others the tag path, in the same launch."""
    batches = _stream(7)
    hot = POOL[_key_group(POOL) == 5][:300]
    assert len(hot) == 300
    for b, (k, t, iv, dv, wm) in enumerate(batches):
        if b == 0:
            continue
        o = PUSH + CH
        if what == "wide_key":
            k[o + 100] += np.int64(1) << 40
        elif what == "far_slice":
            t[o + 17] = T0 + b * STEP + 300 * SIZE
        else:
            k[o:o + 300] = hot
    st, per_wm = _steps_both_modes(monkeypatch, _kw("sum"), batches, cfg_extra=BIG)
    n_sb = st["num_superbuckets"]
    assert per_wm[0] == (n_sb, 0), per_wm
    for old, tag in per_wm[1:]:
        assert old > 0 and tag > 0 and old + tag == n_sb, per_wm


def test_wide_key_pool_keeps_the_entry_table(monkeypatch):
    """Case 6.  A key pool that spans 33 bits: key and rank fields do not fit a tag, no superbucket
    takes the tag path (the rows are PF_PACK all the same)."""
    out = _both_modes(monkeypatch, _kw("max"), _stream(8, pool=np.arange(40000, dtype=np.int64) * 104729 + 11),
                      cfg_extra=BIG)
    st, old, tag = out["1"]
    assert (old, tag) == (N_WM * st["num_superbuckets"], 0), (old, tag)
    assert st["compact_chunks"] > 0, st


def test_state_that_no_longer_converts(monkeypatch):
    """Case 7.  Windows of three steps; after three watermarks the keys move up by 2 000 000, more than
    the 20-bit key field's headroom.  The flush at watermark 4 holds one push, packed with fields that
    cover the new keys, while the window the old keys opened is still live: every superbucket starts on
    the tag path, finds a state entry outside the field and restarts on the entry table."""
    batches = _stream(9)
    for b in range(3, N_WM):
        batches[b][0][:] += 2_000_000
    st, per_wm = _steps_both_modes(monkeypatch, _kw("sum", LONG), batches, cfg_extra=BIG)
    n_sb = st["num_superbuckets"]
    assert per_wm[4][0] >= n_sb and per_wm[4][1] == 0, per_wm
    assert st["compact_chunks"] > 0, st


def test_snapshot_and_restore(monkeypatch):
    """Case 8.  Snapshot after watermark 3 (live windows of three steps), restore into a fresh operator,
    continue: the rows equal the uninterrupted run's (the oracle's, which _run_both snapshots too)."""
    out = _both_modes(monkeypatch, _kw("min", LONG), _stream(10), cfg_extra=BIG, snapshot_at=3)
    assert out["1"][2] > 0, out["1"]
