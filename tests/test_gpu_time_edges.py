"""GPU tests of the time-window kernels at the edges of their time arithmetic (k_ingest, k_ingest_pack,
k_merge_fire, k_merge_hopb: fw_ingest_impl.h, fw_ingest_pack.h, fw_merge_impl.h, fw_merge_hopb.h).

Every other GPU test of the TUMBLE / HOP / CUMULATE path starts at t0 = 1 600 000 000 000 with windows
of seconds; the kernels branch on the time axis itself: the `fast` test on a chunk's first row
(|ts0| < 2^61), the 32-bit slice arithmetic for rows within 2^31 ms of the chunk's base tbase, the
64-bit magic division for every other row, fast32 = interval < 2^30, the rank limit of compact rows,
window_start's negative branch, the 31-bit block index of the narrow HOP block layouts.  The streams
here come from time_edge_cases.py (origins, outliers placed by row position, intervals, watermarks far
from the data); test_time_edges_reference.py pins the oracle on the same streams against a
plain-Python reference, and this module compares the handle with the oracle: after every watermark
the rows bit for bit, at the end the late-drop counter and error_flags == 0.  No DOUBLE SUM / AVG
appears, so nothing takes a tolerance.

The shape is test_gpu_ingest_policy.py's: pushes of 3 chunks + 5 rows (chunks of 4096 rows: every
configuration here has at most four accumulator words), 3 pushes per watermark, 5 watermarks,
max_batch_rows = 1 << 14.  The one-word TUMBLE and the COUNT(*)-only TUMBLE draw their keys from 40 000,
distinct within a push (what k_ingest_pack is made for); the others draw 2000 keys with repetition, so
that k_ingest folds.  Conditions on the inputs are asserted on the oracle's output
(time_edge_cases.check_conditions): 1 % to 50 % of the rows late where the watermark schedule is the
ordinary one, rows fired by at least three watermarks, every placed outlier row emitted and none late.

Where the library reports the path taken (compact_chunks, ingest_pack_launches,
merge_path_superbuckets) the cases named for a branch assert it.  The layout level the HOP block
state chooses has no counter: the block-index cases rely on the origin alone (block indices on both
sides of 2^31, or negative) and on running the three FW_HB_NARROW settings."""
import functools

import numpy as np
import pytest

import time_edge_cases as E
from flink_amd import abi
from parity_common import I64, _cfg, _compare, _rows

pytestmark = pytest.mark.gpu

N_WM = 5
POOL = np.arange(40000, dtype=np.int64) * 7 + 11   # test_gpu_merge_tag.py's: key fields the tag path takes
SMALL = np.arange(2000, dtype=np.int64) * 7919 - 50000
CFG = dict(max_batch_rows=1 << 14, state_capacity=1 << 19, output_capacity=1 << 20)
CONFIGS = E.configs()
ONE_WORD = ("max5s", "count5s")
COUNTERS = ("num_late_records_dropped", "partials_emitted", "partial_bytes_written", "compact_chunks")
PACKED_PUSHES = (N_WM - 1) * E.SPLIT  # the pushes after the first flush epoch
SPLIT4 = E.SPLIT * 4                  # the chunks of one watermark


def _layout(config):
    one = config in ONE_WORD or config.endswith("-max")
    return (POOL if one else SMALL), dict(chunk=4096, n_wm=N_WM, distinct=one)


@functools.lru_cache(maxsize=2)
def _case(kind, name, config, snapshot_at=None):
    """(configuration, stream, the oracle's (rows per watermark, late drops, side output)) of a case;
    the conditions on the input are checked here.  Shared by the runs of one case."""
    if kind == "stream":
        kw = CONFIGS[config]
        pool, layout = _layout(config)
        stream = E.case_stream(name, kw, pool, **layout)
    elif kind == "control":  # an outlier case's stream without the outliers
        kw = CONFIGS[config]
        pool, layout = _layout(config)
        stream = E.build(E._seed("control", name), E.OUTLIER_ORIGINS[name], pool, final_max=True, **layout)
    elif kind == "interval":
        kw, shape = E.interval_cases()[name]
        pool, layout = _layout(name)
        stream = E.interval_stream(name, shape, pool, **layout)
    elif kind == "far_wm":
        kw = CONFIGS[config]
        pool, layout = _layout(config)
        stream = E.far_watermark_stream(pool, **layout)
    else:
        kw = HOPB
        stream = E.build(E._seed("hopb", name), HOPB_ORIGINS[name], SMALL, chunk=4096, n_wm=N_WM, distinct=False, final_max=True)
    cfg = _cfg(kw, **CFG)
    want = E.oracle_run(cfg, stream, snapshot_at)
    late = want[1] + sum(len(s["key"]) for s in want[2] if s is not None)  # (dropped, or sent to the late side output)
    share = E.check_conditions(kw, stream, want[0], late, no_late_rows=name in E.NO_LATE_ROWS)
    print(f"{kind} {name} {config}: {stream.n_rows} rows, late-drop share {share:.4f}, "
          f"rows fired per watermark {[len(r) for r in want[0]]}")
    return cfg, stream, want


def _run(cfg, stream, want, snapshot_at=None):
    """The handle against the oracle's output.  Returns the final stats, the handle's k_ingest_pack
    launch count after every push and its (entry-table, tag) superbucket counts after every watermark."""
    from flink_amd.runtime.handle import WindowAggHandle
    rows, late, side = want
    g = WindowAggHandle(cfg)
    taken, paths = [], []
    try:
        for si, (keys, ts, iv, wm) in enumerate(stream.steps):
            if len(keys):
                vals = E.values_of(iv)
                for p in range(E.SPLIT):
                    sl = slice(p * stream.push, (p + 1) * stream.push)
                    g.push_host(keys[sl], ts[sl], [v[sl] for v in vals])
                    taken.append(g.ingest_pack_launches())
            g.advance(wm)
            _compare(_rows(g.results(reset=True), cfg, set()), rows[si], set(), f"watermark {si} ({wm})")
            paths.append(g.merge_path_superbuckets())
            if cfg.late_side_output:  # the same elements, as a multiset
                sg, so = g.late_records(), side[si]
                as_rows = lambda d: sorted(zip(d["key"].tolist(), d["ts"].tolist(), d["values"][1].tolist()))
                assert as_rows(sg) == as_rows(so), f"watermark {si}: late side output differs"
            if si == snapshot_at:
                blob = g.snapshot()
                g.close()
                g = WindowAggHandle(cfg)
                g.restore(blob)
        st = g.stats()
        assert st["num_late_records_dropped"] == late
        assert st["error_flags"] == 0, st["error_flags"]
    finally:
        g.close()
    return st, taken, paths


def _pack_modes(monkeypatch, case, counters=COUNTERS, packs=True):
    """FW_IG_PACK = 2 and 0 on one case: {mode: (stats, launches, paths)}; the counters agree.  packs:
    whether the handle is one the packing kernel serves at all (then it takes every push of mode 2)."""
    cfg, stream, want = case
    out = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("FW_IG_PACK", mode)
        out[mode] = _run(cfg, stream, want)
    for c in counters + ("error_flags",):
        assert out["0"][0][c] == out["2"][0][c], (c, out["0"][0][c], out["2"][0][c])
    n_push = sum(1 for s in stream.steps if len(s[0])) * E.SPLIT
    assert out["2"][1][-1] == (n_push if packs else 0) and out["0"][1][-1] == 0
    return out


# ---------------------------------------------------------------------------------------------------
# origins and outliers against every configuration
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.STREAM_CASES)
def test_one_word_tumble_pack_modes(monkeypatch, case):
    """TUMBLE MAX(BIGINT) 5 s through k_ingest_pack (FW_IG_PACK=2) and through k_ingest (=0).

    first_row_far: row 0 of each push's middle chunk lies 2^31 + 5000 ms ahead, every other row of the
    chunk below tbase; the packing kernel sends exactly that chunk of every push the slow way, against
    a control run of the same shape without outliers, which packs every chunk after the first epoch.
    lone_2_32: the one case in which a row 2^31 .. 2^32 ms past tbase is alone in its chunk, so that the
    packing kernel's `near` test on that row decides (a slice end taken in 32 bits would wrap below the
    watermark and the row be dropped as late).  origin: exactly the chunks whose first row passes the
    `fast` test pack."""
    cfg, stream, want = _case("stream", case, "max5s")
    out = _pack_modes(monkeypatch, (cfg, stream, want))
    packed = out["2"][0]["compact_chunks"]
    kind, origin = case.split("-")
    if kind == "first_row_far":
        control = _pack_modes(monkeypatch, _case("control", origin, "max5s"))
        assert control["2"][0]["compact_chunks"] == PACKED_PUSHES * 4
        assert packed == PACKED_PUSHES * 3
    elif kind == "origin":
        # the chunks after the first epoch whose first row passes the `fast` test pack, no other does
        first_rows = np.concatenate([s[1][p * stream.push:(p + 1) * stream.push:4096] for s in stream.steps[1:]
                                     for p in range(E.SPLIT)])
        n_fast = int((np.abs(first_rows) < (1 << 61)).sum())
        print(f"{case}: {packed} compact chunks, {n_fast} of {len(first_rows)} chunks fast")
        assert len(first_rows) == PACKED_PUSHES * 4
        if origin == "at_2_62":
            assert n_fast == 0
        elif origin in ("pos_2_61", "neg_2_61"):  # chunks on both sides of the bound
            assert SPLIT4 <= n_fast <= (PACKED_PUSHES - 1) * 4
        else:  # negative times take the packing kernel's fast path and the merge's tag path
            assert n_fast == PACKED_PUSHES * 4 and out["2"][2][-1][1] > 0
        assert packed == n_fast


@pytest.mark.parametrize("case", E.STREAM_CASES)
def test_one_word_tumble_entry_table_merge(monkeypatch, case):
    """The same with FW_MG_TAG=0: the entry table serves every superbucket."""
    monkeypatch.setenv("FW_MG_TAG", "0")
    _, _, paths = _run(*_case("stream", case, "max5s"))
    assert paths[-1][1] == 0


@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "max5s"])
@pytest.mark.parametrize("case", E.STREAM_CASES)
def test_origins_and_outliers(case, config):
    """COUNT(*)-only TUMBLE (PF_UNIT rows), the SQL TUMBLE / HOP / CUMULATE configurations with and
    without offset and the DataStream tumbling and sliding windows, allowed lateness and the late
    side output included."""
    _run(*_case("stream", case, config))


# ---------------------------------------------------------------------------------------------------
# intervals
# ---------------------------------------------------------------------------------------------------
INTERVALS = E.interval_cases()


@pytest.mark.parametrize("name", sorted(INTERVALS))
def test_intervals(monkeypatch, name):
    """TUMBLE sizes 1, 2 (the smallest dividers, tbase 2^30 slices back), 2^30 - 1 (the largest 32-bit
    interval: two ranks), 2^30, 2^30 + 1 and 30 d with offset -8 h (fast32 off: no compact rows, no
    PF_PACK, every row through the 64-bit division), HOP with a slide of 2^29 + 1 (the merge's
    slot_base + rank * interval near 2^31) and CUMULATE with steps of 2^30.  The one-word TUMBLE runs
    under FW_IG_PACK = 2 and 0."""
    case = _case("interval", name, None)
    big = E.slice_interval(INTERVALS[name][0]) >= 1 << 30
    if name.endswith("-max"):
        # The late drops agree, and the partial rows unless keys repeat (sizes 1 and 2: 50 keys, k_ingest
        # folds what the packing kernel cannot).  The row formats need not: with a slice of 2^30 - 1 ms a
        # chunk reaches 2^31 ms past its tbase, which sends the whole chunk the packing kernel's slow way
        # and only the row itself k_ingest's general way.
        few_keys = INTERVALS[name][1][4] is not None
        out = _pack_modes(monkeypatch, case, counters=COUNTERS[:1] if few_keys else COUNTERS[:2], packs=not big)
        st = out["2"][0]
    else:
        st, _, _ = _run(*case)
    if big:
        assert st["compact_chunks"] == 0  # fast32 is off: no compact rows, nothing packs


# ---------------------------------------------------------------------------------------------------
# watermarks far from the data
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["max5s", "sql_tumble_int_aggs", "ds_tumble_sum"])
def test_far_watermarks(monkeypatch, config):
    """advance(Long.MIN_VALUE + 1), push, advance(-2^62), push, the ordinary schedule, Long.MAX_VALUE.
    In k_ingest_pack only the guard on the rank base keeps wm1 = watermark - tbase + 1 from wrapping and
    making every row late; such chunks go the slow way, so no superbucket takes the tag path before the
    ordinary schedule starts (and some do after it has)."""
    case = _case("far_wm", "far_wm", config)
    if config != "max5s":
        _run(*case)
        return
    monkeypatch.setenv("FW_MG_TAG", "1")
    out = _pack_modes(monkeypatch, case)
    for mode in ("2", "0"):
        paths = out[mode][2]
        assert paths[1][1] == 0, paths  # after advance(-2^62)
    assert out["2"][2][-1][1] > 0, out["2"][2]


# ---------------------------------------------------------------------------------------------------
# HOP block state: the block index
# ---------------------------------------------------------------------------------------------------
HOPB = dict(window_kind=abi.WIN_HOP, size_ms=6000, slide_ms=2000, count_star_index=0,
            aggs=[(abi.AGG_COUNT_STAR, 0, I64), (abi.AGG_SUM, 0, I64)])
HB_SPAN = 8 * 2000  # HB_R slices of gcd(size, slide)
HOPB_ORIGINS = {"index_2_31": (1 << 31) * HB_SPAN - 2 * E.STEP - 1877, "neg_epoch": E.ORIGINS["neg_epoch"]}


@pytest.mark.parametrize("origin,narrow", [("index_2_31", "2"), ("index_2_31", "1"), ("index_2_31", "0"), ("neg_epoch", "2")])
def test_hop_block_index(monkeypatch, origin, narrow):
    """HOP 6000 / 2000 keeps block state (k_merge_hopb) in blocks of 16 000 ms.  A narrow layout keeps
    the block index in 31 bits, so a superbucket with a live block index >= 2^31 -- every negative block
    start included -- must stay wide.  index_2_31: the block indices pass 2^31 in the third watermark's
    rows, and a snapshot / restore follows that watermark; neg_epoch: narrow is refused from the start.
    (The level chosen has no counter; the values fit int32, so below 2^31 the narrow layout is taken.)"""
    monkeypatch.setenv("FW_HB_NARROW", narrow)
    cfg, stream, want = _case("hopb", origin, None, snapshot_at=2)
    b2 = stream.steps[2][1]
    if origin == "index_2_31":
        assert b2.min() // HB_SPAN < (1 << 31) <= b2.max() // HB_SPAN
    else:
        assert stream.steps[-2][1].max() < 0
    _run(cfg, stream, want, snapshot_at=2)
