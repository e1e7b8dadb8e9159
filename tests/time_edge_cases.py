"""Helpers of the time-edge tests (test_time_edges_reference.py on the CPU, test_gpu_time_edges.py on
the device); no tests here.

1. A plain-Python reference of the time windows, in Python integers wrapped to 64 bits only where
   Java wraps (`window_start`, `next_trigger_watermark`, the slice operations of fw_host_time_op),
   and a window operator defined by direct window assignment, not by slices (`Reference`):

     TUMBLE    the one window of ts;
     HOP       every window [s, s + size) with s on the slide grid (offset included), s <= ts < s + size;
     CUMULATE  the windows [ws, ws + k * step), k = 1 .. size / step, whose end is above ts, ws being
               the row's size-aligned start.

   A row is folded into each of its windows that has not fired (end - 1 <= W) at the watermark W in
   force when the row arrives; a row without such a window is a late drop; every non-empty window is
   emitted once, at the watermark that fires it.  COUNT(*), SUM (64-bit wrap), MIN and MAX over BIGINT.
   DataStream tumbling / sliding windows with allowedLateness = 0 are the same thing.

2. Stream builders with the time origin as a parameter (`build`): parity_common._stream's shape
   (rows spread over `step` ms per watermark, `ooo` ms of out-of-orderness, the watermark `lag` ms
   behind the batch's end), laid out in pushes of 3 chunks + 5 rows so that outliers can be placed by
   row position within a chunk.

3. The catalogue of cases both test modules run: ORIGINS, OUTLIERS, the interval configurations and the
   far-watermark schedule."""
from math import gcd

import numpy as np

from flink_amd import _native, abi

MIN_VALUE, MAX_VALUE = -(1 << 63), (1 << 63) - 1
I64 = abi.T_I64


# ---------------------------------------------------------------------------------------------------
# 1. the arithmetic
# ---------------------------------------------------------------------------------------------------
def wrap64(x):
    """A Java long: x modulo 2^64 in [-2^63, 2^63)."""
    return ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def java_rem(a, b):
    """Java's %: the remainder takes the dividend's sign."""
    r = abs(a) % b
    return -r if a < 0 else r


def window_start(ts, offset, size):
    """TimeWindow.getWindowStartWithOffset: ts - offset and both results wrap as Java longs.  Where
    nothing wraps this is the floor grid point, ts - ((ts - offset) mod size)."""
    rem = java_rem(wrap64(ts - offset), size)
    return wrap64(ts - (rem + size)) if rem < 0 else wrap64(ts - rem)


def next_trigger_watermark(wm, interval):
    """TimeWindowUtil.getNextTriggerWatermark (UTC)."""
    if wm == MAX_VALUE:
        return wm
    trig = wrap64(window_start(wm, 0, interval) + interval - 1)
    return trig if trig > wm else wrap64(trig + interval)


def slice_interval(kw):
    kind = kw["window_kind"]
    if kind == abi.WIN_TUMBLE:
        return kw["size_ms"]
    if kind == abi.WIN_HOP:
        return gcd(kw["size_ms"], kw["slide_ms"])
    return kw["slide_ms"]


def slice_end(kw, ts):
    """AbstractSliceAssigner.assignSliceEnd (UTC)."""
    iv = slice_interval(kw)
    return wrap64(window_start(ts, kw.get("offset_ms", 0), iv) + iv)


def window_start_of_end(kw, end):
    """SliceAssigner.getWindowStart of a window end."""
    if kw["window_kind"] == abi.WIN_CUMULATE:
        return window_start(wrap64(end - 1), kw.get("offset_ms", 0), kw["size_ms"])
    return wrap64(end - kw["size_ms"])


def windows_of(kw, ts):
    """The windows (start, end) of a row, newest end first.  No wrapping: the streams stay more than a
    window away from the ends of the long range."""
    kind, size, off = kw["window_kind"], kw["size_ms"], kw.get("offset_ms", 0)
    if kind == abi.WIN_TUMBLE:
        s = window_start(ts, off, size)
        return [(s, s + size)]
    if kind == abi.WIN_HOP:
        slide = kw["slide_ms"]
        s = window_start(ts, off, slide)
        out = []
        while s > ts - size:
            out.append((s, s + size))
            s -= slide
        return out
    step = kw["slide_ms"]
    ws = window_start(ts, off, size)
    return [(ws, ws + k * step) for k in range(size // step, 0, -1) if ws + k * step > ts]


def fired(end, wm):
    return end - 1 <= wm


def is_late(kw, ts, wm):
    """No window of the row is left to fire (allowedLateness = 0)."""
    return fired(windows_of(kw, ts)[0][1], wm)


class Reference:
    """The window operator by direct window assignment.  Rows as parity_common._rows makes them:
    (key, window start, window end, aggregate values, null mask 0)."""

    def __init__(self, kw):
        assert not kw.get("allowed_lateness_ms"), "positive lateness stays oracle-only"
        for kind, col, typ in kw["aggs"]:
            assert kind in (abi.AGG_COUNT_STAR, abi.AGG_SUM, abi.AGG_MIN, abi.AGG_MAX) and col == 0 and typ == I64
        self.kw = kw
        self.wm = MIN_VALUE
        self.late = 0
        self.state = {}  # (key, start, end) -> [count, sum, min, max]

    def process_batch(self, keys, ts, vals):
        cache = {}
        for k, t, v in zip(keys.tolist(), ts.tolist(), vals.tolist()):
            wins = cache.get(t)
            if wins is None:
                wins = cache[t] = [w for w in windows_of(self.kw, t) if not fired(w[1], self.wm)]
            if not wins:
                self.late += 1
                continue
            for s, e in wins:
                acc = self.state.get((k, s, e))
                if acc is None:
                    self.state[(k, s, e)] = [1, v, v, v]
                else:
                    acc[0] += 1
                    acc[1] += v
                    if v < acc[2]:
                        acc[2] = v
                    if v > acc[3]:
                        acc[3] = v

    def process_watermark(self, wm):
        """The rows this watermark fires, sorted."""
        if wm <= self.wm:
            return []
        self.wm = wm
        due = [w for w in self.state if fired(w[2], wm)]
        sel = {abi.AGG_COUNT_STAR: 0, abi.AGG_SUM: 1, abi.AGG_MIN: 2, abi.AGG_MAX: 3}
        rows = []
        for w in due:
            acc = self.state.pop(w)
            acc[1] = wrap64(acc[1])
            rows.append((w[0], w[1], w[2], tuple(acc[sel[kind]] for kind, _, _ in self.kw["aggs"]), 0))
        rows.sort()
        return rows


def reference_run(kw, steps):
    """(rows per watermark, late drops) of a stream's steps."""
    r = Reference(kw)
    out = []
    for keys, ts, iv, wm in steps:
        r.process_batch(keys, ts, iv)
        out.append(r.process_watermark(wm))
    return out, r.late


# ---------------------------------------------------------------------------------------------------
# 2. streams
# ---------------------------------------------------------------------------------------------------
# The ordinary schedule advances by 7 s per watermark: at least one slice of every configuration with a
# window offset.  The reference operator flushes its record buffer only when the watermark passes a
# point of the slice grid taken WITHOUT the offset (AbstractSliceSyncStateWindowAggProcessor
# .advanceProgress, TimeWindowUtil.getNextTriggerWatermark) and registers no timer for a window the
# previous watermark had fired (AggCombiner.combine), so a window with an offset whose end a watermark
# passes between two such points is emitted late, in parts, or never.  The oracle restates that; the
# reference above does not ("emitted once, at the watermark that fires it"), and the two coincide when
# every watermark passes such a point.  With 5 s steps sql_tumble_offset (7 s, offset -2.5 s) differs.
# Out-of-orderness 16 s and a lag of 4 s make every configuration below drop rows, the sliding windows
# of 7 s with 2.5 s of allowed lateness included.
T0 = 1_600_000_000_000
STEP, OOO, LAG = 7000, 16000, 4000
SPLIT = 3                           # pushes per watermark
FAR = (1 << 62)


def chunk_rows(kw):
    """Rows per ingest chunk (fw_internal.h: ig_block * ig_rpt): 4096 up to four accumulator words, as
    every configuration here has; a 2048-row chunk starts wherever a 4096-row one does."""
    assert len(kw["aggs"]) <= 4
    return 4096


def tbase_of(kw, ts0):
    """The base of the kernels' 32-bit slice arithmetic for a chunk whose first row is ts0
    (fw_ingest_impl.h, fw_ingest_pack.h), from the library's own window start."""
    iv = slice_interval(kw)
    assert iv < (1 << 30)
    off = kw.get("offset_ms", 0)
    if kw.get("api") == abi.API_DATASTREAM and kw["window_kind"] == abi.WIN_TUMBLE:
        off = java_rem(off, kw["size_ms"])
    return _native.lib().fw_host_window_start(int(ts0), off, iv) - ((1 << 30) // iv) * iv


FAR_AHEAD = ((1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, (1 << 31) + 5000, 1 << 33, 1 << 40)
OUTLIERS = ("far_ahead", "first_row_far", "tbase_boundary", "lone_2_32")


class Stream:
    """steps: [keys, ts, values, watermark] per watermark (a step may have no rows); outliers: per
    step the positions of the placed rows; push: rows per push (SPLIT pushes per step with rows)."""

    def __init__(self, steps, outliers, push, ordinary):
        self.steps, self.outliers, self.push, self.ordinary = steps, outliers, push, ordinary

    @property
    def n_rows(self):
        return sum(len(s[0]) for s in self.steps)


def build(seed, origin, pool, *, step=STEP, ooo=OOO, lag=LAG, n_wm=5, chunk=4096, distinct=True, outliers=None, kw=None,
          final_max=False, far_wm=False):
    """A stream of n_wm watermarks, SPLIT pushes of 3 chunks + 5 rows each.  Batch b lies in
    (base - ooo, base + step), base = origin + b * step, and is followed by the watermark
    base + step - lag.  Keys come from `pool`, distinct within a push if `distinct`.  The five rows that
    end a push are on time: a chunk none of whose rows survives has no row format, and the two ingest
    kernels count such a chunk differently in compact_chunks when it lies off the 32-bit path
    (k_ingest: compact, k_ingest_pack: not), which is no concern of the counters' comparison here.

    outliers (placed by row position; `kw` tells tbase_boundary the slice grid):
      far_ahead       one row in 16, never a chunk's row 0: base + FAR_AHEAD[...] in turn;
      first_row_far   row 0 of the middle chunk of each push: base + 2^31 + 5000, so every other row of
                      that chunk lies below its tbase;
      tbase_boundary  rows 1-4 of the middle chunk of each push: tbase - 1, tbase, tbase + 2^31 - 1 and
                      tbase + 2^31 of that chunk; the watermark schedule is shifted back by whole steps
                      until none of them is late when it arrives;
      lone_2_32       row 1 of the first chunk of each push: that chunk's tbase + 2^32 - 1, where a slice
                      end relative to tbase wraps in 32 bits to a small one, which the ordinary watermark
                      has passed (alone in its chunk: any row further off sends the whole chunk the
                      packing kernel's slow way, whatever the kernel makes of this one).
    final_max: a last watermark Long.MAX_VALUE.  far_wm: the schedule starts advance(MIN + 1), push,
    advance(-2^62), push, then goes on as usual, and ends with Long.MAX_VALUE."""
    rng = np.random.default_rng(seed)
    push = 3 * chunk + 5
    n = SPLIT * push
    batches, placed, shifted = [], [], False
    for b in range(n_wm):
        base = origin + b * step
        late_by = rng.integers(0, ooo, n)
        late_by[np.arange(n) % push >= 3 * chunk] = 0  # (the 5-row chunk of a push: see below)
        ts = (base + rng.integers(0, step, n) - late_by).astype(np.int64)
        if distinct:
            keys = np.concatenate([rng.permutation(pool)[:push] for _ in range(SPLIT)])
        else:
            keys = pool[rng.integers(0, len(pool), n)]
        iv = rng.integers(-10**6, 10**6, n).astype(np.int64)
        idx = np.zeros(0, np.int64)
        mid = np.arange(SPLIT) * push + chunk  # row 0 of each push's middle chunk
        if outliers == "far_ahead":
            idx = np.flatnonzero(np.arange(n) % push % 16 == 7)
            ts[idx] = base + np.array(FAR_AHEAD, dtype=np.int64)[np.arange(len(idx)) % len(FAR_AHEAD)]
        elif outliers == "first_row_far":
            idx = mid
            ts[idx] = base + (1 << 31) + 5000
        elif outliers == "tbase_boundary":
            idx = np.concatenate([m + 1 + np.arange(4) for m in mid])
            for m in mid:
                tb = tbase_of(kw, ts[m])
                ts[m + 1:m + 5] = (tb - 1, tb, tb + (1 << 31) - 1, tb + (1 << 31))
        elif outliers == "lone_2_32":
            idx = mid - chunk + 1
            for i in idx:
                ts[i] = tbase_of(kw, ts[i - 1]) + (1 << 32) - 1
        else:
            assert outliers is None
        batches.append([keys.astype(np.int64), ts, iv, base])
        placed.append(idx)
    if outliers == "tbase_boundary":  # no placed row late under the watermark before its batch
        need = max(bt[3] - min(windows_of(kw, int(t))[0][1] for t in bt[1][idx]) + 2
                   for bt, idx in zip(batches[1:], placed[1:]))
        if need > lag:
            lag += -(-(need - lag) // step) * step
            shifted = True
    none = np.zeros(0, np.int64)
    steps, outl = [], []
    if far_wm:
        steps.append([none, none, none, MIN_VALUE + 1])
        outl.append(none)
    for b, ((keys, ts, iv, base), idx) in enumerate(zip(batches, placed)):
        steps.append([keys, ts, iv, -FAR if far_wm and b == 0 else base + step - lag])
        outl.append(idx)
    if final_max or far_wm:
        steps.append([none, none, none, MAX_VALUE])
        outl.append(none)
    return Stream(steps, outl, push, ordinary=not shifted)


# ---------------------------------------------------------------------------------------------------
# 3. the cases
# ---------------------------------------------------------------------------------------------------
# Time origins, each off every window grid in use, so that some rows of every configuration are late.
# straddle_zero / pos_2_61 / neg_2_61: batch 2 (the third watermark's rows) lies on both sides of 0 /
# +2^61 / -2^61, the bound of the kernels' `fast` test on a chunk's first row.
ORDINARY = T0 + 1877
ORIGINS = {
    "neg_epoch": -1_600_000_000_123,
    "straddle_zero": -2 * STEP - 1877,
    "pos_2_61": (1 << 61) - 2 * STEP - 1877,
    "neg_2_61": -(1 << 61) - 2 * STEP - 1877,
    "at_2_62": (1 << 62) + 3,
}
OUTLIER_ORIGINS = {"ordinary": ORDINARY, "neg_epoch": ORIGINS["neg_epoch"]}

DAY = 86_400_000
TUMBLE_SIZES = {"1": (1, 0), "2": (2, 0), "2_30m1": ((1 << 30) - 1, 0), "2_30": (1 << 30, 0), "2_30p1": ((1 << 30) + 1, 0),
                "30d": (30 * DAY, -8 * 3_600_000)}  # name -> (size, offset)
HOP_BIG = dict(window_kind=abi.WIN_HOP, size_ms=2 * ((1 << 29) + 1), slide_ms=(1 << 29) + 1, count_star_index=0,
               aggs=[(abi.AGG_COUNT_STAR, 0, I64), (abi.AGG_SUM, 0, I64)])
CUMULATE_BIG = dict(window_kind=abi.WIN_CUMULATE, size_ms=4 << 30, slide_ms=1 << 30, count_star_index=0,
                    aggs=[(abi.AGG_COUNT_STAR, 0, I64), (abi.AGG_SUM, 0, I64), (abi.AGG_MIN, 0, I64), (abi.AGG_MAX, 0, I64)])


def interval_shape(interval, offset=0, align=None):
    """(origin, step, ooo, lag, key pool size) of an interval case: step = interval and
    out-of-orderness = interval / 2 at an ordinary time; sizes 1 and 2 take a step of 40 ms and about 50
    keys, which keeps a watermark's output small.  The origin lies a fifth of the interval above the
    window grid, so that the watermark (a sixth of the interval behind the batch's end) has just fired
    the window the batch's oldest rows belong to; `align`: the grid that batch 2 starts on (CUMULATE:
    its size, whose windows are the ones that make a row late)."""
    if interval <= 2:
        return ORDINARY, 40, 20, 6, 50
    align = align or interval
    origin = window_start(T0, offset, align) + align - 2 * interval + interval // 5
    ooo = interval // 2
    return origin, interval, ooo, ooo // 3, None


MAX5S = dict(window_kind=abi.WIN_TUMBLE, size_ms=5000, aggs=[(abi.AGG_MAX, 0, I64)])    # one accumulator word
COUNT5S = dict(window_kind=abi.WIN_TUMBLE, size_ms=5000, aggs=[(abi.AGG_COUNT_STAR, 0, I64)])  # PF_UNIT rows


def configs():
    """name -> configuration keywords of the origin and outlier cases; the first REFERENCE of them
    have no allowed lateness (the plain-Python reference covers those)."""
    from parity_common import CASES
    out = {"max5s": MAX5S, "count5s": COUNT5S}
    for name in ("sql_tumble_int_aggs", "sql_tumble_offset", "sql_hop_offset", "sql_cumulate_countstar", "ds_tumble_sum",
                 "ds_sliding_nondiv_sum", "ds_tumble_lateness", "ds_sliding_nondiv_lateness_side_output"):
        out[name] = CASES[name]
    return out


REFERENCE = 8
STREAM_CASES = [f"origin-{o}" for o in ORIGINS] + [f"{k}-{o}" for k in OUTLIERS for o in OUTLIER_ORIGINS]


def _seed(*parts):
    import zlib
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def case_stream(case, kw, pool, **layout):
    """The stream of one of STREAM_CASES for a configuration (layout: build's chunk, n_wm, distinct)."""
    kind, name = case.split("-")
    if kind == "origin":
        return build(_seed(case), ORIGINS[name], pool, **layout)
    return build(_seed(case), OUTLIER_ORIGINS[name], pool, outliers=kind, kw=kw, final_max=True, **layout)


def with_size(kw, size, offset):
    kw = dict(kw, size_ms=size)
    kw.pop("offset_ms", None)
    if offset:
        kw["offset_ms"] = offset
    return kw


def interval_cases():
    """name -> (configuration keywords, (origin, step, ooo, lag, pool size or None)) of the interval set:
    the TUMBLE sizes against the one-word MAX, sql_tumble_int_aggs and a DataStream tumbling sum, and
    the HOP / CUMULATE configurations with slices of 2^29 + 1 and 2^30 ms."""
    from parity_common import CASES
    out = {}
    for sname, (size, off) in TUMBLE_SIZES.items():
        for cname, kw in (("max", MAX5S), ("int_aggs", CASES["sql_tumble_int_aggs"]), ("ds_sum", CASES["ds_tumble_sum"])):
            out[f"tumble_{sname}-{cname}"] = (with_size(kw, size, off), interval_shape(size, off))
    out["hop_2_29p1"] = (HOP_BIG, interval_shape(HOP_BIG["slide_ms"]))
    out["cumulate_2_30"] = (CUMULATE_BIG, interval_shape(CUMULATE_BIG["slide_ms"], align=CUMULATE_BIG["size_ms"]))
    return out


# Interval cases without a late row, and why.  (Every other case drops 1 % to 50 % of its rows.)
NO_LATE_ROWS = {
    "hop_2_29p1": "size = 2 * slide and the rows reach half a slide back: a row's newest window ends more than a slide "
                  "after the row, the watermark before its batch lies less than a slide after the batch's oldest row",
}


def interval_stream(name, shape, pool, **layout):
    origin, step, ooo, lag, n_keys = shape
    if n_keys is not None:
        pool, layout = pool[:n_keys], dict(layout, distinct=False)
    return build(_seed("interval", name), origin, pool, step=step, ooo=ooo, lag=lag, **layout)


def far_watermark_stream(pool, **layout):
    return build(_seed("far_wm"), ORDINARY, pool, far_wm=True, **layout)


def values_of(iv):
    """The value columns of parity_common.VT: the BIGINT column and a DOUBLE one derived from it."""
    return [iv, (iv.astype(np.float64) * 0.5).view(np.int64)]


def oracle_run(cfg, stream, snapshot_at=None):
    """(rows per watermark, late drops, late side output per watermark) of the oracle."""
    from oracle.oracle import OracleOperator
    from parity_common import _rows
    o = OracleOperator(cfg)
    rows, side = [], []
    for si, (keys, ts, iv, wm) in enumerate(stream.steps):
        if len(keys):
            o.process_batch(keys, ts, values_of(iv), None)
        o.process_watermark(wm)
        rows.append(_rows(o.results(clear=True), cfg, set()))
        side.append(o.side_output() if cfg.late_side_output else None)
        if si == snapshot_at:
            o.snapshot_restore()
    late = o.late_dropped
    o.close()
    return rows, late, side


def check_conditions(kw, stream, rows, late, no_late_rows=False):
    """The conditions on a case's input, on the oracle's output: they keep a case from passing
    vacuously.  Returns the late-drop share."""
    plain = {k: v for k, v in kw.items() if k not in ("allowed_lateness_ms", "late_side_output")}
    share = late / stream.n_rows
    if no_late_rows:
        assert late == 0
    elif stream.ordinary:
        assert 0.01 <= share <= 0.5, f"late-drop share {share:.4f}"
    assert sum(1 for r in rows if r) >= 3, [len(r) for r in rows]
    emitted = {(r[0], r[2]) for rs in rows for r in rs}
    final = {(r[0], r[2]) for r in rows[-1]}
    wm, last = MIN_VALUE, max(s[3] for s in stream.steps[:-1])
    for (keys, ts, _, nwm), idx in zip(stream.steps, stream.outliers):
        for k, t in zip(keys[idx].tolist(), ts[idx].tolist()):
            end = windows_of(plain, t)[0][1]
            assert not fired(end, wm), ("outlier row late", k, t, wm)
            assert (k, end) in (emitted if fired(end, last) else final), ("outlier row not emitted", k, t)
        wm = max(wm, nwm)
    return share
