"""Inputs of the folded paths' capacity tests (test_gpu_folded_capacity_limits.py) and the capped
reference they are compared with.  test_folded_capacity_inputs.py runs every builder against the
plain references alone, so a GPU test cannot pass because its input missed the edge.

The lever: a HOST_HASHED operator that is handed one hash for every key keeps all keys in one
superbucket, and the partition is stable, so with max_batch_rows a multiple of 1024 tile j of a push
is rows [1024 j, 1024 (j + 1)) of that push in arrival order.

A session push is a ``Push``: keys, timestamps and the value columns of its kind --
  static   keyBy().window(EventTimeSessionWindows.withGap(G)), sum LONG      k_sw_fold<1>
  dynamic  withDynamicGap, a gap per row (<= G), sum LONG                    k_sw_fold<1, true>
  sql2 / sql4 / sql8   the SQL SESSION TVF aggregate with 2, 4, 8 words      k_sw_fold<2>, <4>, <8>
"""
import copy

import numpy as np
from count_window_reference import CountWindowReference
from dynamic_session_reference import DynamicSessionReference
from session_window_reference import SessionWindowReference
from sql_session_reference import SqlSessionReference

TILE = 1024
G = 10                      # the session gap of every case (dynamic: the largest gap)
LONG_MAX = (1 << 63) - 1
KINDS = ("static", "dynamic", "sql2", "sql4", "sql8")
AGG = ("sum", "LONG")
# test_gpu_sql_session_windows.LAYOUTS[2], [4], [8] (the GPU module asserts that they are the same)
LAYOUTS = {
    2: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT")], ["BIGINT"], (0,)),
    4: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT"), ("MIN", 1, "INT"), ("COUNT_STAR", 0, "BIGINT"), ("AVG", 0, "BIGINT")],
        ["BIGINT", "INT"], (0,)),
    8: ([("SUM", 0, "BIGINT"), ("AVG", 1, "DOUBLE"), ("MIN", 2, "INT"), ("MAX", 2, "INT"), ("COUNT", 1, "DOUBLE"),
         ("COUNT_STAR", 0, "BIGINT"), ("SUM", 1, "DOUBLE")], ["BIGINT", "DOUBLE", "INT"], (0, 1, 2)),
}


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def layout_of(kind):
    return LAYOUTS[int(kind[3:])] if kind.startswith("sql") else None


class Push:
    """one push of a session case: k, ts and the kind's columns (v, g | vals, nulls)"""

    def __init__(self, kind, k, ts, g=None, seed=0):
        rng = np.random.default_rng(seed)
        self.kind, self.k, self.ts = kind, _i64(k), _i64(ts)
        n = len(self.k)
        self.g = np.full(n, G, np.int64) if g is None else _i64(g)
        self.v = rng.integers(-10**6, 10**6, n).astype(np.int64)
        self.vals, self.nulls = [], {}
        if kind.startswith("sql"):
            _, types, nullable = layout_of(kind)
            for c, t in enumerate(types):
                if t == "DOUBLE":
                    self.vals.append(rng.uniform(0.5, 100.0, n))
                elif t == "INT":
                    self.vals.append(rng.integers(-1000, 1000, n).astype(np.int64))
                else:
                    self.vals.append(rng.integers(-10**12, 10**12, n).astype(np.int64))
                if c in nullable:
                    self.nulls[c] = rng.random(n) < 0.3

    def __len__(self):
        return len(self.k)

    def take(self, sel):
        p = copy.copy(self)
        p.k, p.ts, p.g, p.v = self.k[sel], self.ts[sel], self.g[sel], self.v[sel]
        p.vals = [x[sel] for x in self.vals]
        p.nulls = {c: f[sel] for c, f in self.nulls.items()}
        return p

    def shuffled(self, seed):
        return self.take(np.random.default_rng(seed).permutation(len(self)))

    def feed(self, ref):
        """the push, element by element, into a plain reference: the indices dropped as late"""
        k, ts = self.k.tolist(), self.ts.tolist()
        if self.kind == "static":
            return ref.process(k, ts, self.v.tolist())
        if self.kind == "dynamic":
            return ref.process(k, ts, self.v.tolist(), self.g.tolist())
        cols = [x.tolist() for x in self.vals]
        flags = {c: f.tolist() for c, f in self.nulls.items()}
        return ref.process(k, ts, [[None if c in flags and flags[c][i] else cols[c][i] for c in range(len(cols))]
                                   for i in range(len(k))])


def concat(pushes):
    p = copy.copy(pushes[0])
    for name in ("k", "ts", "g", "v"):
        setattr(p, name, np.concatenate([getattr(q, name) for q in pushes]))
    p.vals = [np.concatenate([q.vals[c] for q in pushes]) for c in range(len(p.vals))]
    p.nulls = {c: np.concatenate([q.nulls[c] for q in pushes]) for c in p.nulls}
    return p


def plain_reference(kind):
    if kind == "static":
        return SessionWindowReference(G, AGG)
    if kind == "dynamic":
        return DynamicSessionReference(AGG)
    return SqlSessionReference(G, layout_of(kind)[0])


def tile_sessions(push):
    """the sessions the push's rows form among themselves under no watermark: what k_sw_fold counts as
    `may_add` (fw_session.hip:249) for a tile without late candidates"""
    ref = plain_reference(push.kind)
    push.feed(ref)
    return ref.live_sessions()


class CappedReference:
    """The plain reference under the contract k_sw_fold's comments give (fw_session.hip:493-499): a push
    is cut into tiles of 1024 rows; a tile is fed to a copy of the reference; if the copy then holds more
    than ``cap_s`` sessions the copy's sessions are thrown away -- the tile is dropped whole -- but its
    late drops stay counted (the kernel counts them at :346-375, before it decides) and the STATE bit
    is up; otherwise the copy becomes the reference.  All keys share one superbucket, so the list's
    length is the reference's live sessions.  ``cap_s`` None: no cap."""

    def __init__(self, kind, cap_s=None):
        self.kind, self.cap_s = kind, cap_s
        self.ref = plain_reference(kind)
        self.fired = 0
        self.state_bit = False
        self.tiles = []     # of every tile pushed: (dropped, sessions held behind it, sessions held before it, its own sessions)

    def push(self, p):
        """the indices (in the push) of the rows dropped as late, dropped tiles' included"""
        late = []
        for a in range(0, len(p), TILE):
            t = p.take(slice(a, a + TILE))
            trial = copy.deepcopy(self.ref)
            late += [a + i for i in t.feed(trial)]
            before = self.ref.live_sessions()
            if self.cap_s is not None and trial.live_sessions() > self.cap_s:
                self.ref.late_dropped = trial.late_dropped
                self.state_bit = True
                self.tiles.append((True, before, before, tile_sessions(t)))
            else:
                self.ref = trial
                self.tiles.append((False, trial.live_sessions(), before, tile_sessions(t)))
        return late

    def wm(self, w):
        rows = self.ref.process_watermark(w)
        self.fired += len(rows)
        return rows

    @property
    def late_dropped(self):
        return self.ref.late_dropped

    @property
    def watermark(self):
        return self.ref.watermark

    def live(self):
        return self.ref.live_sessions()

    def snapshot(self):
        return copy.deepcopy(self.ref)

    def restore(self, snap):
        """a whole-handle restore into the same handle: sessions and watermark come back, the error bits
        are cleared, the late-drop and fired counters -- metrics of the handle, not state -- go on"""
        dropped = self.ref.late_dropped
        self.ref = copy.deepcopy(snap)
        self.ref.late_dropped = dropped
        self.state_bit = False


def merged_order(state, push):
    """the order of k_sw_fold's merged list M for a tile without late candidates: every held session
    (key, start) and every row (key, ts) by key, then time, a session before a row of its time
    (fw_session.hip:292-327).  ``state``: [(key, start)].  Entries are ("s" | "r", key, time)."""
    ent = [(int(k), int(s), 0) for k, s in state] + [(int(k), int(t), 1) for k, t in zip(push.k, push.ts)]
    ent.sort()
    return [("sr"[tag], k, t) for k, t, tag in ent]


# ---- the 40 sessions every cap_s = 64 case starts from ------------------------------------------------
def seed40(kind):
    """keys 0 .. 29 hold [1000, 1015); keys 30 .. 34 hold [1000, 1010) and a second session that a row at
    1010 bridges: [1020, 1030) (even keys: touching) or [1016, 1026) (odd keys: overlapping)"""
    k, ts = [], []
    for q in range(30):
        k += [q, q]
        ts += [1000, 1005]
    for q in range(30, 35):
        k += [q, q]
        ts += [1000, 1020 if q % 2 == 0 else 1016]
    return Push(kind, k, ts, seed=1)


def _joiners(rng, n, keys):
    """n rows that join the session at [1000, 1010+) of one of ``keys`` and open none: ts in
    [996, 1008]; a dynamic row at or behind 1000 may carry a short gap (its window lies inside)"""
    k = rng.choice(keys, n)
    ts = rng.integers(996, 1009, n)
    g = np.where(ts >= 1000, rng.choice([1, 2, G], n), G)
    return k.tolist(), ts.tolist(), g.tolist()


# ---- case 1: tight and fits, small list ---------------------------------------------------------------
def case1(kind, final):
    """cap_s = 64, 40 held sessions; one tile of about 590 rows after which the list holds ``final``
    (63, 64, 65) sessions: per key 0 .. 29 eight rows chaining forward from its session, eight chaining
    backward and two inside it; per key 30 .. 34 the bridge and two inside; final - 35 rows that open a
    session (a new key, or a held key far away).  Shuffled: forward and backward arrival both occur."""
    k, ts, g = [], [], []
    for q in range(30):
        for i in range(8):
            k += [q, q]
            ts += [1008 + 6 * i, 994 - 6 * i]
            g += [G, G]
        k += [q, q]
        ts += [1002, 1003]
        g += [1, 3]
    for q in range(30, 35):
        k += [q, q, q]
        ts += [1010, 1001, 1022]
        g += [G, 2, 2]
    n_new = final - 35      # 40 held - 5 bridged + n_new
    for j in range(n_new):
        k.append(100 + j if j % 2 == 0 else j % 30)
        ts.append(1000 if j % 2 == 0 else 5000 + 50 * j)
        g.append(G)
    tile = Push(kind, k, ts, g, seed=10 + final).shuffled(final)
    return {"cap_s": 64, "seed": seed40(kind), "tile": tile, "held": 40, "final": final, "drops": final > 64}


# ---- case 2: tight and fits, two chunks ------------------------------------------------------------------
SPAN_KEY = 500


def case2(kind, n_new):
    """cap_s = 1024, 1000 held sessions (keys 0 .. 999, one each); a full tile with ``n_new`` (24, 25)
    rows that open a session.  Key 500 holds [945, 955) and gets 40 rows at 900 .. 939: one tile session
    at entry 1000 of M (500 sessions and 500 rows of the keys below come first), whose dead slots run
    to entry 1039, and the held session at entry 1040 joins it across the chunk boundary 1023 / 1024."""
    sk = np.arange(1000)
    seed = Push(kind, sk, np.where(sk == SPAN_KEY, 945, 1000), seed=2)
    k, ts, g = list(range(SPAN_KEY)), [1002] * SPAN_KEY, [(1, 3, G)[q % 3] for q in range(SPAN_KEY)]
    k += [SPAN_KEY] * 40
    ts += list(range(900, 940))
    g += [G] * 40
    n_join = TILE - SPAN_KEY - 40 - n_new
    k += list(range(SPAN_KEY + 1, SPAN_KEY + 1 + n_join))
    ts += [1002] * n_join
    g += [(1, 3, G)[q % 3] for q in range(n_join)]
    for j in range(n_new):
        k.append(2000 + j if j % 2 == 0 else 600 + j)
        ts.append(1000 if j % 2 == 0 else 5000)
        g.append(G)
    tile = Push(kind, k, ts, g, seed=20 + n_new).shuffled(n_new)
    return {"cap_s": 1024, "seed": seed, "tile": tile, "held": 1000, "final": 1000 + n_new, "drops": n_new > 24,
            "state": [(int(q), 945 if q == SPAN_KEY else 1000) for q in sk]}


# ---- case 3: a dropped tile in the middle of a push -------------------------------------------------------
def case3(kind):
    """cap_s = 64, 40 held sessions; one push of three full tiles: tile 0 opens 10 sessions (50: fits),
    tile 1 opens 30 (80: dropped), tile 2 only joins held sessions, those of tile 0 among them"""
    rng = np.random.default_rng(3)
    held = np.arange(30)

    def tile(n_new, first_new, keys, seed):
        k, ts, g = _joiners(rng, TILE - n_new, keys)
        k += list(range(first_new, first_new + n_new))
        ts += [1000] * n_new
        g += [G] * n_new
        return Push(kind, k, ts, g, seed=seed).shuffled(seed)
    tiles = [tile(10, 200, held, 31), tile(30, 300, held, 32), tile(0, 0, np.concatenate([held, np.arange(200, 210)]), 33)]
    return {"cap_s": 64, "seed": seed40(kind), "held": 40, "push": concat(tiles), "without_tile_1": concat([tiles[0], tiles[2]]),
            "tiles": [(False, 50), (True, 50), (False, 50)]}


# ---- case 4: late rows in a tile that is then dropped -----------------------------------------------------
def case4(kind, over):
    """cap_s = 64, 40 held sessions, watermark 1005 (a row with ts + gap - 1 <= 1005 is a late candidate).
    One tile in arrival order: keys 0 .. 9 get 995 then 985 (anchored by [1000, 1015), then by the grown
    session: kept); keys 10 .. 19 get 985 then 995 (985 reaches nothing when it arrives: dropped; 995
    kept); keys 20 .. 24 get 900 (dropped); keys 25 .. 29 a row on time; then 24 (``over``: 25) new keys
    far ahead.  15 rows are late-dropped; the list ends at 64 (65: the tile is dropped)."""
    k, ts = [], []
    for q in range(10):
        k += [q, q]
        ts += [995, 985]
    for q in range(10, 20):
        k += [q, q]
        ts += [985, 995]
    for q in range(20, 25):
        k.append(q)
        ts.append(900)
    for q in range(25, 30):
        k.append(q)
        ts.append(1012)
    late = [i for i, (q, t) in enumerate(zip(k, ts)) if (10 <= q < 20 and t == 985) or t == 900]
    n_new = 25 if over else 24
    k += list(range(400, 400 + n_new))
    ts += [5000] * n_new
    return {"cap_s": 64, "seed": seed40(kind), "held": 40, "watermark": 1005, "tile": Push(kind, k, ts, seed=40 + n_new), "late": late,
            "final": 40 + n_new, "drops": over}


# ---- case 5: lists longer than one tile (static) -------------------------------------------------------------
def case5():
    """cap_s = 2048.  1500 sessions (keys 0 .. 1499, sorted by key in the list); those with key % 15 < 7
    (700, interleaved) start at 0, the others at 1000.  A tile of 1024 joining rows (L = 2524: three
    chunks, and 1500 + its tile sessions > 2048, so pass 0 runs and the tile fits); watermark 500 fires
    the 700, and the 800 kept -- 544 of them in chunk 0, 256 in chunk 1 -- close up; a full tile of 824
    joining rows and 200 new keys (L = 1824); the final watermark."""
    kind, rng = "static", np.random.default_rng(5)
    keys = np.arange(1500)
    start = np.where(keys % 15 < 7, 0, 1000)
    a = Push(kind, keys, start, seed=51)
    jk = rng.integers(0, 1500, TILE)
    b = Push(kind, jk, start[jk] + rng.integers(0, 6, TILE), seed=52)
    kept = keys[keys % 15 >= 7]
    ck = rng.choice(kept, 824)
    c = Push(kind, np.concatenate([ck, np.arange(5000, 5200)]),
             np.concatenate([1000 + rng.integers(0, 9, 824), np.full(200, 1000)]), seed=53).shuffled(5)
    return {"cap_s": 2048, "steps": [("push", a), ("push", b), ("wm", 500), ("push", c), ("wm", LONG_MAX)],
            "live": [1500, 1500, 800, 1000, 0], "fires": [700, 1000], "kept": kept}


# ---- case 6: output capacity (sessions) ------------------------------------------------------------------------
OUT_CAP = 64


def case6(kind):
    """output_capacity = 64, LONG / BIGINT keys over many superbuckets: 64 sessions at 0, 30 at 1000 and
    35 at 1100.  Watermark 500 fires exactly 64; watermark 5000 would fire 65 -- or 30 and 35 when 1050
    comes between."""
    ka = np.arange(64) * 7919 + 1
    kb = np.arange(65) * 104729 + 5
    a = Push(kind, np.repeat(ka, 3), np.tile([0, 3, 5], 64), seed=61).shuffled(61)
    b = Push(kind, np.repeat(kb, 2), np.repeat(np.where(np.arange(65) < 30, 1000, 1100), 2) + np.tile([0, 4], 65),
             seed=62).shuffled(62)
    return {"pushes": [a, b], "first": 500, "over": 5000, "split": [1050, 5000], "fires": [64, 65, 30, 35]}


# ---- case 7: late side capacity ------------------------------------------------------------------------------------
def case7(n):
    """max_batch_rows = 1024, so the side output holds 2048 rows.  Under watermark 10000 and no state,
    ``n`` (2048, 2049) rows of 32 keys at ts < 5000, every one late and alone, in pushes of 1024"""
    rng = np.random.default_rng(7)
    pushes = []
    for a in range(0, n, TILE):
        m = min(TILE, n - a)
        pushes.append(Push("static", rng.integers(0, 32, m), rng.integers(0, 5000, m), seed=70 + a))
    return {"watermark": 10000, "pushes": pushes, "side_cap": 2048, "n": n,
            "after": Push("static", [1, 2, 3], [10, 20, 30], seed=79)}


# ---- the count table ---------------------------------------------------------------------------------------------
COUNT_PAIRS = [(4, 2), (5, 1), (250, 150)]
CAP_E = 64


def _count_push(rng, keys, per):
    """``per`` rows of every key, shuffled: (keys, values)"""
    k = np.repeat(_i64(keys), per)[rng.permutation(len(keys) * per)]
    return k, rng.integers(-10**6, 10**6, len(k)).astype(np.int64)


def case8(size, slide):
    """cap_e = 64: 64 keys in two pushes (slide + 1, then slide rows each: every key fires in both);
    a third push with slide rows of every held key and slide + 2 rows of a 65th and a 66th key; a
    fourth with slide rows of every held key"""
    rng = np.random.default_rng(8)
    held = np.arange(64) * 11 + 3
    extra = _i64([9001, 9002])
    p3k = np.concatenate([np.repeat(held, slide), np.repeat(extra, slide + 2)])
    p3k = p3k[rng.permutation(len(p3k))]
    return {"held": held, "extra": extra,
            "pushes": [_count_push(rng, held, slide + 1), _count_push(rng, held, slide),
                       (p3k, rng.integers(-10**6, 10**6, len(p3k)).astype(np.int64)), _count_push(rng, held, slide)]}


def case9(size, slide):
    """cap_e = 64: 54 keys held with 2 slide - 3 rows each; one tile of 5 rows of every held key (each
    fires) and 8 rows of 40 new keys, of which 10 find a slot; then slide rows of all 94 keys, from which
    the test takes the rows of the keys the table holds"""
    rng = np.random.default_rng(9)
    held = np.arange(54) * 13 + 7
    new = np.arange(40) * 17 + 5000
    rk = np.concatenate([np.repeat(held, 5), np.repeat(new, 8)])
    rk = rk[rng.permutation(len(rk))]
    return {"held": held, "new": new, "room": CAP_E - 54,
            "pushes": [_count_push(rng, held, max(2 * slide - 3, 1)), (rk, rng.integers(-10**6, 10**6, len(rk)).astype(np.int64)),
                       _count_push(rng, np.concatenate([held, new]), slide)]}


def case10(size, slide):
    """output_capacity = 64, LONG keys over many superbuckets: slide rows of 64 keys (64 fires), then slide
    rows of those and a 65th (65 fires), which split behind row ``cut`` fires 32 and 33"""
    rng = np.random.default_rng(10)
    keys = np.arange(65) * 7919 + 1
    first = _count_push(rng, keys[:64], slide)
    k2 = np.concatenate([np.repeat(keys[:32], slide)[rng.permutation(32 * slide)],
                         np.repeat(keys[32:], slide)[rng.permutation(33 * slide)]])
    return {"pushes": [first, (k2, rng.integers(-10**6, 10**6, len(k2)).astype(np.int64))], "cut": 32 * slide, "fires": [64, 65, 32, 33]}


def count_reference_rows(size, slide, agg, pushes):
    """CountWindowReference over the pushes: per push the rows (key, value, window_start, window_end,
    push_seq << 32 | row) in emission order"""
    ref = CountWindowReference(size, slide, agg)
    out, base = [], 0
    for seq, (k, v) in enumerate(pushes):
        rows = ref.process(_i64(k).tolist(), _i64(v).tolist())
        out.append([(kk, vv, ws, we, (seq << 32) | (at - base)) for kk, vv, ws, we, at in rows])
        base += len(k)
    return out
