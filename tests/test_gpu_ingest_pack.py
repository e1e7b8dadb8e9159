"""GPU parity of the early-packing ingest kernel (k_ingest_pack, fw_ingest_pack.h).

SQL TUMBLE handles with one NOT NULL integer MAX / MIN / SUM write PF_PACK run rows; their pushes
that skip the LDS fold go to k_ingest_pack, which packs each row to its 8-B run word as soon as it
is routed and sends every chunk the word cannot hold (and every chunk of a launch that cannot pack
yet) through a rolled loop that writes PF_WIDE rows.  Every case runs with FW_IG_PACK=2 (every push
of an eligible handle) and FW_IG_PACK=0 (k_ingest only) in fresh operator instances: each
watermark's rows are bit-exact against the oracle in both, and the late / partial counters agree
between the two.  Keys are distinct within a push, so no push folds rows whichever kernel takes it
and the counters are comparable.  COUNT(*) alone keeps k_ingest (its pushes that cannot pack are
PF_UNIT / PF_NARROW, which k_ingest_pack does not write): it runs here as an ineligible layout.

Pushes are 3 chunks + 5 rows (a partial last chunk), 3 pushes per watermark, 6 watermarks."""
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
SIZE = 5000                # TUMBLE size = slice (ms)
STEP, OOO = 5000, 4000    # every watermark fires a window, so every watermark flushes: an epoch per watermark
CHUNKS = N_WM * SPLIT * 4  # chunks of a run
FIRST = SPLIT * 4          # chunks of the first flush epoch: no launch of it can pack (no PF_PACK fields yet)

AGGS = {
    "max": [(abi.AGG_MAX, 0, I64)],
    "min": [(abi.AGG_MIN, 0, I64)],
    "sum": [(abi.AGG_SUM, 0, I64)],
}
COUNTERS = ("num_late_records_dropped", "partials_emitted", "partial_bytes_written", "compact_chunks")


def _kw(name, **extra):
    return dict(window_kind=abi.WIN_TUMBLE, size_ms=SIZE, aggs=AGGS[name], **extra)


def _stream(seed, pool=None, n_wm=N_WM):
    """On-time batches of SPLIT pushes; keys: distinct within the batch (a permutation of the pool)."""
    rng = np.random.default_rng(seed)
    if pool is None:
        pool = np.arange(40000, dtype=np.int64) * 104729 + 11
    out = []
    for b in range(n_wm):
        base = T0 + b * STEP
        n = SPLIT * PUSH
        ts = base + rng.integers(0, STEP, n) - rng.integers(0, OOO, n)
        if len(pool) >= n:
            keys = rng.permutation(pool)[:n]
        else:  # a small pool: distinct within each push
            keys = np.concatenate([rng.permutation(pool)[:PUSH] for _ in range(SPLIT)])
        iv = rng.integers(-10**6, 10**6, n).astype(np.int64)
        out.append((keys.astype(np.int64), ts.astype(np.int64), iv, np.zeros(n), base + STEP - OOO - 1))
    return out


def _launches():
    return int(_native.lib().fw_ingest_pack_launches(None))


def _both_modes(monkeypatch, kw, batches, cfg_extra=None):
    """{mode: (stats, k_ingest_pack launches)} of FW_IG_PACK=2 and =0, each checked against the oracle."""
    out = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("FW_IG_PACK", mode)
        st, n0 = {}, _launches()
        _run_both(_cfg(kw, max_batch_rows=1 << 14, **(cfg_extra or {})), batches, set(), split=SPLIT, stats=st)
        out[mode] = (st, _launches() - n0)
    for c in COUNTERS:
        assert out["2"][0][c] == out["0"][0][c], (c, out["2"][0], out["0"][0])
    assert out["0"][1] == 0
    return out


@pytest.mark.parametrize("name", sorted(AGGS))
def test_on_time_pushes_are_packed(monkeypatch, name):
    """Case 1 (and 4: the pushes before the first watermark, the stream's first among them, cannot
    pack and go through the slow chunks).  Every push is taken, every chunk after them is packed."""
    out = _both_modes(monkeypatch, _kw(name), _stream(1))
    st, n = out["2"]
    assert n == N_WM * SPLIT
    assert st["compact_chunks"] == CHUNKS - FIRST, st
    assert st["num_late_records_dropped"] == 0


def test_default_mode_takes_the_pushes_that_skip_the_fold(monkeypatch):
    """FW_IG_PACK=1: the host follows the ingest mirror.  From the second watermark on (the results
    were read: the mirror is current) every push but the 8th and 16th, on which k_ingest folds
    again, is taken; the first watermark's pushes after the first may or may not see the mirror."""
    monkeypatch.setenv("FW_IG_PACK", "1")
    st, n0 = {}, _launches()
    _run_both(_cfg(_kw("max"), max_batch_rows=1 << 14), _stream(2), set(), split=SPLIT, stats=st)
    n = _launches() - n0
    steady = (N_WM - 1) * SPLIT - 2
    assert steady <= n <= steady + SPLIT - 1, n
    assert st["compact_chunks"] == CHUNKS - FIRST, st


def test_1024_superbuckets(monkeypatch):
    """The largest plan the kernel serves (two superbuckets per thread for the run claims)."""
    out = _both_modes(monkeypatch, _kw("max"), _stream(3), cfg_extra=dict(state_capacity=2_000_000))
    assert out["2"][1] == N_WM * SPLIT
    assert out["2"][0]["compact_chunks"] == CHUNKS - FIRST


def test_slow_chunks_inside_packed_pushes(monkeypatch):
    """Case 2.  The middle push of every watermark after the first has a row 300 slices ahead in its
    first chunk, a key 2^40 above the epoch's key field in its second and a value of 2^50 in its
    third: those chunks are PF_WIDE, the partial fourth and the other pushes' chunks are packed.
    (The watermark's last push measures ordinary ranges again for the next epoch.)"""
    batches = _stream(4)
    for b, (k, t, iv, dv, wm) in enumerate(batches):
        if b == 0:
            continue
        o = PUSH
        t[o + 17] = T0 + b * STEP + 300 * SIZE
        k[o + CH + 100] += np.int64(1) << 40
        iv[o + 2 * CH + 9] = np.int64(1) << 50
    out = _both_modes(monkeypatch, _kw("sum"), batches)
    st, n = out["2"]
    assert n == N_WM * SPLIT
    assert st["compact_chunks"] == CHUNKS - FIRST - 3 * (N_WM - 1), st


def test_late_rows_are_dropped_and_counted(monkeypatch):
    """Case 3.  40 rows of one chunk lie in windows the previous watermark fired."""
    batches = _stream(5)
    rng = np.random.default_rng(55)
    hit = 0
    for b, (k, t, iv, dv, wm) in enumerate(batches):
        if b in (2, 4):
            prev_wm = T0 + b * STEP - OOO - 1
            i = PUSH + CH + rng.permutation(CH)[:40]
            t[i] = prev_wm - SIZE - rng.integers(0, 2 * SIZE, 40)
            hit += 40
    out = _both_modes(monkeypatch, _kw("min"), batches)
    st, n = out["2"]
    assert st["num_late_records_dropped"] == hit
    assert st["compact_chunks"] == CHUNKS - FIRST, st  # late rows do not make their chunk slow


def test_sub_run_overflow(monkeypatch):
    """Case 6.  Every key lives in 32 of the 128 superbuckets, ~128 rows per (chunk, superbucket):
    stretches exceed the sub-runs, the rest stays in the chunks' regions behind the overflow flags."""
    cand = np.arange(1, 60000, dtype=np.int64)
    kg = np.zeros(len(cand), dtype=np.int32)
    rc = _native.lib().fw_host_assign_key_groups(cand.ctypes.data, None, len(cand), abi.KEYHASH_LONG, 128, 1,
                                                 kg.ctypes.data, None)
    assert rc == 0
    pool = cand[kg < 32][:PUSH]
    assert len(pool) == PUSH
    out = _both_modes(monkeypatch, _kw("max"), _stream(6, pool=pool))
    assert out["2"][1] == N_WM * SPLIT
    assert out["2"][0]["compact_chunks"] == CHUNKS - FIRST


def _run_steps(cfg, batches, init_wm=None):
    """parity_common._run_both's loop with the k_ingest_pack launches after every watermark."""
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    o, g = OracleOperator(cfg), WindowAggHandle(cfg)
    if init_wm is not None:
        o.initialize_watermark(init_wm)
        g.initialize_watermark(init_wm)
    taken = []
    for bi, (k, t, iv, dv, wm) in enumerate(batches):
        vals = [iv, dv.view(np.int64)]
        o.process_batch(k, t, vals, None)
        for part in np.array_split(np.arange(len(k)), SPLIT):
            g.push_host(k[part], t[part], [v[part] for v in vals])
        o.process_watermark(wm)
        g.advance(wm)
        _compare(_rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"batch {bi}")
        taken.append(g.ingest_pack_launches())
    st = g.stats()
    assert st["num_late_records_dropped"] == o.late_dropped and st["error_flags"] == 0
    g.close()
    return st, taken


def test_first_push_with_an_initialised_watermark(monkeypatch):
    """Case 4.  fw_initialize_watermark was called: the stream's first push has a watermark but no
    PF_PACK fields yet, nor have the others of its flush epoch: slow chunks; the next epoch packs."""
    batches = _stream(7, n_wm=3)
    outs = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("FW_IG_PACK", mode)
        outs[mode] = _run_steps(_cfg(_kw("max"), max_batch_rows=1 << 14), batches, init_wm=T0 - OOO - 1)
    for c in COUNTERS:
        assert outs["2"][0][c] == outs["0"][0][c], c
    assert outs["2"][1] == [3, 6, 9] and outs["0"][1] == [0, 0, 0]
    assert outs["2"][0]["compact_chunks"] == 3 * SPLIT * 4 - FIRST


def test_skew_is_noticed(monkeypatch):
    """Case 5 (FW_IG_PACK=1).  Three uniform watermarks, then half of every push's rows carry one
    key.  k_ingest takes the 16th push (push_count & 7 == 0), folds, clears fold_skip, and from the
    next watermark on (the mirror is read after the results) no push goes to k_ingest_pack."""
    monkeypatch.setenv("FW_IG_PACK", "1")
    batches = _stream(8, n_wm=8)
    for b in range(3, 8):
        k = batches[b][0]
        k[::2] = k[0]
    st, taken = _run_steps(_cfg(_kw("sum"), max_batch_rows=1 << 14), batches)
    assert taken[2] >= 2 * SPLIT - 1          # uniform: taken (pushes 3..8 but the 8th)
    assert taken[5] > taken[2]                # still taken while the skew is unnoticed (pushes 9..15)
    assert taken[7] == taken[6] == taken[5]   # push 16 (watermark 5's second) folded: none after watermark 5


@pytest.mark.parametrize("name", ["hop", "nullable", "precomputed_hash", "count_star"])
def test_ineligible_handles_keep_k_ingest(monkeypatch, name):
    """Case 7.  HOP, a nullable column, a precomputed key hash and COUNT(*) alone never launch it."""
    monkeypatch.setenv("FW_IG_PACK", "2")
    batches = _stream(9, n_wm=3)
    kw, nulls, extra = _kw("max"), None, {}
    if name == "hop":
        kw = dict(window_kind=abi.WIN_HOP, size_ms=10000, slide_ms=5000, count_star_index=0,
                  aggs=[(abi.AGG_COUNT_STAR, 0, I64), (abi.AGG_MAX, 0, I64)])  # (SQL HOP needs its COUNT(*))
    elif name == "nullable":
        extra = dict(nullable_cols=(0,))
        nulls = [{0: (np.arange(len(b[0])) % 97 == 0).astype(np.uint8)} for b in batches]
    elif name == "count_star":
        kw = dict(window_kind=abi.WIN_TUMBLE, size_ms=SIZE, count_star_index=0, aggs=[(abi.AGG_COUNT_STAR, 0, I64)])
    n0 = _launches()
    if name == "precomputed_hash":
        from flink_amd.runtime.handle import WindowAggHandle
        from oracle.oracle import OracleOperator
        cfg = _cfg(kw, max_batch_rows=1 << 14, key_hash=abi.KEYHASH_PRECOMPUTED)
        o, g = OracleOperator(cfg), WindowAggHandle(cfg)
        for bi, (k, t, iv, dv, wm) in enumerate(batches):
            vals = [iv, dv.view(np.int64)]
            kh = (k ^ (k >> 32)).astype(np.int32)
            o.process_batch(k, t, vals, None)  # (the hash only routes)
            for part in np.array_split(np.arange(len(k)), SPLIT):
                g.push_host(k[part], t[part], [v[part] for v in vals], key_hashes=kh[part])
            o.process_watermark(wm)
            g.advance(wm)
            _compare(_rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"batch {bi}")
        g.close()
    else:
        _run_both(_cfg(kw, max_batch_rows=1 << 14, **extra), batches, set(), split=SPLIT, nulls=nulls)
    assert _launches() == n0
