"""GPU parity of k_ingest_pack's two geometries (fw_ingest_pack.h: 512 threads x 8 rows and 256 x 16).

Every case runs in fresh operators with FW_IG_PACK=2 under FW_IGP_GEOM=0 and =1.  A first push and a
watermark that fires a window (a flush) come first, so the case's pushes open a flush epoch with valid
PF_PACK fields and are packed.  Each watermark's rows are bit-exact against the oracle in both
geometries, the two agree with each other in rows and in the fw_stats counters, every push is a
k_ingest_pack launch, and compact_chunks shows which chunks took the packing path.  Keys are distinct
within a push, so nothing folds and the counters are comparable.

The cases run the KH_BINROW_BIGINT instances (the benchmark's); test_hash_kinds runs the other three
kinds, and test_geometry_is_chosen_per_launch the host's choice when FW_IGP_GEOM is not set."""
import os
import re

import numpy as np
import pytest

from flink_amd import _native, abi
from parity_common import I64, _cfg, _compare, _rows

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000_000
CH = 4096
SIZE = 5000               # TUMBLE size = slice (ms)
STEP, OOO = 5000, 4000    # every watermark fires a window, so every watermark flushes
WARM = 3000               # rows of the first push
COUNTERS = ("num_late_records_dropped", "partials_emitted", "partial_bytes_written", "compact_chunks")
GEOMS = {"0": (0, 512, 8), "1": (1, 256, 16)}
POOL = np.arange(40000, dtype=np.int64) * 104729 + 11
PLANS = {128: {}, 1024: dict(state_capacity=2_000_000)}  # superbuckets of the plan: extra configuration
POOL32 = np.arange(40000, dtype=np.int64) * 7919 + 11  # keys the INT hash kinds hold
KW = dict(window_kind=abi.WIN_TUMBLE, size_ms=SIZE, aggs=[(abi.AGG_SUM, 0, I64)], max_batch_rows=1 << 14,
          key_hash=abi.KEYHASH_BINROW_BIGINT)


def _wm(b):
    return T0 + (b + 1) * STEP - OOO - 1


def _push(rng, n, b, pool=POOL):
    """n on-time rows of step b, keys distinct."""
    ts = T0 + b * STEP + rng.integers(0, STEP, n) - rng.integers(0, OOO, n)
    return rng.permutation(pool)[:n].astype(np.int64), ts.astype(np.int64), rng.integers(-10**6, 10**6, n).astype(np.int64)


def _warm(rng, pool=POOL):
    """The first push: its key and value ranges are the pool's, so the next epoch's fields hold every row."""
    k, t, v = _push(rng, WARM, 0, pool)
    k[:2] = pool.min(), pool.max()
    v[:2] = -10**6, 10**6 - 1
    return k, t, v


def _run(monkeypatch, pushes, n_sb=128, pool=POOL, seed=0, key_hash=None):
    """Step 0: the first push and its watermark; step 1: `pushes` and their watermark; step 2: a watermark
    that fires everything.  Returns the counters of geometry 1 (equal to geometry 0's) less step 0's."""
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    monkeypatch.setenv("FW_IG_PACK", "2")
    steps = [([_warm(np.random.default_rng(1000 + seed), pool)], _wm(0)), (pushes, _wm(1)), ([], _wm(10))]
    out = {}
    for geom, shape in GEOMS.items():
        monkeypatch.setenv("FW_IGP_GEOM", geom)
        cfg = _cfg(KW, **PLANS[n_sb], **({} if key_hash is None else dict(key_hash=key_hash)))
        o, g = OracleOperator(cfg), WindowAggHandle(cfg)
        assert g.ingest_pack_geometry() == shape
        rows, st0 = [], None
        for si, (ps, wm) in enumerate(steps):
            for k, t, v in ps:
                vals = [v, np.zeros(len(k)).view(np.int64)]
                o.process_batch(k, t, vals, None)
                g.push_host(k, t, vals)
            o.process_watermark(wm)
            g.advance(wm)
            got, want = _rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set())
            _compare(got, want, set(), f"geometry {geom} step {si}")
            rows += got
            if si == 0:
                st0 = g.stats()
        st = g.stats()
        assert st["error_flags"] == 0 and st["num_late_records_dropped"] == o.late_dropped
        assert st["num_superbuckets"] == n_sb
        assert g.ingest_pack_launches() == 1 + len(pushes)  # the kernel ran, on every push
        assert st0["compact_chunks"] == 0                   # (the first epoch cannot pack)
        g.close()
        out[geom] = (rows, {c: st[c] - st0[c] for c in COUNTERS})
    assert len(out["0"][0]) > 0 and out["0"][0] == out["1"][0]
    assert out["0"][1] == out["1"][1], (out["0"][1], out["1"][1])
    return out["1"][1]


def _chunks(n):
    return -(-n // CH)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 300])
def test_row_counts_around_the_thread_and_chunk_edges(monkeypatch, n):
    """Two pushes of n rows (slot 0 and a later slot).  In the last size the partial chunk's clamped row
    index is reached from j * 256 + tid with j up to 15."""
    rng = np.random.default_rng(n)
    st = _run(monkeypatch, [_push(rng, n, 1), _push(rng, n, 1)], seed=n)
    assert st["compact_chunks"] == 2 * _chunks(n), st
    assert st["partials_emitted"] == 2 * n and st["num_late_records_dropped"] == 0, st


@pytest.mark.parametrize("n", [257, 4097, 2 * 4096 + 300])
def test_1024_superbuckets(monkeypatch, n):
    """The largest plan: each thread of the 256-thread geometry claims four sub-runs."""
    rng = np.random.default_rng(7 * n)
    st = _run(monkeypatch, [_push(rng, n, 1), _push(rng, n, 1)], n_sb=1024, seed=n)
    assert st["compact_chunks"] == 2 * _chunks(n), st
    assert st["partials_emitted"] == 2 * n, st


@pytest.mark.parametrize("n", [257, 2 * 4096 + 300])
@pytest.mark.parametrize("kind", ["LONG", "INT", "BINROW_INT"])
def test_hash_kinds(monkeypatch, kind, n):
    """The instances of the other key-hash kinds, in both geometries."""
    rng = np.random.default_rng(n + len(kind))
    st = _run(monkeypatch, [_push(rng, n, 1, POOL32), _push(rng, n, 1, POOL32)], pool=POOL32, seed=n,
              key_hash=getattr(abi, "KEYHASH_" + kind))
    assert st["compact_chunks"] == 2 * _chunks(n) and st["partials_emitted"] == 2 * n, st


def _stage_rows(n_sb):
    """igp_stage_rows (fw_internal.h), restated from the header's constants."""
    text = open(os.path.join(os.path.dirname(__file__), "..", "flink_amd", "csrc", "fw_internal.h")).read()
    a, b = re.search(r"constexpr int IGP_LDS = (\d+) \* (\d+);", text).groups()
    hdr = int(re.search(r"constexpr int IG_HDR_WORDS = (\d+);", text).group(1))
    hist_words = ((n_sb + 7) >> 3) << 1
    fixed = 8 * (hdr + hist_words) + 6 * ((n_sb + 7) & ~7)
    return ((int(a) * int(b) - fixed) // 12) & ~15


@pytest.mark.parametrize("more", [0, 1])
@pytest.mark.parametrize("n_sb", sorted(PLANS))
def test_store_windows(monkeypatch, n_sb, more):
    """One chunk whose partials fill the store stage exactly (one window), and one more (two); the
    chunk's other rows are late."""
    w = _stage_rows(n_sb) + more
    assert 2048 <= w - more and w < CH
    rng = np.random.default_rng(n_sb + more)
    k, t, v = _push(rng, CH, 1)
    late = rng.permutation(CH)[:CH - w]
    t[late] = _wm(0) - SIZE - rng.integers(0, 2 * SIZE, CH - w)
    st = _run(monkeypatch, [(k, t, v)], n_sb=n_sb, seed=w)
    assert st["partials_emitted"] == w and st["num_late_records_dropped"] == CH - w, st
    assert st["compact_chunks"] == 1, st


def test_sub_run_overflow(monkeypatch):
    """Every key lives in 8 of the 128 superbuckets, ~512 rows per (chunk, superbucket): the stretches
    exceed the sub-runs, the rest stays in the chunks' regions (RUN_LOCAL) behind the overflow flags.
    A sub-run holds 5/4 of a uniform share of a full push + 16 rows, rounded up to 16 (fw_api.hip): 48
    rows here, so the first chunk of a sub-run already overflows it."""
    n = 3 * CH + 5
    subs = 128 * 8  # superbuckets x RUN_X
    sub_cap = ((KW["max_batch_rows"] * 5 // 4 + subs - 1) // subs + 16 + 15) // 16 * 16
    assert sub_cap == 48 and CH // 8 > 4 * sub_cap
    cand = np.arange(1, 400000, dtype=np.int64)
    kg = np.zeros(len(cand), dtype=np.int32)
    rc = _native.lib().fw_host_assign_key_groups(cand.ctypes.data, None, len(cand), KW["key_hash"], 128, 1,
                                                 kg.ctypes.data, None)
    assert rc == 0
    pool = cand[kg < 8][:n]
    assert len(pool) == n
    rng = np.random.default_rng(8)
    st = _run(monkeypatch, [_push(rng, n, 1, pool), _push(rng, n, 1, pool)], pool=pool, seed=8)
    assert st["compact_chunks"] == 2 * 4 and st["partials_emitted"] == 2 * n, st


def test_slow_chunk_inside_a_packed_push(monkeypatch):
    """A key 2^40 above the epoch's key field in the middle chunk of three: that chunk is PF_WIDE."""
    rng = np.random.default_rng(9)
    k, t, v = _push(rng, 3 * CH, 1)
    k[CH + 100] += np.int64(1) << 40
    st = _run(monkeypatch, [(k, t, v)], seed=9)
    assert st["compact_chunks"] == 2 and st["partials_emitted"] == 3 * CH, st


def test_late_rows_are_dropped_and_counted(monkeypatch):
    """40 rows of the second chunk lie in a window the first watermark fired."""
    rng = np.random.default_rng(10)
    k, t, v = _push(rng, 2 * CH + 300, 1)
    i = CH + rng.permutation(CH)[:40]
    t[i] = _wm(0) - SIZE - rng.integers(0, 2 * SIZE, 40)
    st = _run(monkeypatch, [(k, t, v)], seed=10)
    assert st["num_late_records_dropped"] == 40 and st["partials_emitted"] == 2 * CH + 260, st
    assert st["compact_chunks"] == 3, st  # late rows do not make their chunk slow


def test_geometry_is_chosen_per_launch(monkeypatch):
    """FW_IGP_GEOM not set: a push takes 256 x 16 when that makes it resident as a whole and 512 x 8 does
    not, i.e. with more chunks than 512 x 8's workgroups per CU x CUs and at most 256 x 16's, and only
    for the hash kinds whose 256 x 16 instance spills no VGPR.  Pushes just below that interval, just
    inside it and just above it (the sizes at which the choice changes; the only large pushes of this
    file), each followed by the geometry the handle reports, then oracle parity of the rows.  A
    KH_LONG handle keeps 512 x 8 inside the interval."""
    import torch
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    monkeypatch.setenv("FW_IG_PACK", "2")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    occ = []
    for geom in ("0", "1"):
        monkeypatch.setenv("FW_IGP_GEOM", geom)
        h = WindowAggHandle(_cfg(KW))
        occ.append(h.ingest_pack_geometry(occupancy=True)[3])
        h.close()
    monkeypatch.delenv("FW_IGP_GEOM")
    res0, res1 = occ[0] * cus, occ[1] * cus
    assert 0 < res0 < res1
    edges = [(res0 * CH, 0), (res0 * CH + 1, 1), (res1 * CH + 1, 0)]
    rng = np.random.default_rng(77)

    def rows(n, b):
        ts = T0 + b * STEP + rng.integers(0, STEP, n) - rng.integers(0, OOO, n)
        return POOL[rng.integers(0, len(POOL), n)], ts.astype(np.int64), rng.integers(-10**6, 10**6, n).astype(np.int64)

    for kind, sizes in (("BINROW_BIGINT", edges), ("LONG", [(res0 * CH + 1, 0)])):
        expect = [e for _, e in sizes]
        cfg = _cfg(KW, key_hash=getattr(abi, "KEYHASH_" + kind), max_batch_rows=(res1 + 1) * CH)
        o, g = OracleOperator(cfg), WindowAggHandle(cfg)
        assert g.ingest_pack_geometry()[0] == 0
        steps = [([_warm(rng)], _wm(0))] + [([rows(n, 1 + i)], _wm(1 + i)) for i, (n, _) in enumerate(sizes)] + [([], _wm(10))]
        taken = []
        for si, (ps, wm) in enumerate(steps):
            for k, t, v in ps:
                vals = [v, np.zeros(len(k)).view(np.int64)]
                o.process_batch(k, t, vals, None)
                g.push_host(k, t, vals)
                taken.append(g.ingest_pack_geometry()[0])
            o.process_watermark(wm)
            g.advance(wm)
            _compare(_rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"{kind} step {si}")
        st = g.stats()
        assert st["error_flags"] == 0 and st["num_late_records_dropped"] == o.late_dropped
        assert g.ingest_pack_launches() == 1 + len(sizes)
        g.close()
        assert taken == [0] + expect, (kind, taken)
        assert st["compact_chunks"] == sum(_chunks(n) for n, _ in sizes), st  # every large push was packed
