"""GPU tests of the ingest-kernel policy and of k_ingest_pack's slim per-row code (fw_ingest_pack.h, fw_api.hip).

The shapes are those of test_gpu_ingest_pack.py: pushes of 3 chunks + 5 rows, 3 pushes per watermark,
TUMBLE 5 s, max_batch_rows = 1 << 14, every watermark fires a window and so flushes (an epoch per
watermark).  Every watermark's rows are bit-exact against the oracle.

The policy (fw_host_ig_pack_choice; test_ingest_policy_host.py has its table): in the default mode a
push of an eligible handle goes to k_ingest_pack unless the ingest mirror lacks the fold-skip or the
PF_PACK bit, no merge has been launched yet (the pushes of the first flush epoch: no PF_PACK fields
exist, the packing kernel would send every chunk its slow way), or a fold measurement is due: 64
pushes after the last push on which k_ingest folded, 8 while the packing kernel's own sampled
estimate of the fold's yield (one row in eight through a 1024-tag table, Ctrl::ig_skew, mirror bit
4) reaches k_ingest's 2 %.  That push tells k_ingest to fold whatever its push count is.  (Until
this rule k_ingest kept every 8th push of such a handle, and a one-thread report launch followed
each.)"""
import numpy as np
import pytest

from flink_amd import _native, abi
from parity_common import I64, _cfg, _compare, _rows

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000_000
CH = 4096
PUSH = 3 * CH + 5
SPLIT = 3
SIZE = 5000
STEP, OOO = 5000, 4000
COUNTERS = ("num_late_records_dropped", "partials_emitted", "partial_bytes_written", "compact_chunks")
POOL = np.arange(40000, dtype=np.int64) * 104729 + 11


def _kw(agg=abi.AGG_MAX, **extra):
    return dict(window_kind=abi.WIN_TUMBLE, size_ms=SIZE, aggs=[(agg, 0, I64)], **extra)


def _batch(rng, b, keys, vals=None):
    n = len(keys)
    base = T0 + b * STEP
    ts = base + rng.integers(0, STEP, n) - rng.integers(0, OOO, n)
    iv = rng.integers(-10**6, 10**6, n).astype(np.int64) if vals is None else vals
    return [keys.astype(np.int64), ts.astype(np.int64), iv, np.zeros(n), base + STEP - OOO - 1]


def _distinct(rng, pool=POOL):
    """Keys of one watermark's pushes, distinct within every push (within the watermark when the pool allows)."""
    if len(pool) >= SPLIT * PUSH:
        return rng.permutation(pool)[:SPLIT * PUSH]
    return np.concatenate([rng.permutation(pool)[:PUSH] for _ in range(SPLIT)])


def _run(cfg, batches, flags=0):
    """Oracle and GPU side by side; returns the final stats and the handle's k_ingest_pack launch
    count after every push.  `flags`: the error flags the run must end with."""
    from flink_amd.runtime.handle import WindowAggHandle
    from oracle.oracle import OracleOperator
    o, g = OracleOperator(cfg), WindowAggHandle(cfg)
    taken = []
    for bi, (k, t, iv, dv, wm) in enumerate(batches):
        vals = [iv, dv.view(np.int64)]
        o.process_batch(k, t, vals, None)
        for part in np.array_split(np.arange(len(k)), SPLIT):
            g.push_host(k[part], t[part], [v[part] for v in vals])
            taken.append(g.ingest_pack_launches())
        o.process_watermark(wm)
        g.advance(wm)
        _compare(_rows(g.results(reset=True), cfg, set()), _rows(o.results(clear=True), cfg, set()), set(), f"batch {bi}")
    st = g.stats()
    assert st["num_late_records_dropped"] == o.late_dropped
    assert st["error_flags"] == flags, st["error_flags"]
    g.close()
    return st, taken


def _modes(monkeypatch, cfg_of, batches, modes=("2", "0"), flags=0):
    """{mode: (stats, launches per push)}; the COUNTERS and the error flags agree between the modes."""
    out = {}
    for mode in modes:
        monkeypatch.setenv("FW_IG_PACK", mode)
        out[mode] = _run(cfg_of(), [list(b) for b in batches], flags=flags)
    first = out[modes[0]][0]
    for mode in modes[1:]:
        for c in COUNTERS + ("error_flags",):
            assert out[mode][0][c] == first[c], (c, mode, out[mode][0][c], first[c])
    return out


# ---------------------------------------------------------------------------------------------------
# steady state
# ---------------------------------------------------------------------------------------------------
def test_steady_state_packs_all_but_one_push_in_64(monkeypatch):
    """24 watermarks (72 pushes) of distinct keys, default mode.  k_ingest takes the three pushes of
    the first flush epoch and exactly one later push, the 64th after the first (on which it folds
    and measures again): 68 launches of k_ingest_pack.  The chunks of the first epoch are PF_WIDE
    whichever kernel writes them; every other chunk is compact, the ones of the push k_ingest folds on
    included (it writes PF_PACK rows too), so compact_chunks equals that of a FW_IG_PACK=2 run."""
    n_wm = 24
    rng = np.random.default_rng(21)
    batches = [_batch(rng, b, _distinct(rng)) for b in range(n_wm)]
    out = _modes(monkeypatch, lambda: _cfg(_kw(), max_batch_rows=1 << 14), batches, modes=("1", "2"))
    taken = np.array(out["1"][1])
    assert taken[-1] == 68, taken
    k_ingest = [i for i in range(72) if taken[i] == (taken[i - 1] if i else 0)]
    assert k_ingest == [0, 1, 2, 64], k_ingest
    assert out["2"][1][-1] == 72
    assert out["1"][0]["compact_chunks"] == out["2"][0]["compact_chunks"] == (n_wm - 1) * SPLIT * 4


# ---------------------------------------------------------------------------------------------------
# skew
# ---------------------------------------------------------------------------------------------------
def _paired_keys(rng):
    """Every full chunk holds each of 2048 keys twice, spread over all superbuckets (no superbucket's
    count tells: the histogram of such a chunk looks like a uniform one's)."""
    out = []
    for _ in range(SPLIT):
        for _c in range(3):
            k = rng.permutation(POOL)[:CH // 2]
            out.append(rng.permutation(np.concatenate([k, k])))
        out.append(rng.permutation(POOL)[:5])
    return np.concatenate(out)


def _hot_keys(rng):
    k = _distinct(rng).copy()
    k[::2] = k[0]
    return k


def _skew_then_uniform(monkeypatch, skewed, agg):
    """3 uniform watermarks, 6 skewed ones, 4 uniform ones (default mode)."""
    monkeypatch.setenv("FW_IG_PACK", "1")
    rng = np.random.default_rng(31)
    batches = []
    for b in range(13):
        keys = skewed(rng) if 3 <= b < 9 else _distinct(rng)
        bt = _batch(rng, b, keys)
        if 3 <= b < 9:  # both copies of a key in one slice: one timestamp per key and watermark
            _, inv = np.unique(keys, return_inverse=True)
            bt[1] = (T0 + b * STEP + (inv * 7919) % STEP).astype(np.int64)
        batches.append(bt)
    st, taken = _run(_cfg(_kw(agg), max_batch_rows=1 << 14), batches)
    taken = np.array(taken)
    first_skewed = 3 * SPLIT
    # uniform: everything after the first epoch packs
    assert taken[first_skewed - 1] == first_skewed - SPLIT, taken
    # the skew is noticed: within 8 + 3 pushes no push packs any more, up to the end of the skewed part
    stop = first_skewed + 8 + 3
    assert taken[9 * SPLIT - 1] == taken[stop - 1], taken
    assert taken[stop - 1] < stop - SPLIT  # ... and k_ingest did take pushes before that
    # distinct again: k_ingest measures a fold without yield, packing resumes within two watermarks
    resumed = taken[(9 + 2) * SPLIT:] - taken[(9 + 2) * SPLIT - 1:-1]
    assert resumed.all(), taken
    return st


def test_skew_the_histogram_cannot_see(monkeypatch):
    _skew_then_uniform(monkeypatch, _paired_keys, abi.AGG_SUM)


def test_one_hot_key(monkeypatch):
    """Half of every push's rows carry one key."""
    _skew_then_uniform(monkeypatch, _hot_keys, abi.AGG_SUM)


# ---------------------------------------------------------------------------------------------------
# the key's high word
# ---------------------------------------------------------------------------------------------------
KEY_POOLS = {
    "straddle_2_32": (1 << 32) - 20000 + np.arange(40000, dtype=np.int64),
    "above_2_33": (1 << 33) + 12345 + np.arange(40000, dtype=np.int64) * 3,
    "negative": -(1 << 34) - np.arange(40000, dtype=np.int64) * 5,
}
HASHES = {"binrow_bigint": abi.KEYHASH_BINROW_BIGINT, "long": abi.KEYHASH_LONG}


@pytest.mark.parametrize("hash_kind", sorted(HASHES))
@pytest.mark.parametrize("pool", sorted(KEY_POOLS))
def test_key_high_word(monkeypatch, pool, hash_kind):
    """Keys whose high word differs inside an epoch's key field, is large, or is all ones: the packing
    kernel routes them as k_ingest does (same rows, counters and error flags)."""
    rng = np.random.default_rng(41)
    batches = [_batch(rng, b, _distinct(rng, KEY_POOLS[pool])) for b in range(4)]
    out = _modes(monkeypatch, lambda: _cfg(_kw(), max_batch_rows=1 << 14, key_hash=HASHES[hash_kind]), batches)
    assert out["2"][1][-1] == 4 * SPLIT and out["0"][1][-1] == 0
    assert out["2"][0]["compact_chunks"] == 3 * SPLIT * 4


def _own_keys(hash_kind, parallelism, subtask, cand):
    dest = np.zeros(len(cand), dtype=np.int32)
    rc = _native.lib().fw_host_assign_key_groups(cand.ctypes.data, None, len(cand), hash_kind, 128, parallelism, None,
                                                 dest.ctypes.data)
    assert rc == 0
    return cand[dest == subtask], cand[dest != subtask]


def _gpu_only(cfg, batches):
    """The handle alone (the oracle does not model subtasks): rows per watermark, the message of the
    error the last watermark's results raise (a device error flag fails fw_results), final stats."""
    from flink_amd.runtime.handle import WindowAggHandle
    g = WindowAggHandle(cfg)
    rows, err = [], None
    for bi, (k, t, iv, dv, wm) in enumerate(batches):
        vals = [iv, dv.view(np.int64)]
        for part in np.array_split(np.arange(len(k)), SPLIT):
            g.push_host(k[part], t[part], [v[part] for v in vals])
        if bi < len(batches) - 1:
            g.advance(wm)
            rows.append(_rows(g.results(reset=True), cfg, set()))
        else:
            with pytest.raises(_native.FlinkWinError) as e:
                g.advance(wm)
                g.results(reset=True)
            err = str(e.value)
    st = g.stats()
    g.close()
    return rows, err, st


@pytest.mark.parametrize("hash_kind", sorted(HASHES))
def test_foreign_key_raises_keygroup_only(monkeypatch, hash_kind):
    """A parallelism-2 handle fed one key of the other subtask (in a packed epoch, inside the key
    field) raises FW_ERRF_KEYGROUP and nothing else, whichever kernel takes the push."""
    cand = (1 << 33) + np.arange(90000, dtype=np.int64)
    own, other = _own_keys(HASHES[hash_kind], 2, 0, cand)
    rng = np.random.default_rng(43)
    batches = [_batch(rng, b, _distinct(rng, own[:40000])) for b in range(3)]
    mid = other[(other > own[100]) & (other < own[30000])][0]  # inside every epoch's key range
    batches[2][0][2 * PUSH + 77] = mid  # the last push before the watermark whose results report the flag
    res = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("FW_IG_PACK", mode)
        res[mode] = _gpu_only(_cfg(_kw(), max_batch_rows=1 << 14, key_hash=HASHES[hash_kind], parallelism=2, subtask_index=0),
                              [list(b) for b in batches])
        assert res[mode][2]["error_flags"] == abi.ERRF["KEYGROUP"], res[mode][2]["error_flags"]
        assert "bits 0x10:" in res[mode][1], res[mode][1]
    assert len(res["2"][0]) == 2
    for a, b in zip(res["2"][0], res["0"][0]):
        _compare(a, b, set(), "modes")


@pytest.mark.parametrize("hash_kind", sorted(HASHES))
def test_key_outside_the_field_raises_no_flag(monkeypatch, hash_kind):
    """A parallelism-2 handle; one own key 2^40 above the epoch's key field makes its chunk slow (the
    slow path routes it in full) and raises no flag."""
    cand = (1 << 33) + np.arange(90000, dtype=np.int64)
    own, _ = _own_keys(HASHES[hash_kind], 2, 0, cand)
    far, _ = _own_keys(HASHES[hash_kind], 2, 0, own[:2000] + (np.int64(1) << 40))
    rng = np.random.default_rng(44)
    batches = [_batch(rng, b, _distinct(rng, own[:40000])) for b in range(3)]
    batches[2][0][PUSH + CH + 9] = far[0]
    cfg_of = lambda: _cfg(_kw(), max_batch_rows=1 << 14, key_hash=HASHES[hash_kind], parallelism=2, subtask_index=0)
    out = _modes(monkeypatch, cfg_of, batches)
    assert out["2"][0]["compact_chunks"] == 2 * SPLIT * 4 - 1  # that chunk alone is PF_WIDE


# ---------------------------------------------------------------------------------------------------
# field widths: both branches of the range statistics
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kspan,vspan", [(40000, (1 << 32) - 1), (40000, 1 << 32), (40000, 1 << 40),
                                         (1 << 33, 1000), (1 << 30, 1000), (1 << 30, 1 << 20)])
def test_field_widths(monkeypatch, kspan, vspan):
    """Accumulator values spanning 2^32 - 1, 2^32 and 2^40 (beside a 17-bit key field), keys spanning
    2^33 (a 35-bit key field, 21 bits left for the accumulator) and 2^30 (32 and 24 bits): a field of
    span s takes bits(s) + 1 bits, the accumulator's also the word's spare ones, and key and
    accumulator fields together fit 62 bits -- so each of the two fields is at most and more than 32
    bits wide in some case, and both branches of the range statistics run for either.  The ranges
    the packing kernel measures are k_ingest's: the next epochs pack the same chunks into the same bytes."""
    rng = np.random.default_rng(51)
    pool = (np.arange(40000, dtype=np.int64) * (kspan // 40000)) + 7
    batches = []
    for b in range(4):
        n = SPLIT * PUSH
        vals = rng.integers(0, vspan, n, dtype=np.int64) - vspan // 2
        vals[:2] = (-(vspan // 2), vspan - 1 - vspan // 2)  # the whole span in every watermark
        batches.append(_batch(rng, b, _distinct(rng, pool), vals))
    out = _modes(monkeypatch, lambda: _cfg(_kw(abi.AGG_MIN), max_batch_rows=1 << 14), batches)
    assert out["2"][0]["compact_chunks"] == 3 * SPLIT * 4


# ---------------------------------------------------------------------------------------------------
# superbucket counts: the run claims
# ---------------------------------------------------------------------------------------------------
def test_odd_superbucket_count(monkeypatch):
    """max_parallelism 128, parallelism 3, subtask 0: 43 key groups, one superbucket each."""
    own, _ = _own_keys(abi.KEYHASH_LONG, 3, 0, np.arange(1, 60000, dtype=np.int64))
    assert len(own) >= 13000
    rng = np.random.default_rng(61)
    batches = [_batch(rng, b, _distinct(rng, own[:13000])) for b in range(4)]
    cfg_of = lambda: _cfg(_kw(), max_batch_rows=1 << 14, parallelism=3, subtask_index=0)
    out = _modes(monkeypatch, cfg_of, batches)
    assert out["2"][0]["num_superbuckets"] == 43
    assert out["2"][1][-1] == 4 * SPLIT
    assert out["2"][0]["compact_chunks"] == 3 * SPLIT * 4


def test_even_superbucket_count_with_sub_run_overflow(monkeypatch):
    """128 superbuckets, every key in 32 of them (~128 rows per chunk and superbucket): stretches run
    past the sub-runs, the rest stays in the chunks' regions behind the overflow flags."""
    cand = np.arange(1, 60000, dtype=np.int64)
    kg = np.zeros(len(cand), dtype=np.int32)
    rc = _native.lib().fw_host_assign_key_groups(cand.ctypes.data, None, len(cand), abi.KEYHASH_LONG, 128, 1, kg.ctypes.data,
                                                 None)
    assert rc == 0
    pool = cand[kg < 32][:PUSH]
    assert len(pool) == PUSH
    rng = np.random.default_rng(62)
    batches = [_batch(rng, b, _distinct(rng, pool)) for b in range(4)]
    out = _modes(monkeypatch, lambda: _cfg(_kw(), max_batch_rows=1 << 14), batches)
    assert out["2"][0]["num_superbuckets"] % 2 == 0
    assert out["2"][1][-1] == 4 * SPLIT
    assert out["2"][0]["compact_chunks"] == 3 * SPLIT * 4
