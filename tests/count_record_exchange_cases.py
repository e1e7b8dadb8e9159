"""The padded receive buffers of the record count-window exchange tests, in plain numpy: the inputs of
tests/test_gpu_count_record_exchange.py, checked without a GPU by tests/test_count_record_exchange_inputs.py.

Built on count_exchange_cases.build_push: its geometry (3 segments of 1500 rows, its COUNTS: an
over-full, an empty, a one-row and partial segments), its keys (40 % one hot key the subtask owns, 300
more it owns) and its poisoned padding (foreign keys, and the hot key behind the last padded segment's
live rows).  max_batch_rows is 8192 >= 4500, so every buffer is one launch.

A record has F = 4 fields, types RECORD_TYPES[ftype][field]: a copy of the key, the aggregated field,
a LONG tag and a DOUBLE weight.  The tag is unique per buffer position, padding included (push * 10^6
+ position; + 5 * 10^5 on a padding row), so a record gathered from a wrong row -- a padding row, a
neighbour -- never equals the right one.  The weight cycles through NaNs with payloads (a signalling
one among them), -0.0, 0.0 and plain values, so a record compares equal only bit for bit.

The aggregated field's values are drawn from few distinct ones, so min / max / minBy / maxBy meet
ties all the time: LONG from [-3, 4), INT from the four values below 2^31 (every sum of two wraps),
DOUBLE from SPECIAL for the comparing aggregates and from multiples of 0.5 in [0, 100) for sums --
such sums are exact in any order of addition, so DOUBLE sums compare bit for bit as well.
"""
import functools

import count_exchange_cases as cx
import numpy as np
from count_record_reference import CountRecordReference, bits_of, double_of

from flink_amd import abi

MAX_BATCH_ROWS = 8192
SEED = 1
F = 4
FIELD_LAYOUTS = (1, 3)   # index of the aggregated field: (key, AGG, tag, weight) or (key, tag, weight, AGG)
AGGS = [("sum",), ("min",), ("max",), ("minBy", True), ("maxBy", False)]
FTYPES = ("LONG", "INT", "DOUBLE")
SPECIAL = [0x7FF8000000000000, 0xFFF8000000000001 - (1 << 64), 0x7FF00000DEADBEEF, -(1 << 63), 0, bits_of(1.0), bits_of(-1.0),
           bits_of(float("inf")), bits_of(float("-inf")), bits_of(2.5)]
WEIGHTS = [0x7FF80000000ABCDE, 0x7FF00000DEADBEEF, -(1 << 63), 0, bits_of(0.25), bits_of(-7.5), 0xFFF8000000000001 - (1 << 64)]


def aggregation(agg, ftype):
    return (agg[0], ftype) + tuple(agg[1:])


def record_types(ftype, field):
    other = ["LONG", "LONG", "DOUBLE"]   # key copy, tag, weight
    return other[:field] + [ftype] + other[field:]


def field_words(rng, n, fn, ftype):
    """n words of the aggregated field (int64: an INT sign-extended, a DOUBLE its bits)"""
    if ftype == "LONG":
        return rng.integers(-3, 4, n).astype(np.int64)
    if ftype == "INT":
        return rng.integers((1 << 31) - 4, 1 << 31, n).astype(np.int64)
    if fn == "sum":
        return (rng.integers(0, 200, n) * 0.5).view(np.int64)
    return np.array(SPECIAL, np.int64)[rng.integers(0, len(SPECIAL), n)]


def build_record_push(rng, b, fn, ftype, field, counts, n_segs=cx.N_SEGS, seg_len=cx.SEG_LEN, key_kind="LONG"):
    """Push b: count_exchange_cases.build_push's dict plus rows -- the packed buffer [n, 2 + F] int64,
    word 1 garbage --, live_words [n_live, F] and records, the live rows as tuples in arrival order."""
    p = cx.build_push(rng, key_kind, "LONG", counts, n_segs, seg_len)
    n = n_segs * seg_len
    live = np.zeros(n, bool)
    live[p["pos"]] = True
    agg_w = field_words(rng, n, fn, ftype)
    tag = b * 10**6 + np.arange(n, dtype=np.int64) + np.where(live, 0, 5 * 10**5)
    weight = np.array(WEIGHTS, np.int64)[(np.arange(n) + 3 * b) % len(WEIGHTS)]
    weight = np.where(np.arange(n) % 3 == 0, (np.arange(n) * 0.5 + b).view(np.int64), weight)
    other = [p["keys"].copy(), tag, weight]
    cols = other[:field] + [agg_w] + other[field:]
    rows = np.empty((n, 2 + F), np.int64)
    rows[:, 0] = p["keys"]
    rows[:, 1] = rng.integers(-2**62, 2**62, n)   # the word no one reads
    for f, c in enumerate(cols):
        rows[:, 2 + f] = c
    p["rows"] = rows
    p["live_words"] = rows[p["pos"], 2:]
    p["live_values"] = rows[p["pos"], 2 + field]
    p["records"] = words_to_tuples(p["live_words"], record_types(ftype, field))
    return p


def words_to_tuples(words, types):
    """the test's own decode (not the operator's): INT narrowed, DOUBLE by its bits"""
    out = []
    for row in np.asarray(words, np.int64).reshape(-1, len(types)).tolist():
        out.append(tuple(double_of(w) if t == "DOUBLE" else int(np.int32(np.int64(w))) if t == "INT" else w for w, t in zip(row, types)))
    return out


@functools.lru_cache(maxsize=None)
def build_case(fn, ftype, field=1, seed=SEED, counts_list=tuple(cx.COUNTS)):
    """the case's pushes; the same for every window and tie rule of (fn, ftype, field)"""
    rng = np.random.default_rng(seed)
    return [build_record_push(rng, b, fn, ftype, field, c) for b, c in enumerate(counts_list)]


def ordinals(p, b, first_push_seq=0):
    return (((first_push_seq + b) << 32) | p["pos"]).tolist()


@functools.lru_cache(maxsize=None)
def reference_run(window, agg, ftype, field=1, seed=SEED):
    """One CountRecordReference over the case's live rows in buffer position order: per push
    (fired rows, held() after the push).  Computed once and shared; nobody changes it."""
    pushes = build_case(agg[0], ftype, field, seed)
    ref = CountRecordReference(window[0], window[1], aggregation(agg, ftype), field=field)
    out = []
    for b, p in enumerate(pushes):
        rows = ref.process(p["live_keys"].tolist(), p["records"], ordinals(p, b))
        out.append((rows, frozenset(ref.held())))
    return out


def keyhash_of(key_kind="LONG"):
    return {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT}[key_kind]
