"""The inputs of tests/test_gpu_count_record_exchange.py reach the edges they are meant to reach -- checked
on the reference alone, without a GPU -- and the host pieces of the exchange form: the word <-> tuple
codec of RecordCountWindowOperator and the refusals of record_types=.

The reference (CountRecordReference) runs over the live rows in buffer position order with the
ordinals count_exchange_cases.expected_ord gives, push_seq << 32 | buffer position.
"""
import count_exchange_cases as cx
import count_record_exchange_cases as cases
import numpy as np
import pytest
from count_record_reference import bits_of, double_of, record_image

from flink_amd.datastream import record_count_window_operator as rcw

WINDOWS = cx.WINDOWS


def test_geometry_and_ordinals():
    pushes = cases.build_case("sum", "LONG")
    assert [p["counts"] for p in pushes] == cx.COUNTS and cx.N_SEGS * cx.SEG_LEN <= cases.MAX_BATCH_ROWS
    n_foreign_pad = 0
    for b, p in enumerate(pushes):
        assert p["rows"].shape == (4500, 2 + cases.F)
        ords = cases.ordinals(p, b)
        assert ords == [cx.expected_ord(pushes, sum(len(q["pos"]) for q in pushes[:b]) + i) for i in range(len(ords))]
        # tags are unique over the whole buffer, padding included, and a padding row's is none of a live row's
        tags = p["rows"][:, 2 + 2]
        assert len(set(tags.tolist())) == 4500
        assert [r[2] for r in p["records"]] == tags[p["pos"]].tolist()
        # the padding holds foreign keys and the hot key
        hot, _, foreign = cx.keys_of("LONG")
        live = np.zeros(4500, bool)
        live[p["pos"]] = True
        pad_keys = set(p["rows"][~live, 0].tolist())
        assert pad_keys <= set(foreign.tolist()) | {hot} and hot in pad_keys
        n_foreign_pad += len(pad_keys) - 1
    assert n_foreign_pad > 100
    # the weights: NaNs with payloads, both zeros
    w = {record_image(r)[3] for p in pushes for r in p["records"]}
    assert {("f64", 0x7FF80000000ABCDE), ("f64", 0x7FF00000DEADBEEF), ("f64", -(1 << 63)), ("f64", 0)} <= w


def test_a_hot_key_run_exceeds_the_tile():
    hot = cx.keys_of("LONG")[0]
    assert max(int((p["live_keys"] == hot).sum()) for p in cases.build_case("sum", "LONG")) > cx.TILE


@pytest.mark.parametrize("window", WINDOWS, ids=str)
@pytest.mark.parametrize("agg", cases.AGGS, ids=lambda a: "-".join(map(str, a)))
def test_reference_reaches_the_edges(window, agg):
    run = cases.reference_run(window, agg, "LONG")
    assert all(len(rows) > 0 for rows, _ in run)
    held_before = frozenset()
    ever_held = set()
    earlier = current_unretained = both = False
    for b, (rows, held) in enumerate(run):
        ever_held |= held
        both |= bool(held - held_before) and bool(held_before - held)
        held_before = held
    for b, (rows, held) in enumerate(run):
        for _, _, trig, rord in rows:
            assert trig >> 32 == b and rord <= trig
            earlier |= rord >> 32 < b
            current_unretained |= rord >> 32 == b and rord not in ever_held
    assert both                  # some push both retains and releases
    assert current_unretained    # some result names an element of its own push that is never retained
    # some result names a record retained in an earlier push -- but for maxBy, ties to the newest, over
    # (250, 150): only the hot key fires there, and among its last 250 values from [-3, 4) the newest
    # maximum is a handful of rows old, never a push old
    assert earlier or (window, agg) == ((250, 150), ("maxBy", False))


@pytest.mark.parametrize("window", WINDOWS, ids=str)
@pytest.mark.parametrize("fn", ["minBy", "maxBy"])
@pytest.mark.parametrize("ftype", cases.FTYPES)
def test_ties_decide_results_under_both_tie_rules(window, fn, ftype):
    """the same stream under first = True and first = False: the rules pick different elements, so a tie
    occurred inside a fired window under each"""
    a = [r for rows, _ in cases.reference_run(window, (fn, True), ftype) for r in rows]
    b = [r for rows, _ in cases.reference_run(window, (fn, False), ftype) for r in rows]
    assert len(a) == len(b) > 0 and [r[2] for r in a] == [r[2] for r in b]
    differ = [(x, y) for x, y in zip(a, b) if x[3] != y[3]]
    assert differ and all(x[3] < y[3] for x, y in differ)   # first: the earlier element, last: the later one


def test_int_sums_wrap_and_double_sums_are_exact():
    for window in WINDOWS:
        rows = [r for rs, _ in cases.reference_run(window, ("sum",), "INT") for r in rs]
        # every window adds at least three values just below 2^31: an INT result means the sum wrapped
        assert rows and all(-(1 << 31) <= r[1][1] < (1 << 31) for r in rows) and min(window[0], window[1] or window[0]) >= 3
        rows = [r for rs, _ in cases.reference_run(window, ("sum",), "DOUBLE") for r in rs]
        assert rows and all(float(r[1][1] * 2).is_integer() for r in rows)


# ---- the word <-> tuple codec -------------------------------------------------------------------------
def test_words_round_trip():
    types = ["INT", "DOUBLE", "LONG", "DOUBLE", "INT"]
    nan_bits = [0x7FF80000000ABCDE, 0x7FF00000DEADBEEF, 0xFFF8000000000001 - (1 << 64), -(1 << 63), 0, bits_of(1.5)]
    recs = [(i32, double_of(d), lng, double_of(nan_bits[(i + 1) % len(nan_bits)]), -i32 - 1)
            for i, (i32, d, lng) in enumerate(zip([-(1 << 31), (1 << 31) - 1, -1, 0, 7, -9],
                                                  nan_bits, [-(1 << 63), (1 << 63) - 1, -1, 0, 1 << 40, -(1 << 40)]))]
    words = np.array([rcw.record_to_words(r, types) for r in recs], np.int64)
    assert words[:, 1].tolist() == nan_bits                       # a DOUBLE travels as its bits
    assert words[0, 0] == -(1 << 31) and words[1, 0] == (1 << 31) - 1   # an INT sign-extended
    back = rcw.words_to_records(words, types)
    assert [record_image(r) for r in back] == [record_image(r) for r in recs]
    assert all(type(x) is (float if t == "DOUBLE" else int) for r in back for x, t in zip(r, types))
    # an INT word is narrowed: the upper half of a 64-bit word is not part of the field
    assert rcw.words_to_records(np.array([[(5 << 32) | 0xFFFFFFFE]], np.int64), ["INT"]) == [(-2,)]
    assert rcw.words_to_records(np.empty((0, 5), np.int64), types) == []
    assert [record_image(r) for r in cases.words_to_tuples(words, types)] == [record_image(r) for r in back]   # the tests' own decode agrees


# ---- record_types= refusals (host only: no handle is opened) ---------------------------------------------
def test_record_types_refusals():
    from flink_amd.datastream import RecordCountWindowOperator as Op
    with pytest.raises(ValueError, match="1 .. 8 fields"):
        Op(4, None, ("sum", "LONG"), field=0, record_types=[])
    with pytest.raises(ValueError, match="1 .. 8 fields"):
        Op(4, None, ("sum", "LONG"), field=0, record_types=["LONG"] * 9)
    with pytest.raises(ValueError, match="outside the record"):
        Op(4, None, ("sum", "LONG"), field=2, record_types=["LONG", "LONG"])
    with pytest.raises(ValueError, match="not LONG / INT / DOUBLE"):
        Op(4, None, ("sum", "LONG"), field=0, record_types=["LONG", "STRING"])
    with pytest.raises(ValueError, match="aggregated field is LONG"):
        Op(4, None, ("sum", "LONG"), field=1, record_types=["LONG", "DOUBLE"])
    op = Op(5, 3, ("maxBy", "DOUBLE", False), field=7, record_types=["LONG"] * 7 + ["DOUBLE"], parallelism=2)
    assert op.cfg.n_value_cols == 8 and op.cfg.aggs[0].input_col == 7 and op.record_types[7] == "DOUBLE"
    plain = Op(5, 3, ("sum", "LONG"))   # the default: the operator as it was
    assert plain.record_types is None and plain.cfg.n_value_cols == 1 and plain.cfg.aggs[0].input_col == 0


def test_exchange_step_refusals():
    from flink_amd.datastream import RecordCountExchangeStep
    from flink_amd.datastream import RecordCountWindowOperator as Op
    with pytest.raises(ValueError, match="record_types"):
        RecordCountExchangeStep(Op(5, 3, ("sum", "LONG"), parallelism=2))
    with pytest.raises(ValueError, match="parallelism 1"):
        RecordCountExchangeStep(Op(5, 3, ("sum", "LONG"), field=0, record_types=["LONG"]))
