"""The inputs of test_gpu_folded_capacity_limits.py, run against the references alone: every builder
of folded_capacity_cases.py must sit on the edge it was designed for (63 / 64 / 65 sessions,
1024 / 1025, 64 fires and 65, 2048 / 2049 late rows, `may_add > cap_s - ns` where pass 0 has to run,
the chunk-spanning group's place in the merged list).  No GPU."""
import numpy as np
import pytest
from folded_capacity_cases import (CAP_E, COUNT_PAIRS, KINDS, LONG_MAX, OUT_CAP, SPAN_KEY, TILE, CappedReference, case1, case2,
                                   case3, case4, case5, case6, case7, case8, case9, case10, count_reference_rows,
                                   merged_order, plain_reference, tile_sessions)


def _seeded(kind, c):
    ref = CappedReference(kind, c["cap_s"])
    assert ref.push(c["seed"]) == [] and ref.live() == c["held"] and not ref.state_bit
    return ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("final", [63, 64, 65])
def test_case1_ends_at_63_64_65(kind, final):
    c = case1(kind, final)
    ref = _seeded(kind, c)
    plain = ref.snapshot()
    assert ref.push(c["tile"]) == [] and len(c["tile"]) <= TILE
    c["tile"].feed(plain)
    assert plain.live_sessions() == final                    # what the tile makes of the list, capacity aside
    dropped, after, before, own = ref.tiles[-1]
    assert before == 40 and own > c["cap_s"] - before        # ns + may_add > cap_s: pass 0 runs
    assert (dropped, after, ref.state_bit) == ((True, 40, True) if final == 65 else (False, final, False))
    assert len(ref.wm(LONG_MAX)) == after


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [24, 25])
def test_case2_ends_at_1024_1025_and_spans_the_chunk_boundary(kind, n_new):
    c = case2(kind, n_new)
    ref = _seeded(kind, c)
    assert len(c["tile"]) == TILE and ref.push(c["tile"]) == []
    dropped, after, before, own = ref.tiles[-1]
    assert before == 1000 and own > c["cap_s"] - before and before + len(c["tile"]) == 2024
    assert (dropped, after) == ((True, 1000) if n_new == 25 else (False, 1024))
    m = merged_order(c["state"], c["tile"])
    head, held = m.index(("r", SPAN_KEY, 900)), m.index(("s", SPAN_KEY, 945))
    assert (head, held) == (1000, 1040) and head < TILE <= held
    assert all(e[0] == "r" and e[1] == SPAN_KEY for e in m[head:held])     # the tile session's head and its dead slots
    if not dropped:                                                       # and the held session joins it
        rows = [r for r in ref.wm(LONG_MAX) if r[0] == SPAN_KEY]
        assert len(rows) == 1 and rows[0][-2:] == (900, 955)


@pytest.mark.parametrize("kind", KINDS)
def test_case3_drops_the_middle_tile(kind):
    c = case3(kind)
    ref = _seeded(kind, c)
    assert len(c["push"]) == 3 * TILE and ref.push(c["push"]) == []
    assert [(t[0], t[1]) for t in ref.tiles[-3:]] == c["tiles"] and ref.state_bit
    assert all(t[3] > c["cap_s"] - t[2] for t in ref.tiles[-3:-1])       # tiles 0 and 1 run pass 0
    plain = plain_reference(kind)
    for p in (c["seed"], c["without_tile_1"]):
        p.feed(plain)
    assert len(c["without_tile_1"]) == 2 * TILE
    assert plain.process_watermark(LONG_MAX) == ref.wm(LONG_MAX)


@pytest.mark.parametrize("kind", ["static", "dynamic"])
@pytest.mark.parametrize("over", [False, True])
def test_case4_late_rows_of_a_tile_at_the_edge(kind, over):
    c = case4(kind, over)
    ref = _seeded(kind, c)
    assert ref.wm(c["watermark"]) == [] and ref.live() == 40
    assert ref.push(c["tile"]) == c["late"] and len(c["late"]) == 15 and ref.late_dropped == 15
    dropped, after, _, _ = ref.tiles[-1]
    assert (dropped, after, ref.state_bit) == ((True, 40, True) if over else (False, 64, False))
    plain = plain_reference(kind)
    c["seed"].feed(plain)
    plain.process_watermark(c["watermark"])
    c["tile"].feed(plain)
    assert plain.live_sessions() == c["final"] == (65 if over else 64)


def test_case5_fills_two_chunks_and_closes_up():
    c = case5()
    ref = CappedReference("static", c["cap_s"])
    live, fires = [], []
    for st in c["steps"]:
        if st[0] == "push":
            assert ref.push(st[1]) == []
        else:
            fires.append(len(ref.wm(st[1])))
        live.append(ref.live())
    assert live == c["live"] and fires == c["fires"] and not ref.state_bit
    (_, _, b0, own0), (_, _, b1, own1) = ref.tiles[2], ref.tiles[3]      # the joining tile, the tile behind the watermark
    assert b0 == 1500 and b0 + own0 > c["cap_s"] and b0 + TILE > 2 * TILE  # pass 0 runs; L spans three chunks
    assert b1 == 800 and b1 + own1 <= c["cap_s"] and b1 + TILE == 1824
    kept = c["kept"]
    assert len(kept) == 800 and int((kept < TILE).sum()) == 544            # 256 sessions of chunk 1 move into chunk 0's slots
    due = np.arange(1500) % 15 < 7                                         # due and kept interleave in both chunks
    assert int(due[:TILE].sum()) == 480 and int(due[TILE:].sum()) == 220


@pytest.mark.parametrize("kind", ["static", "sql4"])
def test_case6_fires_64_then_65(kind):
    c = case6(kind)
    ref = CappedReference(kind)
    for p in c["pushes"]:
        assert ref.push(p) == []
    assert ref.live() == 64 + 65 and len(ref.wm(c["first"])) == 64 == OUT_CAP
    snap = ref.snapshot()
    whole = ref.wm(c["over"])
    assert len(whole) == 65 == OUT_CAP + 1 and ref.live() == 0
    ref.restore(snap)
    parts = [ref.wm(w) for w in c["split"]]
    assert [len(p) for p in parts] == c["fires"][2:] and {r[0]: r for r in parts[0] + parts[1]} == {r[0]: r for r in whole}


@pytest.mark.parametrize("n", [2048, 2049])
def test_case7_late_rows_at_the_side_capacity(n):
    c = case7(n)
    ref = CappedReference("static")
    ref.wm(c["watermark"])
    late = [i for p in c["pushes"] for i in ref.push(p)]
    assert len(late) == n == ref.late_dropped and ref.live() == 0 and c["side_cap"] == 2048
    assert all(len(p) <= TILE for p in c["pushes"]) and ref.push(c["after"]) == [0, 1, 2]


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
def test_case8_fills_the_table_then_two_more(size, slide):
    c = case8(size, slide)
    held, extra = set(c["held"].tolist()), set(c["extra"].tolist())
    assert len(held) == CAP_E and len(extra) == 2 and not held & extra
    assert all(set(k.tolist()) == held for k, _ in c["pushes"][:2] + c["pushes"][3:])
    assert set(c["pushes"][2][0].tolist()) == held | extra
    rows = count_reference_rows(size, slide, ("sum", "LONG"), c["pushes"])
    assert all({r[0] for r in per} >= held for per in rows)                # every held key fires in every push
    # count windows are independent per key: the held keys' rows are those of the stream without the two
    sel = np.isin(c["pushes"][2][0], c["held"])
    filtered = c["pushes"][:2] + [(c["pushes"][2][0][sel], c["pushes"][2][1][sel])]
    want = [r[:4] for r in rows[2] if r[0] in held]
    assert [r[:4] for r in count_reference_rows(size, slide, ("sum", "LONG"), filtered)[2]] == want and len(want) >= CAP_E


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
def test_case9_race_tile(size, slide):
    c = case9(size, slide)
    held, new = set(c["held"].tolist()), set(c["new"].tolist())
    race = c["pushes"][1][0]
    assert len(held) == CAP_E - 10 and len(new) == 40 and c["room"] == 10 and not held & new
    assert len(race) <= TILE and set(race.tolist()) == held | new
    rows = count_reference_rows(size, slide, ("sum", "LONG"), c["pushes"])
    assert {r[0] for r in rows[1]} >= held and {r[0] for r in rows[2]} == held | new


@pytest.mark.parametrize("size,slide", COUNT_PAIRS)
def test_case10_fires_64_then_65(size, slide):
    c = case10(size, slide)
    (k1, v1), (k2, v2) = c["pushes"]
    cut = c["cut"]
    rows = count_reference_rows(size, slide, ("sum", "LONG"), [(k1, v1), (k2, v2)])
    split = count_reference_rows(size, slide, ("sum", "LONG"), [(k1, v1), (k2[:cut], v2[:cut]), (k2[cut:], v2[cut:])])
    assert [len(r) for r in rows] + [len(r) for r in split[1:]] == c["fires"]
    assert [r[:4] for r in split[1] + split[2]] == [r[:4] for r in rows[1]]


def test_tile_sessions_counts_what_the_tile_forms_alone():
    c = case1("static", 64)
    assert tile_sessions(c["seed"]) == 40 and tile_sessions(c["tile"]) == 30 + 10 + 29
