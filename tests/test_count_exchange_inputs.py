"""The inputs of tests/test_gpu_count_exchange.py exercise what they are meant to (no GPU needed):
conditions on the cases of tests/count_exchange_cases.py against the count-window reference.  If a
case fails one, change the case, not the assertion.

Also: the library exports the count handle's segment pushes, and the ABI version did not move.
"""
import ctypes as C

import numpy as np
import pytest
from count_window_reference import CountWindowReference

import count_exchange_cases as cases
from flink_amd import _native, abi


@pytest.mark.parametrize("key_kind", sorted(cases.KEY_KINDS))
@pytest.mark.parametrize("window", cases.WINDOWS)
def test_case_reaches_the_edges(key_kind, window):
    size, slide = window
    pushes, _ = cases.build_case(key_kind, "LONG")
    hot, own, foreign = cases.keys_of(key_kind)
    ref = CountWindowReference(size, slide, ("count", "LONG"))
    hot_push, hot_launch = [], []       # per hot element, in its per-key order
    tile_ok = False
    for b, p in enumerate(pushes):
        assert len(p["keys"]) == cases.N_SEGS * cases.SEG_LEN and len(p["pos"]) == len(p["live_keys"])
        assert sum(min(c, cases.SEG_LEN) for c in p["counts"]) == len(p["pos"])
        launch = p["pos"] // cases.MAX_BATCH_ROWS
        first = ref.arrived
        fired = ref.process(p["live_keys"].tolist(), p["live_values"].tolist())
        assert fired, f"push {b} fires nothing"                       # the reference fires rows in every push
        for i in np.flatnonzero(p["live_keys"] == hot):
            hot_push.append(b)
            hot_launch.append(int(launch[i]))
        # the hot key fires twice inside one 1024-row tile: a tile holds up to 1024 consecutive rows of
        # one superbucket of one launch, a subset of the launch's live rows -- so of three fires of one
        # launch that lie within 1024 live rows, two share a tile wherever the tile boundary falls
        trig = np.array([r[4] - first for r in fired if r[0] == hot], dtype=np.int64)  # live-row indices
        for la in np.unique(launch):
            t = trig[launch[trig] == la]
            if any(t[j + 2] - t[j] < cases.TILE for j in range(len(t) - 2)):
                tile_ok = True
        # the padding: no live row is foreign, every padding row is foreign or the hot key
        pad = np.ones(len(p["keys"]), dtype=bool)
        pad[p["pos"]] = False
        assert not np.isin(p["live_keys"], foreign).any()
        assert (np.isin(p["keys"][pad], foreign) | (p["keys"][pad] == hot)).all()
    assert tile_ok
    # fired windows of the hot key that hold elements of two launches of one push, and of two pushes
    ref2 = CountWindowReference(size, slide, ("count", "LONG"))
    two_launches = two_pushes = False
    for p in pushes:
        for k, _, ws, we, _ in ref2.process(p["live_keys"].tolist(), p["live_values"].tolist()):
            if k != hot:
                continue
            pb, la = hot_push[ws:we], hot_launch[ws:we]
            if len(set(pb)) > 1:
                two_pushes = True
            elif len(set(la)) > 1:
                two_launches = True
    assert two_launches and two_pushes
    # some padding carries the hot key
    assert any((p["keys"][np.setdiff1d(np.arange(len(p["keys"])), p["pos"])] == hot).any() for p in pushes)


def test_hot_key_share_and_key_count():
    pushes, _ = cases.build_case("LONG", "LONG")
    hot, own, _ = cases.keys_of("LONG")
    live = np.concatenate([p["live_keys"] for p in pushes])
    assert 0.35 < (live == hot).mean() < 0.45
    assert len(np.unique(live)) > 250


def test_library_exports_the_count_segment_pushes():
    L = _native.lib()
    raw = C.CDLL(L._name)
    for name in ("fw_push_device_count_segments", "fw_push_device_count_packed_segments"):
        assert hasattr(raw, name), name
        assert name in _native.EXPORTED
    assert L.fw_abi_version() == abi.FW_ABI_VERSION == 11
