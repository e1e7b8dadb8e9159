"""The time-window checkpoint path end to end on the device (flink_amd/csrc/fw_checkpoint.hip): a
restore decodes and checks its blob on the host before the handle changes, and a heap restore installs
the decoded state directly.

* A damaged whole-handle or key-group blob raises, and the handle it was offered to is untouched: its
  next snapshot is byte for byte the one taken before, and it goes on matching the oracle.
* Heap export -> heap restore into a fresh handle -> heap export gives the same bytes.
* A key-row key-group blob written at one parallelism and sub-bucket split restores at another
  parallelism and split with every entry, flag and key row intact: the decoder refuses nothing the
  restore accepts."""
import struct

import numpy as np
import pytest

from flink_amd import abi
from test_gpu_key_rows import _OracleKeys, _route

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000_000
SNAP_HDR, KG_HDR = 72, 80  # SnapHeader / KgHeader bytes (fw_ckpt_format.h)

CONFIGS = {
    # SQL TUMBLE, BIGINT keys
    "tumble_bigint": dict(key_type="BIGINT", tumble=4000, aggs=[("COUNT_STAR", 0, "BIGINT"), ("SUM", 0, "BIGINT")]),
    # SQL HOP (block state), (VARCHAR, BIGINT) key rows
    "hop_key_rows": dict(key_type=("VARCHAR", "BIGINT"), hop=(3000, 1000),
                         aggs=[("COUNT_STAR", 0, "BIGINT"), ("SUM", 0, "BIGINT")]),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _op_kw(c, **extra):
    from flink_amd.table.slice_assigners import SliceAssigners
    assigner = SliceAssigners.tumbling(0, c["tumble"]) if "tumble" in c else SliceAssigners.hopping(0, *c["hop"])
    kw = dict(assigner=assigner, aggs=c["aggs"], value_types=["BIGINT"], count_star_index=0, key_type=c["key_type"],
              state_capacity=1 << 14, max_batch_rows=1 << 12, output_capacity=1 << 14, key_row_max_bytes=64)
    kw.update(extra)
    return kw


def _universe(c, n):
    if c["key_type"] == "BIGINT":
        return [(int(k) * 7919 - 50000,) for k in range(n)]
    return [("key-%d" % (k * 31), int(k) * 13 - 40) for k in range(n)]


class _Rig:
    """One operator beside one oracle: step(b) pushes batch b to both, advances both and compares."""

    def __init__(self, c):
        from flink_amd.table.window_agg import WindowAggOperator
        from oracle import oracle as O
        self.c, self.rows_of, self.ids = c, _universe(c, 20), _OracleKeys()
        self.op = WindowAggOperator(**_op_kw(c)).open()
        kind, size, slide = (abi.WIN_TUMBLE, c["tumble"], 0) if "tumble" in c else (abi.WIN_HOP, *c["hop"])
        self.orc = O.OracleOperator(abi.make_config(
            api=abi.API_SQL, window_kind=kind, size_ms=size, slide_ms=slide, count_star_index=0, value_col_types=[abi.T_I64],
            aggs=[(abi.AGG_NAMES[k], col, abi.TYPE_NAMES[t]) for k, col, t in c["aggs"]], key_hash=abi.KEYHASH_PRECOMPUTED))
        self.rng = np.random.default_rng(41)

    def step(self, b, n=200):
        rows = [self.rows_of[i] for i in self.rng.integers(0, len(self.rows_of), n)]
        ts = T0 + b * 1500 + self.rng.integers(-1200, 1200, n)
        val = self.rng.integers(-1000, 1000, n).astype(np.int64)
        keys = np.array([r[0] for r in rows], np.int64) if self.c["key_type"] == "BIGINT" else rows
        self.op.process_batch(keys, ts, [val])
        self.orc.process_batch(self.ids.encode(rows), ts, [val])
        wm = T0 + b * 1500 - 500
        got = self.op.output_rows(self.op.process_watermark(wm))
        self.orc.process_watermark(wm)
        r = self.orc.results(clear=True)
        want = [self.ids.decode(k) + tuple(int(v[i]) for v in r["values"]) + (int(ws), int(we))
                for i, (k, ws, we) in enumerate(zip(r["key"], r["window_start"], r["window_end"]))]
        assert sorted(got, key=repr) == sorted(want, key=repr), f"batch {b}"
        return len(got)

    def close(self):
        self.op.close()
        self.orc.close()


def _poke(blob, at, fmt, v):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, v)
    return bytes(b)


def _key_row_section(blob):
    """Byte offset of a blob's key-row section: [n][id, hash << 32 | length, image words]..."""
    if struct.unpack_from("<Q", blob, 0)[0] == 0x464c4b57494e3033:  # whole handle: header, counts, entries
        n_sb, _, pwe = struct.unpack_from("<3i", blob, 12)
        return SNAP_HDR + 4 * n_sb + struct.unpack_from("<q", blob, 48)[0] * pwe * 8
    return KG_HDR + struct.unpack_from("<q", blob, 56)[0] * struct.unpack_from("<i", blob, 16)[0] * 8


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_refused_blob_leaves_the_handle_untouched(name):
    """About 200 rows over 20 keys; the whole-handle blob and one non-empty key-group blob, each with
    one field damaged (a superbucket count above cap_e, an entry count of -1, a key-row length of 12),
    are refused, and the handle they were offered to snapshots and computes as if nothing had happened."""
    from flink_amd._native import FlinkWinError
    c = CONFIGS[name]
    rig = _Rig(c)
    try:
        rig.step(0)
        rig.step(1)
        h = rig.op.handle
        kgs, _ = h.snapshot_key_groups()
        whole = h.snapshot()
        kg = max(kgs.values(), key=len)
        assert struct.unpack_from("<q", whole, 48)[0] > 0 and struct.unpack_from("<q", kg, 56)[0] > 0
        n_sb, cap_e = struct.unpack_from("<2i", whole, 12)
        first = next(s for s in range(n_sb) if struct.unpack_from("<i", whole, SNAP_HDR + 4 * s)[0] > 0)
        bad = [("whole", _poke(whole, SNAP_HDR + 4 * first, "<i", cap_e + 1)),  # a count above cap_e
               ("whole", _poke(whole, 48, "<q", -1)),                            # live = -1
               ("kg", _poke(kg, 56, "<q", -1))]                                  # n = -1
        if c["key_type"] != "BIGINT":  # the first key row's length word: 12 bytes
            for kind, blob in (("whole", whole), ("kg", kg)):
                at = _key_row_section(blob) + 16
                bad.append((kind, _poke(blob, at, "<I", 12)))
        for kind, blob in bad:
            with pytest.raises(FlinkWinError):
                (h.restore if kind == "whole" else h.restore_key_group_blob)(blob)
        assert h.snapshot() == whole
        assert h.snapshot_key_groups()[0] == kgs
        assert h.stats()["error_flags"] == 0
        assert rig.step(2) + rig.step(3) > 0
    finally:
        rig.close()


def test_heap_restore_round_trip_is_byte_identical():
    """HOP block state with key rows: heap export, heap restore into a fresh handle, heap export again
    give the same bytes, key group by key group.  The heap bytes list a key group's states in entry order
    and break ties among its timers by table id, neither of which a restore promises to keep across
    keys; so every key group holds one key here (each key's slices lie in one block: one entry)."""
    from flink_amd.table.window_agg import WindowAggOperator
    c = CONFIGS["hop_key_rows"]
    rng = np.random.default_rng(9)
    cand = _universe(c, 400)
    kgs = _route(cand, c["key_type"], 128)  # at parallelism 128 a subtask is a key group
    rows_of = [cand[i] for i in np.unique(kgs, return_index=True)[1]]
    assert len(rows_of) > 60
    a = WindowAggOperator(**_op_kw(c)).open()
    b = WindowAggOperator(**_op_kw(c)).open()
    try:
        rows = [rows_of[i] for i in rng.integers(0, len(rows_of), 800)]
        a.process_batch(rows, T0 + rng.integers(0, 6000, len(rows)), [rng.integers(-1000, 1000, len(rows)).astype(np.int64)])
        a.process_watermark(T0 + 2500)
        first = {kg: a.handle.snapshot_key_group_heap(kg) for kg in range(128)}
        assert sum(len(x) > 22 for x in first.values()) > 60  # (an empty key group is 4 + 3 * 6 bytes)
        b.handle.initialize_watermark(a.handle.stats()["current_watermark"])
        for blob in first.values():
            b.handle.restore_key_group_heap(blob)
        again = {kg: b.handle.snapshot_key_group_heap(kg) for kg in range(128)}
        assert again == first
        assert b.handle.stats()["error_flags"] == 0
    finally:
        a.close()
        b.close()


def _kg_entries(blob):
    """A key-row key-group blob's entries with their key images in place of the table ids, sorted:
    (image, slice or block start, flags without the source sub-bucket, accumulator words)."""
    pwe = struct.unpack_from("<i", blob, 16)[0]
    n = struct.unpack_from("<q", blob, 56)[0]
    w = np.frombuffer(blob, np.uint64, offset=KG_HDR)
    ent, sec = w[:n * pwe].reshape(n, pwe), w[n * pwe:]
    images, p = {}, 1
    for _ in range(int(sec[0])):
        words = (int(sec[p + 1]) & 0xFFFFFFFF) // 8
        images[int(sec[p])] = sec[p + 2:p + 2 + words].tobytes()
        p += 2 + words
    return sorted((images[int(e[0])], int(e[1]), int(e[2]) & 0xFFFFFFFF, e[3:].tobytes()) for e in ent)


def test_key_group_restore_at_another_parallelism_and_split_round_trips():
    """Key-row key-group blobs written at parallelism 2 with several sub-buckets per key group restore
    at parallelism 3 with one: the blobs the new subtasks write hold the same entries and key rows."""
    from flink_amd.table.window_agg import WindowAggOperator
    c = CONFIGS["hop_key_rows"]
    rng = np.random.default_rng(13)
    rows_of = _universe(c, 300)
    src = [WindowAggOperator(parallelism=2, subtask_index=i, **_op_kw(c, state_capacity=1 << 21)).open() for i in range(2)]
    dst = [WindowAggOperator(parallelism=3, subtask_index=i, **_op_kw(c)).open() for i in range(3)]
    try:
        for b in range(3):
            rows = [rows_of[i] for i in rng.integers(0, len(rows_of), 1500)]
            ts = T0 + b * 2000 + rng.integers(-1500, 1500, len(rows))
            val = rng.integers(-1000, 1000, len(rows)).astype(np.int64)
            dest = _route(rows, c["key_type"], 2)
            for d, op in enumerate(src):
                m = dest == d
                op.process_batch([r for r, keep in zip(rows, m) if keep], ts[m], [val[m]])
                op.process_watermark(T0 + b * 2000 - 1600)
        blobs, wms = {}, []
        for op in src:
            bl, wm = op.handle.snapshot_key_groups()
            blobs.update(bl)
            wms.append(wm)
        assert len(blobs) == 128 and sum(len(_kg_entries(x)) for x in blobs.values()) >= 200  # (most keys: one block)
        again = {}
        for op in dst:
            op.handle.restore_key_groups(blobs, wms)
            again.update(op.handle.snapshot_key_groups()[0])
        split = lambda bl: {struct.unpack_from("<i", x, 24)[0] for x in bl.values()}  # KgHeader.sb_log2
        assert split(again) == {0} and min(split(blobs)) > 0, "the two sides must split their key groups differently"
        assert sorted(again) == sorted(blobs)
        for kg in blobs:
            assert _kg_entries(again[kg]) == _kg_entries(blobs[kg]), f"key group {kg}"
        assert all(op.handle.stats()["error_flags"] == 0 for op in src + dst)
    finally:
        for op in src + dst:
            op.close()
