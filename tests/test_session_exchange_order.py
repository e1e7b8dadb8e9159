"""The order helper of the session multirank test (tests/session_exchange_order.py) against the keyBy
exchange itself, on CPU: a two-process gloo group runs KeyByExchange's packed exchange over CPU
tensors (the host partition), and the row sequence every destination receives -- its segments
sender by sender, then its spill -- must be the helper's, with and without overflow.  And the streams
the multirank test uses must exercise what makes a session fold depend on that order: rows that are
late when they arrive, some dropped, some kept because an open session of their key reaches them.
"""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import session_exchange_order as order

WORLD = 2


def _worker(rank, port, name, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        from flink_amd.runtime.exchange import KeyByExchange
        sc = order.SCENARIOS[name]
        ex = KeyByExchange(order.key_hash_kind(sc), order.MAX_PARALLELISM)
        seqs, wms = [], []
        for b in range(order.N_BATCHES):
            cols = [torch.from_numpy(c) for c in order.stream(sc, rank, b)]
            cap = order.segment_cap(b, WORLD)
            px = ex.exchange_packed_async(cols[0], cols[1], cols[2:], capacity=cap)
            spill, wm = px.finish(order.proposed_wm(b, rank))
            w = px.row_words
            seg = px.rows.view(WORLD, cap, w)
            keep = torch.arange(cap)[None, :] < px.recv_counts.clamp(max=cap)[:, None]
            got = seg[keep]
            if spill is not None:
                got = torch.cat([got, spill.view(-1, w)])
            seqs.append(got.numpy().copy())
            wms.append(wm)
        out_q.put((rank, seqs, wms, ex.spill_rounds))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_destination_sequence_is_the_helpers():
    name = "dynamic_gap"  # four words a row
    sc = order.SCENARIOS[name]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, name, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in range(WORLD))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    overflowed = 0
    for b in range(order.N_BATCHES):
        senders = [order.stream(sc, r, b) for r in range(WORLD)]
        cap = order.segment_cap(b, WORLD)
        for d in range(WORLD):
            want = np.stack(order.destination_sequence(senders, cap, d, order.key_hash_kind(sc), order.MAX_PARALLELISM,
                                                       WORLD), axis=1)
            got = res[d][1][b]
            assert got.shape == want.shape and (got == want).all(), f"batch {b}, destination {d}"
        _, n_spill = order.reference_order(senders, cap, order.key_hash_kind(sc), order.MAX_PARALLELISM, WORLD)
        assert (n_spill > 0) == bool(b % 2)   # odd steps overflow, even steps do not
        overflowed += n_spill > 0
        assert res[0][2][b] == res[1][2][b] == order.proposed_wm(b, 0)
    assert res[0][3] == res[1][3] == overflowed == order.N_BATCHES // 2
    # the helper's one global order holds every destination's sequence as a subsequence
    senders = [order.stream(sc, r, 1) for r in range(WORLD)]
    cols, _ = order.reference_order(senders, order.segment_cap(1, WORLD), order.key_hash_kind(sc), order.MAX_PARALLELISM, WORLD)
    dest = order.destinations(cols[0], order.key_hash_kind(sc), order.MAX_PARALLELISM, WORLD)
    for d in range(WORLD):
        sub = np.stack([c[dest == d] for c in cols], axis=1)
        assert (sub == res[d][1][1]).all()


def test_multirank_streams_depend_on_arrival_order():
    for name in order.SCENARIOS:
        for world, own in ((WORLD, None), (1, (2, 0))):
            rows, late, seen = order.expected(name, world, own)
            assert seen["late_drop"] >= 1 and seen["late_kept"] >= 1, (name, world, seen)
            assert late == seen["late_drop"] and seen["spill_rows"] > 0 and len(rows) > 1000


def test_in_segment_is_the_first_cap_rows_of_a_destination():
    dest = np.array([0, 1, 0, 0, 1, 0, 1], dtype=np.int32)
    assert order.in_segment(dest, 2, 2).tolist() == [True, True, True, False, True, False, False]
    assert order.in_segment(dest, 9, 2).all()
