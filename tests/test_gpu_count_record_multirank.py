"""Record-shaped count windows behind the N > 1 keyBy exchange across real ranks: two spawned processes,
one operator subtask each (parallelism 2, maxParallelism 128), a gloo process group, both on the one
GPU of the box -- the pattern of test_gpu_count_multirank.py.

Every rank drives its subtask with RecordCountExchangeStep (flink_amd/datastream/record_count_exchange.py):
the record's four fields travel as the packed row, the received segments and the spill rows are folded
where they land (fw_push_device_count_record_packed_segments) and the records the operator needs are
gathered on the device (fw_count_record_rows).  Both valves run; odd steps use segments of a quarter of
the even share, so the overflow round runs.

The expected value is ONE unsharded CountRecordReference fed, step by step, every destination's records
in the order that destination sees them (session_exchange_order.destination_sequence).  A key has one
destination, so the reference's rows for a rank's keys, in emission order, are that rank's records in
emission order.  Records compare bit for bit (record_image: the weight field holds NaNs with payloads);
the ordinals are the subtask's own (buffer positions) and are only checked to be strictly increasing
triggers that never precede their record.

The one-rank scenario runs the same step over the nccl backend (RCCL) with force_collectives.
"""
import os
import socket

import numpy as np
import pytest
from count_record_reference import CountRecordReference, double_of, record_image

import session_exchange_order as order
from flink_amd import abi

pytestmark = pytest.mark.gpu

WORLD = 2
N_BATCHES, N_ROWS = 6, 2000
HOT = 7 * 7919 + 13
SCENARIOS = {"sum_int_250_150": (250, 150, ("sum", "INT")), "minby_last_5_3": (5, 3, ("minBy", "LONG", False))}
FIELD = 1
KIND = abi.KEYHASH_LONG
T0 = 1_600_000_000_000
WEIGHTS = [0x7FF80000000ABCDE, 0x7FF00000DEADBEEF, -(1 << 63), 0]


def record_types(name):
    return ["LONG", SCENARIOS[name][2][1], "LONG", "DOUBLE"]


def stream(name, rank, batch, own=None):
    """Rank ``rank``'s slice of batch ``batch``: the columns (key, field, tag, weight bits) over 60 keys,
    30 % of the rows the one hot key.  The field: INT values whose sums wrap, or LONG values from
    [-3, 4) (ties).  The tag names the row: rank, batch, index.
    ``own`` = (parallelism, subtask): only the keys of that subtask's key groups."""
    rng = np.random.default_rng(104729 * batch + 31 * rank + 7)
    k = rng.integers(0, 60, N_ROWS).astype(np.int64) * 7919 + 13
    k[rng.random(N_ROWS) < 0.3] = HOT
    if SCENARIOS[name][2][1] == "INT":
        v = rng.integers(-2**31, 2**31, N_ROWS).astype(np.int64)
    else:
        v = rng.integers(-3, 4, N_ROWS).astype(np.int64)
    tag = (rank * 100 + batch) * 10**6 + np.arange(N_ROWS, dtype=np.int64)
    w = np.where(np.arange(N_ROWS) % 3 == 0, (np.arange(N_ROWS) * 0.25 - batch).view(np.int64),
                 np.array(WEIGHTS, np.int64)[np.arange(N_ROWS) % len(WEIGHTS)])
    cols = [k, v, tag, w]
    if own is not None:
        m = order.destinations(k, KIND, order.MAX_PARALLELISM, own[0]) == own[1]
        cols = [c[m] for c in cols]
    return tuple(cols)


def records_of(cols):
    k, v, tag, w = (c.tolist() for c in cols)
    return [(a, b, c, double_of(d)) for a, b, c, d in zip(k, v, tag, w)]


def proposed_wm(batch, rank):
    return T0 + batch * 1000 + 300 * rank   # the valve's minimum is rank 0's


def segment_cap(batch, world):
    return int(N_ROWS / world * 1.25) + 1024 if batch % 2 == 0 else N_ROWS // (4 * world)


def _worker(rank, port, name, valve, out_q, world=WORLD, backend="gloo"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        from flink_amd.datastream import RecordCountExchangeStep, RecordCountWindowOperator
        from flink_amd.runtime.exchange import KeyByExchange

        size, slide, agg = SCENARIOS[name]
        own = (2, 0) if world == 1 else None   # one rank: subtask 0 of 2, its own key groups' keys only
        op = RecordCountWindowOperator(size, slide, agg, field=FIELD, record_types=record_types(name),
                                       max_parallelism=order.MAX_PARALLELISM, parallelism=2, subtask_index=rank,
                                       state_capacity=1 << 12, max_batch_rows=8192, output_capacity=1 << 16).open()
        ex = KeyByExchange(KIND, order.MAX_PARALLELISM, force_collectives=backend == "nccl")
        drv = RecordCountExchangeStep(op, ex, dev)
        rows, trig, rord = [], [], []

        def take(res):
            if res is not None:
                rows.extend(zip(res["key"], [record_image(r) for r in res["records"]]))
                trig.extend(res["trigger_ord"].tolist())
                rord.extend(res["record_ord"].tolist())

        for b in range(N_BATCHES):
            cols = [torch.from_numpy(c).to(dev) for c in stream(name, rank, b, own=own)]
            cols[3] = cols[3].view(torch.float64)   # the weight travels as a DOUBLE column
            cap = segment_cap(b, world)
            step = drv.step_device_valve if valve == "device" else drv.step
            take(step(cols[0], cols, proposed_wm(b, rank), capacity=cap)[1])
        if valve == "device":
            take(drv.settle())
        refused = ""
        try:
            drv.step(cols[0], cols, 0, collect=False)
        except ValueError as e:
            refused = str(e)
        st = op.handle.stats()
        held = len(op.retained_ordinals())
        op.close()
        torch.cuda.synchronize()
        out_q.put((rank, dict(rows=rows, trig=trig, rord=rord, received=drv.received, spill_rounds=ex.spill_rounds,
                              backend=dist.get_backend(), collectives=ex.collectives, wm=st["current_watermark"],
                              err=st["error_flags"], refused=refused, held=held)))
    except Exception as e:  # reported to the parent, which fails the test with it
        import traceback
        out_q.put((rank, dict(error=f"{type(e).__name__}: {e}\n{traceback.format_exc()}")))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(name, valve, world=WORLD, backend="gloo"):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, name, valve, q, world, backend)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=180) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert "error" not in res[r], f"rank {r}: {res[r]['error']}"
    for p in procs:
        assert p.exitcode == 0
    return res


def _expected(name, world, own):
    """per destination: the records of one unsharded reference for that destination's keys, in emission
    order, and how many records it must hold at the end; and the number of spill rows"""
    size, slide, agg = SCENARIOS[name]
    ref = CountRecordReference(size, slide, agg, field=FIELD)
    want = [[] for _ in range(world)]
    n_spill = n = 0
    for b in range(N_BATCHES):
        senders = [stream(name, r, b, own=own) for r in range(world)]
        cap = segment_cap(b, world)
        n_spill += order.reference_order(senders, cap, KIND, order.MAX_PARALLELISM, world)[1]
        for d in range(world):
            cols = order.destination_sequence(senders, cap, d, KIND, order.MAX_PARALLELISM, world)
            recs = records_of(cols)
            want[d] += [(k, record_image(r)) for k, r, _, _ in ref.process(cols[0].tolist(), recs, range(n, n + len(recs)))]
            n += len(recs)
    return want, n_spill, len(ref.held())


def _check(name, res, world, own):
    assert all(res[r]["err"] == 0 for r in range(world))
    assert res[0]["spill_rounds"] > 0 and all(res[r]["spill_rounds"] == res[0]["spill_rounds"] for r in range(world))
    n_sent = sum(len(stream(name, r, b, own=own)[0]) for r in range(world) for b in range(N_BATCHES))
    assert sum(res[r]["received"] for r in range(world)) == n_sent   # every row arrived exactly once
    want, n_spill, n_held = _expected(name, world, own)
    assert n_spill > 0
    for r in range(world):
        t = res[r]["trig"]
        assert t == sorted(t) and len(set(t)) == len(t) and all(o <= x for o, x in zip(res[r]["rord"], t))
        assert len(want[r]) > 20 and res[r]["rows"] == want[r], f"rank {r}"
        assert res[r]["wm"] == proposed_wm(N_BATCHES - 1, 0)        # the valve's minimum travelled
        assert "collect=False" in res[r]["refused"]
    assert sum(res[r]["held"] for r in range(world)) == n_held
    hot_dest = int(order.destinations(np.array([HOT]), KIND, order.MAX_PARALLELISM, 2)[0])
    if hot_dest < world:
        assert sum(1 for row in want[hot_dest] if row[0] == HOT) > 20


@pytest.mark.timeout(300)
@pytest.mark.parametrize("valve", ["host", "device"])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_two_ranks_equal_the_unsharded_reference(name, valve):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check(name, _run_ranks(name, valve), WORLD, None)


@pytest.mark.timeout(300)
def test_rccl_single_rank_record_step_equals_reference():
    """RCCL does not put two ranks on one device: one rank over the nccl backend, force_collectives
    keeping the all-to-all, the device valve's all-reduce and the overflow round's all-to-all.
    The stream holds subtask 0's keys only and the hot key is subtask 1's, so countWindow(250, 150)
    would fire six times in the whole run; countWindow(5, 3) fires over a thousand."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks("minby_last_5_3", "device", world=1, backend="nccl")
    assert res[0]["backend"] == "nccl" and res[0]["collectives"]
    _check("minby_last_5_3", res, 1, (2, 0))
