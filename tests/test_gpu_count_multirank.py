"""Count windows behind the N > 1 keyBy exchange across real ranks: two spawned processes, one
operator subtask each (parallelism 2, maxParallelism 128), a gloo process group, both on the one
GPU of the box -- the pattern of test_gpu_session_multirank.py.

Every rank drives its subtask with CountExchangeStep (flink_amd/datastream/count_exchange.py):
  * host valve: exchange_packed_async (zero ts column) -> fw_push_device_count_packed_segments ->
    PackedExchange.finish -> the spill push -> fw_advance;
  * device valve: finish_device -> fw_advance_device, the spill rows settled one step late.
Odd steps use segments of a quarter of the even share, so the overflow round runs.

Arrival order is the whole semantics of a count window, so the expected value is ONE unsharded
CountWindowReference fed, step by step, every destination's rows in the order that destination sees
them (session_exchange_order.destination_sequence: the segments sender by sender, then the spills).
A key has one destination, so the reference's rows for a rank's keys, in emission order, are that
rank's rows in trigger_ord order -- under both valves: the watermark only travels.  Sums are INT sums
of values that wrap, everything is compared bit-exact.

The one-rank scenario runs the same step over the nccl backend (RCCL) with force_collectives: the
handle is subtask 0 of parallelism 2 and the stream holds only its key groups' keys.
"""
import os
import socket

import numpy as np
import pytest
from count_window_reference import CountWindowReference

import session_exchange_order as order
from flink_amd import abi

pytestmark = pytest.mark.gpu

WORLD = 2
N_BATCHES, N_ROWS = 6, 4000
HOT = 7 * 7919 + 13
SCENARIOS = {"sliding_250_150": (250, 150), "tumbling_4": (4, None)}
AGG = ("sum", "INT")
KIND = abi.KEYHASH_LONG
T0 = 1_600_000_000_000


def stream(rank, batch, own=None):
    """Rank ``rank``'s slice of batch ``batch``: (keys, values) over 60 keys, so that every key fires
    countWindow(250, 150) several times; 30 % of the rows are the one hot key.
    ``own`` = (parallelism, subtask): only the keys of that subtask's key groups."""
    rng = np.random.default_rng(104729 * batch + 31 * rank + 7)
    k = rng.integers(0, 60, N_ROWS).astype(np.int64) * 7919 + 13
    k[rng.random(N_ROWS) < 0.3] = HOT
    v = rng.integers(-2**31, 2**31, N_ROWS).astype(np.int64)
    if own is not None:
        m = order.destinations(k, KIND, order.MAX_PARALLELISM, own[0]) == own[1]
        k, v = k[m], v[m]
    return k, v


def proposed_wm(batch, rank):
    return T0 + batch * 1000 + 300 * rank   # the valve's minimum is rank 0's


def segment_cap(batch, world):
    return int(N_ROWS / world * 1.25) + 1024 if batch % 2 == 0 else N_ROWS // (4 * world)


def _rows(res):
    if res is None:
        return []
    return list(zip(res["key"].tolist(), res["value"].tolist(), res["window_start"].tolist(), res["window_end"].tolist()))


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
        from flink_amd.datastream import CountExchangeStep, CountWindowOperator
        from flink_amd.runtime.exchange import KeyByExchange

        size, slide = SCENARIOS[name]
        own = (2, 0) if world == 1 else None   # one rank: subtask 0 of 2, its own key groups' keys only
        op = CountWindowOperator(size, slide, AGG, max_parallelism=order.MAX_PARALLELISM, parallelism=2, subtask_index=rank,
                                 state_capacity=1 << 12, max_batch_rows=4096, output_capacity=1 << 16).open()
        ex = KeyByExchange(KIND, order.MAX_PARALLELISM, force_collectives=backend == "nccl")
        drv = CountExchangeStep(op, ex, dev)
        rows, ords = [], []

        def take(res):
            if res is not None:
                rows.extend(_rows(res))
                ords.extend(res["trigger_ord"].tolist())

        for b in range(N_BATCHES):
            k, v = (torch.from_numpy(c).to(dev) for c in stream(rank, b, own=own))
            cap = segment_cap(b, world)
            if valve == "device":
                _, res = drv.step_device_valve(k, v, proposed_wm(b, rank), capacity=cap)
            else:
                _, res = drv.step(k, v, proposed_wm(b, rank), capacity=cap)
            take(res)
        if valve == "device":
            take(drv.settle())
        st = op.handle.stats()
        op.close()
        torch.cuda.synchronize()
        out_q.put((rank, dict(rows=rows, ords=ords, received=drv.received, spill_rounds=ex.spill_rounds,
                              backend=dist.get_backend(), collectives=ex.collectives, wm=st["current_watermark"],
                              err=st["error_flags"])))
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
    """per destination: the rows of one unsharded reference for that destination's keys, in emission
    order; and the number of spill rows"""
    size, slide = SCENARIOS[name]
    ref = CountWindowReference(size, slide, AGG)
    want = [[] for _ in range(world)]
    n_spill = 0
    for b in range(N_BATCHES):
        senders = [stream(r, b, own=own) for r in range(world)]
        cap = segment_cap(b, world)
        n_spill += order.reference_order(senders, cap, KIND, order.MAX_PARALLELISM, world)[1]
        for d in range(world):
            k, v = order.destination_sequence(senders, cap, d, KIND, order.MAX_PARALLELISM, world)
            want[d] += [r[:4] for r in ref.process(k.tolist(), v.tolist())]
    return want, n_spill


def _check(name, res, world, own):
    assert all(res[r]["err"] == 0 for r in range(world))
    assert res[0]["spill_rounds"] > 0 and all(res[r]["spill_rounds"] == res[0]["spill_rounds"] for r in range(world))
    n_sent = sum(len(stream(r, b, own=own)[0]) for r in range(world) for b in range(N_BATCHES))
    assert sum(res[r]["received"] for r in range(world)) == n_sent   # every row arrived exactly once
    want, n_spill = _expected(name, world, own)
    assert n_spill > 0
    for r in range(world):
        assert res[r]["ords"] == sorted(res[r]["ords"]) and len(set(res[r]["ords"])) == len(res[r]["ords"])
        assert len(want[r]) > 20 and res[r]["rows"] == want[r], f"rank {r}"
        assert res[r]["wm"] == proposed_wm(N_BATCHES - 1, 0)        # the valve's minimum travelled
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
def test_rccl_single_rank_count_step_equals_reference():
    """RCCL does not put two ranks on one device: one rank over the nccl backend, force_collectives
    keeping the all-to-all, the device valve's all-reduce and the overflow round's all-to-all."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks("sliding_250_150", "device", world=1, backend="nccl")
    assert res[0]["backend"] == "nccl" and res[0]["collectives"]
    _check("sliding_250_150", res, 1, (2, 0))
