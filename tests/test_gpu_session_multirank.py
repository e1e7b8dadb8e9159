"""Session windows behind the N > 1 keyBy exchange across real ranks: two spawned processes, one
operator subtask each (parallelism 2, maxParallelism 128), a gloo process group, both on the one
GPU of the box -- the pattern of test_gpu_multirank.py.

Every rank drives its subtask with SessionExchangeStep (flink_amd/datastream/session_exchange.py):
  * host valve: exchange_packed_async -> fw_push_device_packed_segments -> PackedExchange.finish ->
    the spill push -> fw_advance;
  * device valve: finish_device -> fw_advance_device, the spill rows and the held watermark settled
    one step late.
Odd steps use segments of a quarter of the even share, so the overflow round runs; the ranks propose
different watermarks and the valve takes their minimum.

A session fold depends on the arrival order of rows that are late when they arrive, so the expected
value is ONE unsharded reference (session_window_reference.py, dynamic_session_reference.py,
sql_session_reference.py) fed in the order the destinations see the rows
(tests/session_exchange_order.py, checked against the exchange on CPU by
test_session_exchange_order.py): all values are integers, so everything is compared bit-exact.

The one-rank scenario runs the same step over the nccl backend (RCCL) with force_collectives: the
handle is subtask 0 of parallelism 2 and the stream holds only its key groups' keys.
"""
import os
import socket

import numpy as np
import pytest

import session_exchange_order as order

pytestmark = pytest.mark.gpu

WORLD = 2


def _operator(sc, subtask):
    kw = dict(max_parallelism=order.MAX_PARALLELISM, parallelism=2, subtask_index=subtask, state_capacity=1 << 14,
              max_batch_rows=4096, output_capacity=1 << 16)
    if sc["kind"] == "ds":
        from flink_amd.datastream import SessionWindowOperator
        return SessionWindowOperator(order.GAP, sc["aggregation"], **kw)
    if sc["kind"] == "dyn":
        from flink_amd.datastream import DynamicSessionWindowOperator
        return DynamicSessionWindowOperator(order.GAP, sc["aggregation"], **kw)
    from flink_amd.table.session_window_agg import SessionWindowAggOperator
    return SessionWindowAggOperator(order.GAP, sc["aggs"], sc["value_types"], **kw)


def _rows(op, sc, res):
    if res is None:
        return []
    if sc["kind"] == "sql":
        return op.output_rows(res)
    return [(int(k), int(v), int(s), int(e)) for k, v, s, e in zip(res["key"], res["value"], res["window_start"],
                                                                   res["window_end"])]


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
        from flink_amd.datastream import SessionExchangeStep
        from flink_amd.runtime.exchange import KeyByExchange

        sc = order.SCENARIOS[name]
        own = (2, 0) if world == 1 else None   # one rank: subtask 0 of 2, its own key groups' keys only
        op = _operator(sc, rank).open()
        ex = KeyByExchange(order.key_hash_kind(sc), order.MAX_PARALLELISM, force_collectives=backend == "nccl")
        drv = SessionExchangeStep(op, ex, dev)
        rows, wms = [], []
        for b in range(order.N_BATCHES):
            cols = [torch.from_numpy(c).to(dev) for c in order.stream(sc, rank, b, own=own)]
            cap = order.segment_cap(b, world)
            if valve == "device":
                wm, res = drv.step_device_valve(cols[0], cols[1], cols[2:], order.proposed_wm(b, rank), capacity=cap)
                wms.append(int(wm.item()))  # (the test reads it back; the step itself never waits for it)
            else:
                wm, res = drv.step(cols[0], cols[1], cols[2:], order.proposed_wm(b, rank), capacity=cap)
                wms.append(wm)
            rows += _rows(op, sc, res)
        if valve == "device":
            rows += _rows(op, sc, drv.settle())
        rows += _rows(op, sc, op.process_watermark(order.FINAL_WM))
        st = op.handle.stats()
        op.close()
        torch.cuda.synchronize()
        out_q.put((rank, dict(rows=rows, wms=wms, received=drv.received, spill_rounds=ex.spill_rounds,
                              backend=dist.get_backend(), collectives=ex.collectives,
                              late=st["num_late_records_dropped"], err=st["error_flags"])))
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


def _check(name, valve, res, world, own):
    sc = order.SCENARIOS[name]
    wms = res[0]["wms"]
    assert all(res[r]["wms"] == wms for r in range(world))
    agreed = [order.proposed_wm(b, 0) for b in range(order.N_BATCHES)]
    if valve == "device":  # held at the previous watermark while an overflow round is outstanding
        held = [b for b in range(order.N_BATCHES) if wms[b] != agreed[b]]
        assert held and all(wms[b] == (wms[b - 1] if b else -(1 << 63)) for b in held)
    else:
        assert wms == agreed
    assert all(res[r]["err"] == 0 for r in range(world))
    assert res[0]["spill_rounds"] > 0 and all(res[r]["spill_rounds"] == res[0]["spill_rounds"] for r in range(world))
    n_sent = sum(len(order.stream(sc, r, b, own=own)[0]) for r in range(world) for b in range(order.N_BATCHES))
    assert sum(res[r]["received"] for r in range(world)) == n_sent   # every row arrived exactly once
    for r in range(world):  # each rank emitted only keys of its own key-group range (of parallelism 2)
        lo, hi = (r * order.MAX_PARALLELISM + 1) // 2, ((r + 1) * order.MAX_PARALLELISM - 1) // 2
        kgs = order.key_groups(np.array([row[0] for row in res[r]["rows"]], dtype=np.int64), order.key_hash_kind(sc),
                               order.MAX_PARALLELISM, 2)
        assert len(kgs) and lo <= int(kgs.min()) and int(kgs.max()) <= hi, f"rank {r}: foreign key group"
    want, late, seen = order.expected(name, world, own)
    assert seen["late_drop"] >= 1 and seen["late_kept"] >= 1   # the arrival order matters on this stream
    got = [row for r in range(world) for row in res[r]["rows"]]
    assert len(want) > 1000 and sorted(got) == sorted(want)
    assert sum(res[r]["late"] for r in range(world)) == late


@pytest.mark.timeout(300)
@pytest.mark.parametrize("valve", ["host", "device"])
@pytest.mark.parametrize("name", sorted(order.SCENARIOS))
def test_two_ranks_union_equals_unsharded_reference(name, valve):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks(name, valve)
    _check(name, valve, res, WORLD, None)


@pytest.mark.timeout(300)
def test_rccl_single_rank_session_step_equals_reference():
    """RCCL does not put two ranks on one device: one rank over the nccl backend, force_collectives
    keeping the all-to-all, the device valve's all-reduce and the overflow round's all-to-all."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks("ds_sum", "device", world=1, backend="nccl")
    assert res[0]["backend"] == "nccl" and res[0]["collectives"]
    _check("ds_sum", "device", res, 1, (2, 0))
