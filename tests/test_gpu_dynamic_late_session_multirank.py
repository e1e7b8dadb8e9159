"""Dynamic-gap session windows with an allowed lateness behind the N > 1 keyBy exchange across real
ranks: two spawned processes, one LateDynamicSessionWindowOperator subtask each (parallelism 2,
maxParallelism 128), a gloo process group, both on the one GPU of the box -- the pattern and the
spawn helpers of test_gpu_session_multirank.py, in a file of its own because the workers are spawned
by module name.

Every rank drives its subtask with SessionExchangeStep under the host valve and under the device
valve; odd steps use segments of a quarter of the even share, so the overflow round runs.  The rows
are session_exchange_order's dynamic-gap stream (gaps 1 .. 150), shortened.  With a lateness the
output depends on the arrival order of every late row, so the expected value is ONE unsharded
reference (dynamic_late_session_reference.py) fed in the order tests/session_exchange_order.py gives:
the union of the ranks' rows -- timer rows and rows fired at once -- and their summed drops must
equal it, bit-exact."""
import os

import numpy as np
import pytest
from dynamic_late_session_reference import DynamicLateSessionReference

import session_exchange_order as order
import test_gpu_session_multirank as mr

pytestmark = pytest.mark.gpu

WORLD = 2
N_ROWS = 1500
LATENESS = 200
SC = order.SCENARIOS["dynamic_gap"]


def _worker(rank, port, valve, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        from flink_amd.datastream import LateDynamicSessionWindowOperator, SessionExchangeStep
        from flink_amd.runtime.exchange import KeyByExchange

        op = LateDynamicSessionWindowOperator(order.GAP, LATENESS, SC["aggregation"], max_parallelism=order.MAX_PARALLELISM,
                                              parallelism=2, subtask_index=rank, state_capacity=1 << 14, max_batch_rows=4096,
                                              output_capacity=1 << 16).open()
        ex = KeyByExchange(order.key_hash_kind(SC), order.MAX_PARALLELISM)
        drv = SessionExchangeStep(op, ex, dev)
        rows, wms = [], []
        for b in range(order.N_BATCHES):
            cols = [torch.from_numpy(c).to(dev) for c in order.stream(SC, rank, b, n=N_ROWS)]
            cap = order.segment_cap(b, WORLD, n=N_ROWS)
            if valve == "device":
                wm, res = drv.step_device_valve(cols[0], cols[1], cols[2:], order.proposed_wm(b, rank), capacity=cap)
                wms.append(int(wm.item()))
            else:
                wm, res = drv.step(cols[0], cols[1], cols[2:], order.proposed_wm(b, rank), capacity=cap)
                wms.append(wm)
            rows += mr._rows(op, SC, res)
        if valve == "device":
            rows += mr._rows(op, SC, drv.settle())
        rows += mr._rows(op, SC, op.process_watermark(order.FINAL_WM))
        st = op.handle.stats()
        op.close()
        torch.cuda.synchronize()
        out_q.put((rank, dict(rows=rows, wms=wms, received=drv.received, spill_rounds=ex.spill_rounds,
                              late=st["num_late_records_dropped"], fired=st["num_fired_windows"], err=st["error_flags"],
                              live=st["live_state_entries"])))
    except Exception as e:  # reported to the parent, which fails the test with it
        import traceback
        out_q.put((rank, dict(error=f"{type(e).__name__}: {e}\n{traceback.format_exc()}")))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run_ranks(valve):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = mr._free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, valve, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=180) for _ in range(WORLD))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(WORLD):
        assert "error" not in res[r], f"rank {r}: {res[r]['error']}"
    for p in procs:
        assert p.exitcode == 0
    return res


def _expected():
    """one unsharded reference over both senders' streams in the order their destinations see them"""
    ref = DynamicLateSessionReference(LATENESS, SC["aggregation"], max_gap=order.GAP)
    rows, n_spill = [], 0
    for b in range(order.N_BATCHES):
        senders = [order.stream(SC, r, b, n=N_ROWS) for r in range(WORLD)]
        cols, sp = order.reference_order(senders, order.segment_cap(b, WORLD, n=N_ROWS), order.key_hash_kind(SC),
                                         order.MAX_PARALLELISM, WORLD)
        n_spill += sp
        _, at_once = ref.process(cols[0].tolist(), cols[1].tolist(), cols[2].tolist(), cols[3].tolist())
        rows += at_once + ref.process_watermark(order.proposed_wm(b, 0))
    rows += ref.process_watermark(order.FINAL_WM)
    return [tuple(r) for r in rows], ref, n_spill


@pytest.mark.timeout(300)
@pytest.mark.parametrize("valve", ["host", "device"])
def test_two_ranks_union_equals_unsharded_reference(valve):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    res = _run_ranks(valve)
    wms = res[0]["wms"]
    assert all(res[r]["wms"] == wms for r in range(WORLD))
    agreed = [order.proposed_wm(b, 0) for b in range(order.N_BATCHES)]
    if valve == "device":  # held at the previous watermark while an overflow round is outstanding
        held = [b for b in range(order.N_BATCHES) if wms[b] != agreed[b]]
        assert held and all(wms[b] == (wms[b - 1] if b else -(1 << 63)) for b in held)
    else:
        assert wms == agreed
    assert all(res[r]["err"] == 0 and res[r]["live"] == 0 for r in range(WORLD))
    assert res[0]["spill_rounds"] > 0 and all(res[r]["spill_rounds"] == res[0]["spill_rounds"] for r in range(WORLD))
    assert sum(res[r]["received"] for r in range(WORLD)) == WORLD * order.N_BATCHES * N_ROWS   # every row arrived exactly once
    for r in range(WORLD):  # each rank emitted only keys of its own key-group range
        lo, hi = (r * order.MAX_PARALLELISM + 1) // 2, ((r + 1) * order.MAX_PARALLELISM - 1) // 2
        kgs = order.key_groups(np.array([row[0] for row in res[r]["rows"]], dtype=np.int64), order.key_hash_kind(SC),
                               order.MAX_PARALLELISM, 2)
        assert len(kgs) and lo <= int(kgs.min()) and int(kgs.max()) <= hi, f"rank {r}: foreign key group"
    want, ref, n_spill = _expected()
    c = ref.counts   # the arrival order matters on this stream, in every way the lateness rules know
    assert n_spill > 0 and min(c["dropped"], c["fired_at_once"], c["candidate_into_unfired"], c["ontime_into_fired"]) >= 20, c
    got = [row for r in range(WORLD) for row in res[r]["rows"]]
    assert len(want) > 1000 and sorted(got) == sorted(want)
    assert sum(res[r]["late"] for r in range(WORLD)) == ref.late_dropped
    assert sum(res[r]["fired"] for r in range(WORLD)) == ref.fired == len(want)
