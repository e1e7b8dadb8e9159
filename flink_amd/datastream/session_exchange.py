"""One subtask of a session-window operator of parallelism > 1 behind its keyBy exchange: the step
driver of SessionWindowOperator, DynamicSessionWindowOperator, their lateness forms
(LateSessionWindowOperator, LateDynamicSessionWindowOperator) and the SQL SessionWindowAggOperator,
as TwoPhaseWindowAgg is the two-phase plan's.

A step is one watermark interval of the subtask's input: its rows are routed by key group
(KeyByExchange.exchange_packed_async: the packed partition and all-to-all), the received padded
segments are folded in place (process_packed_segments_device), the overflow round's spill rows are
folded after them, and the valve's watermark -- the minimum over the subtasks
(StatusWatermarkValve.inputWatermark) -- fires the due sessions.

Arrival order.  A session fold depends on the order of a key's elements only where an element is
late when it arrives.  The order a destination sees in one step is: the in-segment rows sender by
sender, each sender's in its input order (the partition is a stable counting sort and the fold takes
buffer position order), then the spill rows sender by sender, then the agreed watermark.  Under the
device valve a step with overflow holds the watermark at the previous one; its spill rows land at the
start of the next step, still under the held watermark, and the agreed watermark follows them -- the
same order one step late.

Packed rows carry no NULL flags, key hashes or key rows: NOT NULL inputs and LONG / INT / BINROW keys.
"""
import numpy as np
import torch

from ..runtime.exchange import KeyByExchange


class SessionExchangeStep:
    def __init__(self, operator, exchange=None, device=None):
        """operator: an opened session operator whose configuration has parallelism > 1 (its
        subtask_index the rank of ``exchange``); exchange: the KeyByExchange of its keyBy."""
        cfg = operator.cfg
        if cfg.parallelism <= 1:
            raise ValueError("a session operator of parallelism 1 has no keyBy exchange in front of it")
        if cfg.nullable_cols:
            raise ValueError("the step moves packed rows, which carry no NULL flags: NOT NULL inputs only")
        self.op = operator
        self.exchange = exchange if exchange is not None else KeyByExchange(cfg.key_hash, cfg.max_parallelism)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.received = 0      # rows this subtask was sent (segments and spill; counted by the collecting steps)
        self._px = None        # the device-valve step whose overflow round is outstanding
        self._wm_dev = None    # its watermark (device)

    def _push_spill(self, px, spill):
        if spill is None:
            return
        n_sp = spill.numel() // px.row_words
        self.received += n_sp
        self.op.process_packed_segments_device(torch.tensor([n_sp], dtype=torch.int64, device=self.device), spill,
                                               px.row_words)

    def _exchange(self, keys, ts, values, capacity):
        px = self.exchange.exchange_packed_async(keys, ts, list(values), capacity=capacity)
        self.op.process_packed_segments_device(px.recv_counts, px.rows, px.row_words)
        return px

    def _count(self, px):
        self.received += int(px.recv_counts.clamp(max=px._cap).sum())

    def _advance(self, watermark, collect):
        if collect:
            return self.op.process_watermark(watermark)
        self.op.handle.advance(watermark)
        return None

    def step(self, keys, ts, values, watermark, capacity=None, collect=True):
        """The host valve: exchange, packed push, PackedExchange.finish (the overflow round and the
        valve in one host all-reduce), spill push, advance.  ``values``: the operator's value columns
        (a dynamic-gap operator's: the field, then the gap).  Returns (the agreed watermark, the
        fired rows in the operator's usual order -- None with ``collect`` off: the rows stay in the
        handle)."""
        px = self._exchange(keys, ts, values, capacity)
        spill, wm = px.finish(watermark)
        self._count(px)
        self._push_spill(px, spill)
        return wm, self._advance(wm, collect)

    def step_device_valve(self, keys, ts, values, watermark, capacity=None, collect=True):
        """The device valve: the previous step is settled first (one step late), then exchange, packed
        push, PackedExchange.finish_device (one device all-reduce; the watermark stays in device
        memory) and process_watermark_device.  No host wait on this step's GPU work except collecting
        the fired rows.  Returns (the valve's watermark as a one-element device tensor -- the
        previous one if any subtask overflowed --, the fired rows).  Call settle() after the last
        step."""
        fired = self.settle(collect)
        px = self._exchange(keys, ts, values, capacity)
        wm = px.finish_device(watermark, self._wm_dev)
        self._px, self._wm_dev = px, wm
        if not collect:  # nothing waits: not for the rows, not for the received counts
            self.op.handle.advance_device(wm)
            return wm, None
        res = self.op.process_watermark_device(wm)
        self._count(px)
        return wm, _concat(fired, res)

    def settle(self, collect=True):
        """The previous device-valve step's overflow round: its spill rows are folded under the
        watermark that step held, then the watermark it agreed on is issued (a lower or equal one
        changes nothing, so a step without overflow is a no-op here).  Returns the rows that fires,
        or None if no step is outstanding."""
        px, self._px = self._px, None
        if px is None:
            return None
        self._push_spill(px, px.settle())
        # every subtask advances, also one that received no spill rows: the valve held the watermark for all
        return self._advance(px.agreed_watermark, collect)


def _concat(a, b):
    """Two result dicts of one operator, a's rows first (None: no rows)."""
    if a is None:
        return b
    if b is None:
        return a
    out = {}
    for k, v in b.items():
        if isinstance(v, list):
            out[k] = [np.concatenate([x, y]) for x, y in zip(a[k], v)]
        else:
            out[k] = np.concatenate([np.asarray(a[k]), np.asarray(v)])
    return out
