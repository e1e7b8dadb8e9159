"""One subtask of a count-window operator (countWindow) of parallelism > 1 behind its keyBy
exchange: the step driver of CountWindowOperator, as SessionExchangeStep is the session operators'.

A step is one batch of the subtask's input: its rows are routed by key group
(KeyByExchange.exchange_packed_async with a zero ts column: the packed partition and all-to-all),
the received padded segments are folded in place (process_packed_segments_device), the overflow
round's spill rows are folded after them as a one-segment push, and the valve's watermark is
recorded.

Arrival order is the whole semantics of a count window: a key's n-th element fires.  The order a
destination sees in one step is: the in-segment rows sender by sender, each sender's in its input
order (the partition is a stable counting sort and the fold takes buffer position order), then the
spill rows sender by sender.  Flink fixes no order between input channels, so this is a valid one.
The watermark only travels: CountTrigger.onEventTime continues, so it changes no result, and the
device valve -- whose spill rows settle one step late, in front of the next step's rows -- gives a
destination the same row sequence as the host valve.

Packed rows carry no key hashes: LONG / INT keys.  The ts word of a row is sent as zero and never read.
"""
import torch

from .. import abi
from .session_exchange import SessionExchangeStep


class CountExchangeStep(SessionExchangeStep):
    def __init__(self, operator, exchange=None, device=None):
        """operator: an opened CountWindowOperator whose configuration has parallelism > 1 (its
        subtask_index the rank of ``exchange``); exchange: the KeyByExchange of its keyBy."""
        cfg = operator.cfg
        if cfg.parallelism <= 1:
            raise ValueError("a count operator of parallelism 1 has no keyBy exchange in front of it")
        if cfg.key_hash == abi.KEYHASH_PRECOMPUTED:
            raise ValueError("the step moves packed rows, which carry no key hashes: LONG / INT keys only")
        super().__init__(operator, exchange, device)

    def _exchange(self, keys, values, capacity):
        px = self.exchange.exchange_packed_async(keys, torch.zeros_like(keys), [values], capacity=capacity)
        self.op.process_packed_segments_device(px.recv_counts, px.rows, px.row_words)
        return px

    def _advance(self, watermark, collect):
        self.op.handle.advance(watermark)  # recorded; nothing fires on a watermark
        return self.op.collect() if collect else None

    def step(self, keys, values, watermark, capacity=None, collect=True):
        """The host valve: exchange, packed push, PackedExchange.finish (the overflow round and the
        valve in one host all-reduce), spill push, advance.  ``values``: the operator's value column
        (any int64 / float64 column for a count).  Returns (the agreed watermark, the rows fired since
        the last collection in emission order -- None with ``collect`` off: the rows stay in the
        handle)."""
        px = self._exchange(keys, values, capacity)
        spill, wm = px.finish(watermark)
        self._count(px)
        self._push_spill(px, spill)
        return wm, self._advance(wm, collect)

    def step_device_valve(self, keys, values, watermark, capacity=None, collect=True):
        """The device valve: the previous step's overflow round is settled first (its spill rows go in
        one step late, in front of this step's rows), then exchange, packed push,
        PackedExchange.finish_device (one device all-reduce; the watermark stays in device memory)
        and process_watermark_device.  No host wait on this step's GPU work except collecting the
        fired rows.  Returns (the valve's watermark as a one-element device tensor, the rows fired
        since the last collection in emission order).  Call settle() after the last step."""
        self.settle(collect=False)  # its rows are collected below, with this step's: one emission order
        px = self._exchange(keys, values, capacity)
        wm = px.finish_device(watermark, self._wm_dev)
        self._px, self._wm_dev = px, wm
        self.op.process_watermark_device(wm)
        if not collect:  # nothing waits: not for the rows, not for the received counts
            return wm, None
        self._count(px)
        return wm, self.op.collect()
