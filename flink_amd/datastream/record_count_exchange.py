"""One subtask of a record-shaped count-window operator (countWindow emitting whole records) of
parallelism > 1 behind its keyBy exchange: the step driver of RecordCountWindowOperator, as
CountExchangeStep is CountWindowOperator's.

The record travels as the packed row itself: ``values`` is the list of the record's F field columns
(the operator's record_types), so a row is (key, zero ts word, field 0 .. field F - 1) and
row_words = 2 + F.  The received padded segments are folded where they land
(fw_push_device_count_record_packed_segments), the spill rows after them as a one-segment call of the
same entry, and after each of the two the device gathers the few record rows the operator needs
(fw_count_record_rows): the receive buffer never crosses to the host.

Arrival order and the two valves are CountExchangeStep's.  What differs: the operator drains after
every push -- a retain names a row of the buffer just pushed, which the next exchange reuses -- so a
step waits for the device once per push and ``collect=False`` is refused.  The fired records of a step
are whatever the operator's collect() returns after it.

Packed rows carry no key hashes: LONG / INT keys (no STRING keys behind the exchange).
"""
import torch

from .count_exchange import CountExchangeStep


class RecordCountExchangeStep(CountExchangeStep):
    def __init__(self, operator, exchange=None, device=None):
        """operator: an opened RecordCountWindowOperator with record_types and parallelism > 1 (its
        subtask_index the rank of ``exchange``); exchange: the KeyByExchange of its keyBy."""
        if getattr(operator, "record_types", None) is None:
            raise ValueError("the step moves records as packed rows: the operator needs record_types=[...]")
        super().__init__(operator, exchange, device)

    def _check(self, values, collect):
        if not collect:
            raise ValueError("a record count operator drains after every push (the retained records are read out of the "
                             "receive buffer before it is reused): collect=False is not available for this kind")
        if len(values) != len(self.op.record_types):
            raise ValueError(f"values: the record has {len(self.op.record_types)} fields, got {len(values)} columns")

    def _exchange(self, keys, values, capacity):
        px = self.exchange.exchange_packed_async(keys, torch.zeros_like(keys), list(values), capacity=capacity)
        self.op.process_packed_segments_device(px.recv_counts, px.rows, px.row_words)
        return px

    def step(self, keys, values, watermark, capacity=None, collect=True):
        """The host valve, as CountExchangeStep.step; ``values``: the record's F field columns.
        Returns (the agreed watermark, the records fired since the last collection in emission order)."""
        self._check(values, collect)
        return super().step(keys, values, watermark, capacity, True)

    def step_device_valve(self, keys, values, watermark, capacity=None, collect=True):
        """The device valve, as CountExchangeStep.step_device_valve: the previous step's spill rows go
        in first.  The watermark stays in device memory; the pushes' drains are the step's host waits."""
        self._check(values, collect)
        return super().step_device_valve(keys, values, watermark, capacity, True)

    def settle(self, collect=True):
        """The previous device-valve step's overflow round.  Inside a step its rows are drained into the
        operator and collected with that step's; called after the last step it returns them."""
        return super().settle(collect)
