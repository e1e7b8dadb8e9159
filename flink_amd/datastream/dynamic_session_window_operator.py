"""GPU-backed drop-in for keyBy(...).window(EventTimeSessionWindows.withDynamicGap(extractor)) on its
eligible subset.

WindowOperatorBuilder would return this operator iff the assigner is DynamicEventTimeSessionWindows,
the trigger the default EventTimeTrigger, no evictor, allowedLateness 0, and the function a built-in
field aggregation sum / min / max or a count on a LONG / INT / DOUBLE field of (key, field) tuples.
The job names the largest gap its extractor can return (``max_gap_ms``, at most 2^40): the session
gap extractor runs on the host, or in the producer of a device batch, and its result arrives as a
column beside the field.  With allowedLateness > 0 the job takes
late_dynamic_session_window_operator.LateDynamicSessionWindowOperator; this seam keeps refusing it.

Semantics (DynamicEventTimeSessionWindows.assignWindows, then the static path's
WindowOperator.processElement merging branch, MergingWindowSet.addWindow, TimeWindow.intersects /
mergeWindows, EventTimeTrigger; recalled, parity rests on tests/dynamic_session_reference.py): an
element's window is [ts, ts + g) with g = extractor.extract(element); g <= 0 throws
IllegalArgumentException("Dynamic session time gap must satisfy 0 < gap").  The window and every
session of its key that it intersects -- touching counts -- become one session; an element whose
own window is late (ts + g - 1 <= watermark) and intersects no session of its key when it arrives
is dropped (or goes to the late side output).  A watermark W fires every session with
end - 1 <= W once, as (key, aggregate) with timestamp end - 1, and clears it.
"""
import numpy as np

from .. import abi
from .session_operator_base import _AGG, _KEY, _TYPE, MAX_GAP, SessionOperatorBase, _common_eligibility  # noqa: F401
from .windowing import DynamicEventTimeSessionWindows, EventTimeTrigger

GAP_MESSAGE = "Dynamic session time gap must satisfy 0 < gap"   # the reference's IllegalArgumentException


def is_gpu_eligible(assigner, trigger, aggregation, *, max_gap=MAX_GAP, evictor=None, allowed_lateness=0, conf=None):
    """WindowOperatorBuilder's seam for dynamic-gap session windows.  ``max_gap``: the largest gap the
    job's extractor returns; ``conf``: the job configuration (``gpu.window-agg.enabled``); None = the
    GPU operator was chosen."""
    return _common_eligibility(
        assigner, DynamicEventTimeSessionWindows,
        "assigner is not DynamicEventTimeSessionWindows (EventTimeSessionWindows.withDynamicGap)",
        trigger, aggregation, evictor=evictor, conf=conf,
        lateness_refusal=None if allowed_lateness == 0 else
        "allowedLateness > 0 needs late re-fires of merged windows (stays on the reference operator)",
        gap=max_gap, gap_refusal="max_gap must be in (0, 2^40]")


class DynamicSessionWindowOperator(SessionOperatorBase):
    def __init__(self, max_gap_ms, aggregation=("sum", "LONG"), key_type="LONG", late_side_output=False, max_parallelism=128,
                 parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16, max_batch_rows=1 << 20,
                 output_capacity=1 << 20):
        ok, why = is_gpu_eligible(DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 1), EventTimeTrigger.create(),
                                  aggregation, max_gap=max_gap_ms)
        if not ok:
            raise ValueError(f"not eligible for the GPU dynamic-gap session-window operator: {why}")
        fn, ftype = aggregation
        t = _TYPE[ftype]
        self.max_gap = max_gap_ms
        # value column 0: the aggregated field; value column 1: the element's gap
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_DYNAMIC, size_ms=max_gap_ms, aggs=[(_AGG[fn], 0, t)],
            count_star_index=-1, value_col_types=[t, abi.T_I64], key_hash=_KEY[key_type], late_side_output=late_side_output,
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self._init_common(aggregation, key_type)

    def process_batch(self, keys, timestamps, values, gaps, key_hashes=None):
        """processElement for a batch of (key, field) elements with their timestamps and the gaps the
        extractor returned for them, in arrival order.  A gap <= 0 raises the reference's exception
        and one above max_gap_ms a ValueError, before anything is pushed.  A STRING-keyed operator
        takes its keys as Python strings."""
        gaps = np.asarray(gaps, dtype=np.int64)
        if len(gaps) and int(gaps.min()) <= 0:
            raise ValueError(GAP_MESSAGE)
        if len(gaps) and int(gaps.max()) > self.max_gap:
            raise ValueError(f"a session gap of {int(gaps.max())} exceeds max_gap_ms = {self.max_gap}")
        self._push_host(keys, timestamps, [np.asarray(values), gaps], key_hashes)

    def process_batch_device(self, keys, timestamps, values, gaps, key_hashes=None):
        """Device-resident columns (torch cuda tensors).  The kernel drops a row whose gap is outside
        (0, max_gap_ms] and raises FW_ERRF_GAP; the next process_watermark raises for it."""
        self._push_device(keys, timestamps, [values, gaps], key_hashes)

    def process_segments_device(self, seg_counts, keys, timestamps, values, gaps, key_hashes=None):
        """A padded exchange receive buffer of SoA columns (KeyByExchange.exchange_padded): segment s
        holds its first min(seg_counts[s], segment length) rows; arrival order is buffer position
        order.  Padding rows are never read, so their gaps are not checked."""
        self._push_segments(seg_counts, keys, timestamps, [values, gaps], key_hashes)

    def _check_gaps(self):
        if self._device_pushed:
            if self.handle.stats()["error_flags"] & abi.ERRF["GAP"]:
                raise ValueError(f"{GAP_MESSAGE} (a device batch held a gap outside (0, max_gap_ms = {self.max_gap}])")
            self._device_pushed = False
