"""GPU-backed drop-in for keyBy(...).window(EventTimeSessionWindows.withGap(gap)) on its eligible
subset.

WindowOperatorBuilder would return this operator iff the assigner is EventTimeSessionWindows with a
static gap, the trigger the default EventTimeTrigger, no evictor, allowedLateness 0, and the
function a built-in field aggregation sum / min / max (SumAggregator / ComparableAggregator) or a
count on a LONG / INT / DOUBLE field of (key, field) tuples.  Other triggers, evictors and minBy /
maxBy stay on the reference operator; dynamic gaps and an allowed lateness have operators of their
own (dynamic_session_window_operator.DynamicSessionWindowOperator,
late_session_window_operator.LateSessionWindowOperator, and for both together
late_dynamic_session_window_operator.LateDynamicSessionWindowOperator).

Semantics (WindowOperator.processElement's merging branch, MergingWindowSet.addWindow,
TimeWindow.intersects / mergeWindows, EventTimeTrigger): an element's window [ts, ts + gap) and
every session of its key that it intersects -- touching counts -- become one session; an element
whose window is late and intersects no session of its key when it arrives is dropped (or goes to
the late side output).  A watermark W fires every session with end - 1 <= W once, as
(key, aggregate) with timestamp end - 1, and clears it.
"""
import numpy as np

from .. import abi
from .session_operator_base import _AGG, _KEY, _TYPE, MAX_GAP, SessionOperatorBase, _common_eligibility  # noqa: F401
from .windowing import EventTimeSessionWindows, EventTimeTrigger


def is_gpu_eligible(assigner, trigger, aggregation, *, evictor=None, allowed_lateness=0, conf=None):
    """WindowOperatorBuilder's seam for session windows.  ``conf``: the job configuration
    (``gpu.window-agg.enabled``); None = the GPU operator was chosen."""
    return _common_eligibility(
        assigner, EventTimeSessionWindows,
        "assigner is not EventTimeSessionWindows with a static gap (dynamic gaps stay on the reference operator)",
        trigger, aggregation, evictor=evictor, conf=conf,
        lateness_refusal=None if allowed_lateness == 0 else
        "allowedLateness > 0 needs late re-fires of merged windows (late_session_window_operator.LateSessionWindowOperator)",
        gap=getattr(assigner, "gap", 0), gap_refusal="session gap must be in (0, 2^40]")


class SessionWindowOperator(SessionOperatorBase):
    def __init__(self, gap_ms, aggregation=("sum", "LONG"), key_type="LONG", late_side_output=False, max_parallelism=128,
                 parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16, max_batch_rows=1 << 20,
                 output_capacity=1 << 20):
        ok, why = is_gpu_eligible(EventTimeSessionWindows.with_gap(gap_ms), EventTimeTrigger.create(), aggregation)
        if not ok:
            raise ValueError(f"not eligible for the GPU session-window operator: {why}")
        fn, ftype = aggregation
        t = _TYPE[ftype]
        self.gap = gap_ms
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=gap_ms, aggs=[(_AGG[fn], 0, t)], count_star_index=-1,
            value_col_types=[t], key_hash=_KEY[key_type], late_side_output=late_side_output, max_parallelism=max_parallelism,
            parallelism=parallelism, subtask_index=subtask_index, device=device, state_capacity=state_capacity,
            max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self._init_common(aggregation, key_type)

    def process_batch(self, keys, timestamps, values, key_hashes=None):
        """processElement for a batch of (key, field) elements with their timestamps, in arrival
        order.  A STRING-keyed operator takes its keys as Python strings."""
        self._push_host(keys, timestamps, [np.asarray(values)], key_hashes)

    def process_batch_device(self, keys, timestamps, values, key_hashes=None):
        self._push_device(keys, timestamps, [values], key_hashes)

    def process_segments_device(self, seg_counts, keys, timestamps, values, key_hashes=None):
        """A padded exchange receive buffer of SoA columns (KeyByExchange.exchange_padded): segment s
        holds its first min(seg_counts[s], segment length) rows; arrival order is buffer position
        order.  A late record's ``row`` is its position in the buffer."""
        self._push_segments(seg_counts, keys, timestamps, [values], key_hashes)
