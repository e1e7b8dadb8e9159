"""GPU-backed drop-in for
keyBy(...).window(EventTimeSessionWindows.withDynamicGap(extractor)).allowedLateness(L) on its
eligible subset.

WindowOperatorBuilder would return this operator iff the assigner is DynamicEventTimeSessionWindows,
the trigger the default EventTimeTrigger, no evictor, allowedLateness >= 0, and the function a
built-in field aggregation sum / min / max or a count on a LONG / INT / DOUBLE field of (key, field)
tuples.  The job names the largest gap its extractor can return (``max_gap_ms``, at most 2^40); the
gaps arrive as a column beside the field.  The SQL SESSION TVF with a lateness stays on the reference
operator.

Semantics (DynamicEventTimeSessionWindows.assignWindows, WindowOperator.processElement's merging
branch, EventTimeTrigger.onElement, cleanupTime; recalled, parity unpinned).  Lateness L, watermark W:
  * an element's window [ts, ts + g), g = extractor.extract(element) > 0, and every session of its
    key that it intersects -- touching counts -- become one session;
  * an element that intersects nothing and has ts + g - 1 + L <= W is dropped (or goes to the late
    side output): of two elements with one timestamp the one with the longer gap may stay;
  * any other element is kept, and if the session it produced has end - 1 <= W that session is
    emitted at once with the element in it.  Nothing is purged;
  * a watermark W' > W emits every session with W < end - 1 <= W' and removes every session with
    end - 1 + L <= W'.  Which held sessions have fired is read off the watermark.
``collect()`` returns the rows late elements fired since the last collection; ``process_watermark``
returns those and the timer rows.
"""
from .. import abi
from .dynamic_session_window_operator import _AGG, _KEY, _TYPE, MAX_GAP, DynamicSessionWindowOperator  # noqa: F401
from .late_session_window_operator import MAX_LATENESS
from .session_operator_base import _common_eligibility
from .windowing import DynamicEventTimeSessionWindows, EventTimeTrigger


def is_gpu_eligible(assigner, trigger, aggregation, *, max_gap=MAX_GAP, evictor=None, allowed_lateness=0, conf=None):
    """WindowOperatorBuilder's seam for dynamic-gap session windows with an allowed lateness.
    ``max_gap``: the largest gap the job's extractor returns; ``conf``: the job configuration
    (``gpu.window-agg.enabled``); None = the GPU operator was chosen."""
    return _common_eligibility(
        assigner, DynamicEventTimeSessionWindows,
        "assigner is not DynamicEventTimeSessionWindows (EventTimeSessionWindows.withDynamicGap)",
        trigger, aggregation, evictor=evictor, conf=conf,
        lateness_refusal=None if 0 <= allowed_lateness <= MAX_LATENESS else "allowedLateness must be in [0, 2^40]",
        gap=max_gap, gap_refusal="max_gap must be in (0, 2^40]")


class LateDynamicSessionWindowOperator(DynamicSessionWindowOperator):
    """DynamicSessionWindowOperator's methods (the host gap checks, _check_gaps and the segment and
    device-watermark ones included) over a FW_WIN_SESSION_DYNAMIC_LATENESS handle, and collect()."""

    def __init__(self, max_gap_ms, allowed_lateness_ms, aggregation=("sum", "LONG"), key_type="LONG", late_side_output=False,
                 max_parallelism=128, parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16,
                 max_batch_rows=1 << 20, output_capacity=1 << 20):
        ok, why = is_gpu_eligible(DynamicEventTimeSessionWindows.with_dynamic_gap(lambda e: 1), EventTimeTrigger.create(),
                                  aggregation, max_gap=max_gap_ms, allowed_lateness=allowed_lateness_ms)
        if not ok:
            raise ValueError(f"not eligible for the GPU late dynamic-gap session-window operator: {why}")
        fn, ftype = aggregation
        t = _TYPE[ftype]
        self.max_gap = max_gap_ms
        self.allowed_lateness = allowed_lateness_ms
        # value column 0: the aggregated field; value column 1: the element's gap
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_DYNAMIC_LATENESS, size_ms=max_gap_ms,
            allowed_lateness_ms=allowed_lateness_ms, aggs=[(_AGG[fn], 0, t)], count_star_index=-1,
            value_col_types=[t, abi.T_I64], key_hash=_KEY[key_type], late_side_output=late_side_output,
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self._init_common(aggregation, key_type)

    def collect(self):
        """The rows in the result buffer, without advancing: after a push, the sessions its late
        elements fired at once, sorted by (timestamp, key, window_start) -- rows of one session differ
        in their value."""
        return self._fired()
