"""GPU-backed drop-in for the SQL SESSION window TVF aggregate on its eligible subset:

    SELECT k, <aggs> FROM TABLE(SESSION(TABLE t PARTITION BY k, DESCRIPTOR(rowtime), gap))
    GROUP BY k, window_start, window_end

On the Table side a session query does not slice: WindowAggOperatorBuilder builds an unslicing
processor (recalled, parity unpinned -- the Flink sources are not at hand: UnsliceWindowAggProcessor
over UnsliceAssigners.SessionUnsliceAssigner, the table runtime's
MergingWindowProcessFunction.assignActualWindows / MergingFunctionImpl.merge, fired from
WindowAggOperator.processWatermark).  This operator stands at that seam for event time with a
static gap on a TIMESTAMP rowtime:

* a row with rowtime ts gets the window [ts, ts + gap) and is merged with every window of its key
  it intersects (TimeWindow.intersects is inclusive: touching windows merge); the merged
  accumulator is the aggregates' merge of the members' accumulators, then the row is accumulated;
* a row whose merged window is late (end - 1 <= currentWatermark) is dropped, counted in
  numLateRecordsDropped, and leaves the window set as it was (no side output in SQL);
* a watermark W' above the current one fires every session with end - 1 <= W' once, as
  key ++ aggs ++ (window_start, window_end), and clears it;
* a NULL value still opens or extends its session; only its aggregates skip it.

MIN / MAX over DOUBLE, TIMESTAMP_LTZ rowtimes, two-phase plans, key rows and DISTINCT / retraction
stay on the reference operator.
"""
import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from .window_agg import GPU_AGGS, GPU_TYPES, KEY_HASH

MAX_GAP = 1 << 40


def is_gpu_eligible(gap_ms, aggs, value_types, *, is_event_time=True, shift_time_zone="UTC", has_distinct=False,
                    needs_retraction=False, key_type="BIGINT", conf=None):
    """The builder-seam eligibility rule for a session window aggregate.  ``aggs``: (kind, input
    column, type) triples as for WindowAggOperator.  Returns (ok, reason); callers stay on the
    reference operator when not ok."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    if not is_event_time:
        return False, "processing-time session windows run on the reference operator"
    if shift_time_zone not in (None, "UTC"):
        return False, "TIMESTAMP_LTZ session windows (shift time zones) run on the reference operator"
    if has_distinct or needs_retraction:
        return False, "DISTINCT / retraction aggregates run on the reference operator"
    if not isinstance(gap_ms, (int, np.integer)) or gap_ms <= 0 or gap_ms > MAX_GAP:
        return False, "session gap must be a static gap in (0, 2^40] ms"
    if isinstance(key_type, (tuple, list)):
        return False, "key rows run on the reference operator for session windows"
    if key_type not in KEY_HASH:
        return False, f"key type {key_type} must be host-hashed"
    if not 1 <= len(aggs) <= abi.FW_MAX_AGGS:
        return False, f"{len(aggs)} aggregates (1 .. {abi.FW_MAX_AGGS} run on the GPU)"
    for kind, col, typ in aggs:
        if kind not in GPU_AGGS:
            return False, f"aggregate {kind} is not a built-in GPU aggregate"
        if kind != "COUNT_STAR" and (typ not in GPU_TYPES or value_types[col] != typ):
            return False, f"aggregate input type {typ} not supported on the GPU"
        if kind in ("MIN", "MAX") and typ == "DOUBLE":
            return False, f"{kind}(DOUBLE) compares strictly in arrival order and runs on the reference operator"
    return True, ""


class SessionWindowAggOperator:
    """The interface of WindowAggOperator for a session window aggregate.  A plan of more than 8
    accumulator words is refused by the library when the operator is opened."""

    def __init__(self, gap_ms, aggs, value_types, key_type="BIGINT", nullable_cols=(), count_star_index=-1,
                 max_parallelism=128, parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16,
                 max_batch_rows=1 << 20, output_capacity=1 << 20):
        ok, why = is_gpu_eligible(gap_ms, aggs, value_types, key_type=key_type)
        if not ok:
            raise ValueError(f"not eligible for the GPU session window operator: {why}")
        self.gap = int(gap_ms)
        self.aggs = list(aggs)
        self.cfg = abi.make_config(
            api=abi.API_SQL, window_kind=abi.WIN_SESSION, size_ms=self.gap,
            aggs=[(abi.AGG_NAMES[k], c, abi.TYPE_NAMES[t]) for k, c, t in aggs], count_star_index=count_star_index,
            value_col_types=[abi.TYPE_NAMES[t] for t in value_types], key_hash=KEY_HASH[key_type],
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity,
            nullable_cols=nullable_cols)
        self.handle = None
        self.current_watermark = -(1 << 63)

    # ---- AbstractStreamOperator lifecycle
    def open(self):
        self.handle = WindowAggHandle(self.cfg)
        return self

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

    # ---- OneInputStreamOperator
    def process_batch(self, keys, rowtimes, values=(), key_hashes=None, nulls=None):
        """processElement for every row of a columnar batch in arrival order (host arrays;
        ``nulls``: {column: per-row NULL flags} for the NULL-able columns).  The rows are folded
        into the sessions now, under the current watermark."""
        self.handle.push_host(keys, rowtimes, values, key_hashes, nulls=nulls)

    def process_batch_device(self, keys, rowtimes, values=(), key_hashes=None, nulls=None):
        """processElement for a batch already resident in HBM (torch cuda tensors)."""
        self.handle.push_device(keys, rowtimes, values, key_hashes, nulls=nulls)

    def process_watermark(self, watermark, collect=True):
        """processWatermark: fires every session with end - 1 <= watermark; returns the rows emitted
        for this watermark (before it is forwarded)."""
        self.handle.advance(watermark)
        if watermark > self.current_watermark:
            self.current_watermark = watermark
        if not collect:
            return None
        return self.handle.results(reset=True)

    # ---- behind the N > 1 keyBy exchange (parallelism > 1; a subtask of parallelism 1 has no exchange
    # in front of it and its handle refuses these)
    def process_segments_device(self, seg_counts, keys, rowtimes, values=(), key_hashes=None, nulls=None):
        """A padded exchange receive buffer of SoA columns (KeyByExchange.exchange_padded): segment s
        holds its first min(seg_counts[s], segment length) rows; arrival order is buffer position
        order."""
        self.handle.push_device_segments(seg_counts, keys, rowtimes, values, key_hashes, nulls=nulls)

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """A packed padded exchange receive buffer (KeyByExchange.exchange_packed_async): rows of
        (key, rowtime, value words); NOT NULL columns and device-hashable keys only."""
        self.handle.push_device_packed_segments(seg_counts, rows, row_words)

    def process_watermark_device(self, wm_tensor, collect=True):
        """processWatermark with the watermark in device memory (the exchange's device valve): the
        handle takes max(its watermark, wm_tensor[0]) with no host wait.  current_watermark follows
        at the next collect or state call."""
        self.handle.advance_device(wm_tensor)
        if not collect:
            return None
        res = self.handle.results(reset=True)
        self.current_watermark = max(self.current_watermark, self.handle.stats()["current_watermark"])
        return res

    def prepare_snapshot_pre_barrier(self, checkpoint_id=0):
        self.handle.flush()  # (nothing is buffered: every push is folded when it is pushed)

    def snapshot_state(self) -> bytes:
        return self.handle.snapshot()

    def initialize_state(self, blob: bytes):
        self.handle.restore(blob)
        self.current_watermark = self.handle.stats()["current_watermark"]

    @property
    def num_late_records_dropped(self):
        return self.handle.stats()["num_late_records_dropped"]

    def output_rows(self, res):
        """Materialise result columns as reference-shaped rows: key ++ aggs ++ (ws, we), None for NULL."""
        rows = []
        for i in range(len(res["key"])):
            vals = []
            for a, (kind, _, typ) in enumerate(self.aggs):
                if res["null_mask"][i] >> a & 1:
                    vals.append(None)
                elif abi.result_is_double(abi.AGG_NAMES[kind], abi.TYPE_NAMES[typ]):
                    vals.append(float(np.int64(res["values"][a][i]).view(np.float64)))
                else:
                    vals.append(int(res["values"][a][i]))
            rows.append((int(res["key"][i]), *vals, int(res["window_start"][i]), int(res["window_end"][i])))
        return rows
