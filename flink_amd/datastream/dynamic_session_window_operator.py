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
import json
import struct

import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from .count_window_operator import StringKeyTable
from .windowing import DynamicEventTimeSessionWindows, EventTimeTrigger

MAX_GAP = 1 << 40
GAP_MESSAGE = "Dynamic session time gap must satisfy 0 < gap"   # the reference's IllegalArgumentException
_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_KEY = {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT, "HOST_HASHED": abi.KEYHASH_PRECOMPUTED,
        "STRING": abi.KEYHASH_PRECOMPUTED}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def is_gpu_eligible(assigner, trigger, aggregation, *, max_gap=MAX_GAP, evictor=None, allowed_lateness=0, conf=None):
    """WindowOperatorBuilder's seam for dynamic-gap session windows.  ``max_gap``: the largest gap the
    job's extractor returns; ``conf``: the job configuration (``gpu.window-agg.enabled``); None = the
    GPU operator was chosen."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    if not isinstance(assigner, DynamicEventTimeSessionWindows):
        return False, "assigner is not DynamicEventTimeSessionWindows (EventTimeSessionWindows.withDynamicGap)"
    if not isinstance(trigger, EventTimeTrigger):
        return False, "trigger is not EventTimeTrigger"
    if evictor is not None:
        return False, "session windows with an evictor stay on the reference operator"
    if allowed_lateness != 0:
        return False, "allowedLateness > 0 needs late re-fires of merged windows (stays on the reference operator)"
    if max_gap <= 0 or max_gap > MAX_GAP:
        return False, "max_gap must be in (0, 2^40]"
    if len(aggregation) != 2 or aggregation[0] not in _AGG:
        return False, "not sum / min / max / count (minBy / maxBy stay on the reference operator)"
    if aggregation[1] not in _TYPE:
        return False, f"field type {aggregation[1]} is not LONG / INT / DOUBLE"
    return True, ""


class DynamicSessionWindowOperator:
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
        self.aggregation = aggregation
        self.key_type = key_type
        # value column 0: the aggregated field; value column 1: the element's gap
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION_DYNAMIC, size_ms=max_gap_ms, aggs=[(_AGG[fn], 0, t)],
            count_star_index=-1, value_col_types=[t, abi.T_I64], key_hash=_KEY[key_type], late_side_output=late_side_output,
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self.handle = None
        self._keys = StringKeyTable()
        self._device_pushed = False   # a device batch's gaps are checked by the kernel (FW_ERRF_GAP)

    def open(self):
        self.handle = WindowAggHandle(self.cfg)
        return self

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

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
        if self.key_type == "STRING":
            keys, key_hashes = self._keys.intern_batch(keys)
        keys = np.asarray(keys, dtype=np.int64)
        self.handle.push_host(keys, np.asarray(timestamps, dtype=np.int64), [np.asarray(values), gaps], key_hashes)

    def process_batch_device(self, keys, timestamps, values, gaps, key_hashes=None):
        """Device-resident columns (torch cuda tensors).  The kernel drops a row whose gap is outside
        (0, max_gap_ms] and raises FW_ERRF_GAP; the next process_watermark raises for it."""
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self._device_pushed = True
        self.handle.push_device(keys, timestamps, [values, gaps], key_hashes)

    # ---- behind the N > 1 keyBy exchange (parallelism > 1; a subtask of parallelism 1 has no exchange
    # in front of it and its handle refuses these)
    def process_segments_device(self, seg_counts, keys, timestamps, values, gaps, key_hashes=None):
        """A padded exchange receive buffer of SoA columns (KeyByExchange.exchange_padded): segment s
        holds its first min(seg_counts[s], segment length) rows; arrival order is buffer position
        order.  Padding rows are never read, so their gaps are not checked."""
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self._device_pushed = True
        self.handle.push_device_segments(seg_counts, keys, timestamps, [values, gaps], key_hashes)

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """A packed padded exchange receive buffer (KeyByExchange.exchange_packed_async): rows of
        (key, ts, value, gap) words."""
        self._device_pushed = True
        self.handle.push_device_packed_segments(seg_counts, rows, row_words)

    def process_watermark_device(self, wm_tensor):
        """process_watermark with the watermark in device memory (the exchange's device valve): the
        handle takes max(its watermark, wm_tensor[0]) with no host wait; the gap check and collecting
        the rows wait."""
        self._check_gaps()
        self.handle.advance_device(wm_tensor)
        return self._fired()

    def _key_objects(self, ids):
        return self._keys.objects(ids) if self.key_type == "STRING" else ids

    def _check_gaps(self):
        if self._device_pushed:
            if self.handle.stats()["error_flags"] & abi.ERRF["GAP"]:
                raise ValueError(f"{GAP_MESSAGE} (a device batch held a gap outside (0, max_gap_ms = {self.max_gap}])")
            self._device_pushed = False

    def process_watermark(self, watermark):
        """The sessions the watermark fires, sorted by (timestamp, key, window_start)."""
        self._check_gaps()
        self.handle.advance(watermark)
        return self._fired()

    def _fired(self):
        r = self.handle.results(reset=True)
        ts = r["window_end"] - 1
        order = np.lexsort((r["window_start"], r["key"], ts))
        return {"key": self._key_objects(r["key"][order]), "value": r["values"][0][order], "timestamp": ts[order],
                "window_start": r["window_start"][order], "window_end": r["window_end"][order]}

    def late_records(self):
        """The late side output since the last call (late_side_output): key, ts, value, push_seq, row
        (the element's gap is the one the caller passed at that push_seq, row)."""
        r = self.handle.late_records()
        return {"key": self._key_objects(r["key"]), "ts": r["ts"], "value": r["values"][0], "push_seq": r["push_seq"],
                "row": r["row"]}

    def snapshot_state(self) -> bytes:
        """The device blob; a STRING-keyed operator appends the Strings behind its device key ids."""
        blob = self.handle.snapshot()
        if self.key_type != "STRING":
            return blob
        return struct.pack("<q", len(blob)) + blob + json.dumps({"strings": self._keys.strings}).encode()

    def initialize_state(self, blob: bytes):
        if self.key_type != "STRING":
            self.handle.restore(blob)
            return
        n = struct.unpack_from("<q", blob, 0)[0]
        self.handle.restore(blob[8:8 + n])
        self._keys = StringKeyTable(json.loads(blob[8 + n:].decode())["strings"])

    def output_records(self, res):
        fn, ftype = self.aggregation
        vals = res["value"]
        if ftype == "DOUBLE" and fn != "count":
            vals = vals.view(np.float64)
        elif ftype == "INT" and fn != "count":
            vals = vals.astype(np.int32)
        return [(k if isinstance(k, str) else int(k), v.item(), int(t)) for k, v, t in zip(res["key"], vals, res["timestamp"])]
