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
import json
import struct

import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from .count_window_operator import StringKeyTable
from .windowing import EventTimeSessionWindows, EventTimeTrigger

MAX_GAP = 1 << 40
_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_KEY = {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT, "HOST_HASHED": abi.KEYHASH_PRECOMPUTED,
        "STRING": abi.KEYHASH_PRECOMPUTED}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def is_gpu_eligible(assigner, trigger, aggregation, *, evictor=None, allowed_lateness=0, conf=None):
    """WindowOperatorBuilder's seam for session windows.  ``conf``: the job configuration
    (``gpu.window-agg.enabled``); None = the GPU operator was chosen."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    if not isinstance(assigner, EventTimeSessionWindows):
        return False, "assigner is not EventTimeSessionWindows with a static gap (dynamic gaps stay on the reference operator)"
    if not isinstance(trigger, EventTimeTrigger):
        return False, "trigger is not EventTimeTrigger"
    if evictor is not None:
        return False, "session windows with an evictor stay on the reference operator"
    if allowed_lateness != 0:
        return False, "allowedLateness > 0 needs late re-fires of merged windows (late_session_window_operator.LateSessionWindowOperator)"
    if assigner.gap <= 0 or assigner.gap > MAX_GAP:
        return False, "session gap must be in (0, 2^40]"
    if len(aggregation) != 2 or aggregation[0] not in _AGG:
        return False, "not sum / min / max / count (minBy / maxBy stay on the reference operator)"
    if aggregation[1] not in _TYPE:
        return False, f"field type {aggregation[1]} is not LONG / INT / DOUBLE"
    return True, ""


class SessionWindowOperator:
    def __init__(self, gap_ms, aggregation=("sum", "LONG"), key_type="LONG", late_side_output=False, max_parallelism=128,
                 parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16, max_batch_rows=1 << 20,
                 output_capacity=1 << 20):
        ok, why = is_gpu_eligible(EventTimeSessionWindows.with_gap(gap_ms), EventTimeTrigger.create(), aggregation)
        if not ok:
            raise ValueError(f"not eligible for the GPU session-window operator: {why}")
        fn, ftype = aggregation
        t = _TYPE[ftype]
        self.gap = gap_ms
        self.aggregation = aggregation
        self.key_type = key_type
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=gap_ms, aggs=[(_AGG[fn], 0, t)], count_star_index=-1,
            value_col_types=[t], key_hash=_KEY[key_type], late_side_output=late_side_output, max_parallelism=max_parallelism,
            parallelism=parallelism, subtask_index=subtask_index, device=device, state_capacity=state_capacity,
            max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self.handle = None
        self._keys = StringKeyTable()

    def open(self):
        self.handle = WindowAggHandle(self.cfg)
        return self

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

    def process_batch(self, keys, timestamps, values, key_hashes=None):
        """processElement for a batch of (key, field) elements with their timestamps, in arrival
        order.  A STRING-keyed operator takes its keys as Python strings."""
        if self.key_type == "STRING":
            keys, key_hashes = self._keys.intern_batch(keys)
        keys = np.asarray(keys, dtype=np.int64)
        self.handle.push_host(keys, np.asarray(timestamps, dtype=np.int64), [np.asarray(values)], key_hashes)

    def process_batch_device(self, keys, timestamps, values, key_hashes=None):
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self.handle.push_device(keys, timestamps, [values], key_hashes)

    # ---- behind the N > 1 keyBy exchange (parallelism > 1; a subtask of parallelism 1 has no exchange
    # in front of it and its handle refuses these)
    def process_segments_device(self, seg_counts, keys, timestamps, values, key_hashes=None):
        """A padded exchange receive buffer of SoA columns (KeyByExchange.exchange_padded): segment s
        holds its first min(seg_counts[s], segment length) rows; arrival order is buffer position
        order.  A late record's ``row`` is its position in the buffer."""
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self.handle.push_device_segments(seg_counts, keys, timestamps, [values], key_hashes)

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """A packed padded exchange receive buffer (KeyByExchange.exchange_packed_async): rows of
        (key, ts, value) words."""
        self.handle.push_device_packed_segments(seg_counts, rows, row_words)

    def process_watermark_device(self, wm_tensor):
        """process_watermark with the watermark in device memory (the exchange's device valve): the
        handle takes max(its watermark, wm_tensor[0]) with no host wait; collecting the rows waits."""
        self.handle.advance_device(wm_tensor)
        return self._fired()

    def _key_objects(self, ids):
        return self._keys.objects(ids) if self.key_type == "STRING" else ids

    def process_watermark(self, watermark):
        """The sessions the watermark fires, sorted by (timestamp, key, window_start)."""
        self.handle.advance(watermark)
        return self._fired()

    def _fired(self):
        r = self.handle.results(reset=True)
        ts = r["window_end"] - 1
        order = np.lexsort((r["window_start"], r["key"], ts))
        return {"key": self._key_objects(r["key"][order]), "value": r["values"][0][order], "timestamp": ts[order],
                "window_start": r["window_start"][order], "window_end": r["window_end"][order]}

    def late_records(self):
        """The late side output since the last call (late_side_output): key, ts, value, push_seq, row."""
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
