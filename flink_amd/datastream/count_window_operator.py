"""GPU-backed drop-in for the operators KeyedStream.countWindow builds, on their eligible subset.

countWindow(size)        GlobalWindows + PurgingTrigger.of(CountTrigger.of(size)), no evictor
                         (WindowOperator with reducing state)
countWindow(size, slide) GlobalWindows + CountTrigger.of(slide) + CountEvictor.of(size)
                         (EvictingWindowOperator)

WindowOperatorBuilder would return this operator iff the window is one of those two shapes and the
function is a built-in field aggregation sum / min / max (SumAggregator / ComparableAggregator) or a
count, on a LONG / INT / DOUBLE field of (key, field) tuples.  Anything else -- other evictors,
other triggers, minBy / maxBy, record-shaped outputs -- stays on the reference operator.

Semantics: a key fires at every slide-th of its elements with the aggregate of its last
min(count, size) elements; nothing fires on a watermark, so a last partial window is never emitted,
and no element is late.  Output records are (key, aggregate) with timestamp
GlobalWindow.maxTimestamp() = Long.MAX_VALUE.  The reference emits a result at the element that
triggers it; every device row carries that element's arrival ordinal and collect() returns the rows
sorted by it.
"""
import json
import math
import struct

import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from . import heap_state
from .windowing import CountEvictor, CountTrigger, GlobalWindows, PurgingTrigger

LONG_MAX = (1 << 63) - 1
_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_KEY = {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT, "HOST_HASHED": abi.KEYHASH_PRECOMPUTED,
        "STRING": abi.KEYHASH_PRECOMPUTED}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


class StringKeyTable:
    """STRING keys (keyBy a String field): each String is interned to a dense int64 id -- the device
    key -- and the device gets its String.hashCode, which routes it as
    KeyGroupRangeAssignment.assignToKeyGroup(key) does (FW_KEYHASH_PRECOMPUTED).  Ids are never reused."""

    def __init__(self, strings=()):
        self.strings = list(strings)
        self.ids = {k: i for i, k in enumerate(self.strings)}
        self.hashes = [heap_state.java_string_hash(k) for k in self.strings]

    def intern(self, key):
        i = self.ids.get(key)
        if i is None:
            i = self.ids[key] = len(self.strings)
            self.strings.append(key)
            self.hashes.append(heap_state.java_string_hash(key))
        return i, self.hashes[i]

    def intern_batch(self, keys):
        if not len(keys):
            return np.empty(0, np.int64), np.empty(0, np.int32)
        uniq, inv = np.unique(np.asarray([str(k) for k in keys], dtype=object), return_inverse=True)
        ids = np.empty(len(uniq), np.int64)
        hashes = np.empty(len(uniq), np.int32)
        for i, k in enumerate(uniq.tolist()):
            ids[i], hashes[i] = self.intern(k)
        return ids[inv], hashes[inv]

    def objects(self, ids):
        return np.array([self.strings[int(i)] for i in ids], dtype=object)


def _shape(assigner, trigger, evictor):
    """(size, slide) of the two shapes countWindow builds, or a reason"""
    if not isinstance(assigner, GlobalWindows):
        return None, "assigner is not GlobalWindows"
    if evictor is None:
        if isinstance(trigger, PurgingTrigger) and isinstance(trigger.nested, CountTrigger):
            return (trigger.nested.max_count, trigger.nested.max_count), ""
        if isinstance(trigger, CountTrigger):
            return None, "a CountTrigger without CountEvictor never drops elements (not countWindow(size, slide))"
        return None, "trigger is not PurgingTrigger(CountTrigger)"
    if not isinstance(evictor, CountEvictor):
        return None, "evictor is not CountEvictor"
    if evictor.do_evict_after:
        return None, "CountEvictor with doEvictAfter"
    if not isinstance(trigger, CountTrigger):
        return None, "CountEvictor with a trigger other than CountTrigger"
    return (evictor.max_count, trigger.max_count), ""


def is_gpu_eligible(assigner, trigger, aggregation, *, evictor=None, conf=None):
    """WindowOperatorBuilder's seam for count windows: exactly the two shapes countWindow builds, with
    sum / min / max / count on LONG / INT / DOUBLE.  ``conf``: the job configuration
    (``gpu.window-agg.enabled``); None = the GPU operator was chosen."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    shape, why = _shape(assigner, trigger, evictor)
    if shape is None:
        return False, why
    size, slide = shape
    if size < 1 or slide < 1:
        return False, "count window size and slide must be >= 1"
    if len(aggregation) != 2 or aggregation[0] not in _AGG:
        return False, "not sum / min / max / count (minBy / maxBy stay on the reference operator)"
    if aggregation[1] not in _TYPE:
        return False, f"field type {aggregation[1]} is not LONG / INT / DOUBLE"
    if size // math.gcd(size, slide) > abi.FW_COUNT_MAX_SLICES:
        return False, f"size / gcd(size, slide) exceeds {abi.FW_COUNT_MAX_SLICES} count slices"
    return True, ""


class CountWindowOperator:
    def __init__(self, size, slide=None, aggregation=("sum", "LONG"), key_type="LONG", max_parallelism=128,
                 parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16, max_batch_rows=1 << 20,
                 output_capacity=1 << 20):
        """countWindow(size) when ``slide`` is None, else countWindow(size, slide)."""
        trig = CountTrigger.of(size if slide is None else slide)
        ok, why = is_gpu_eligible(GlobalWindows.create(), PurgingTrigger.of(trig) if slide is None else trig, aggregation,
                                  evictor=None if slide is None else CountEvictor.of(size))
        if not ok:
            raise ValueError(f"not eligible for the GPU count-window operator: {why}")
        fn, ftype = aggregation
        t = _TYPE[ftype]
        self.size, self.slide = size, size if slide is None else slide
        self.aggregation = aggregation
        self.key_type = key_type
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT, size_ms=size, slide_ms=0 if slide is None else slide,
            aggs=[(_AGG[fn], 0, t)], count_star_index=-1, value_col_types=[t], key_hash=_KEY[key_type],
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity)
        self.handle = None
        self._keys = StringKeyTable()

    def open(self):
        self.handle = WindowAggHandle(self.cfg)
        return self

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

    def process_batch(self, keys, values, key_hashes=None):
        """processElement for a batch of (key, field) elements, in arrival order.  A STRING-keyed
        operator takes its keys as Python strings."""
        if self.key_type == "STRING":
            keys, key_hashes = self._keys.intern_batch(keys)
        keys = np.asarray(keys, dtype=np.int64)
        self.handle.push_host(keys, np.zeros(len(keys), np.int64), [np.asarray(values)], key_hashes)

    def process_batch_device(self, keys, values, key_hashes=None):
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self.handle.push_device(keys, None, [values], key_hashes)

    def process_segments_device(self, seg_counts, keys, values, key_hashes=None):
        """Behind the N > 1 keyBy exchange: a padded receive buffer as columns, len(seg_counts)
        segments, segment s holding seg_counts[s] live rows in front of its padding.  The elements
        arrive in buffer position order; ``values`` may be None for a count."""
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self.handle.push_device_count_segments(seg_counts, keys, values, key_hashes)

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """The same over the exchange's packed rows (key, ts, value); the ts word is not read."""
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        self.handle.push_device_count_packed_segments(seg_counts, rows, row_words)

    def collect(self):
        """The rows fired since the last call, in the reference's emission order."""
        r = self.handle.results(reset=True)
        order = np.argsort(r["first_ord"], kind="stable")
        ids = r["key"][order]
        n = len(order)
        return {"key": self._keys.objects(ids) if self.key_type == "STRING" else ids, "value": r["values"][0][order],
                "timestamp": np.full(n, LONG_MAX, np.int64), "window_start": r["window_start"][order],
                "window_end": r["window_end"][order], "trigger_ord": r["first_ord"][order]}

    def process_watermark(self, watermark):
        """CountTrigger.onEventTime returns CONTINUE: the watermark is recorded and nothing fires."""
        self.handle.advance(watermark)
        return self._no_rows()

    def process_watermark_device(self, wm_tensor):
        """The watermark in device memory (the exchange's device valve): recorded on the device,
        nothing fires, no host wait."""
        self.handle.advance_device(wm_tensor)
        return self._no_rows()

    def _no_rows(self):
        e = np.empty(0, np.int64)
        return {"key": np.empty(0, object) if self.key_type == "STRING" else e, "value": e, "timestamp": e,
                "window_start": e, "window_end": e, "trigger_ord": e}

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
