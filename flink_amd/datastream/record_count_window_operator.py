"""GPU-backed drop-in for KeyedStream.countWindow programs that emit whole records.

countWindow(size[, slide]) with sum / min / max on a field of a record with more fields than (key,
field), and with minBy / maxBy: the operators of count_window_operator.py, whose outputs are

sum / min / max(field)     SumAggregator / ComparableAggregator (byAggregate = false): a copy of value1
                           -- the window's OLDEST element -- with the aggregated field set
minBy / maxBy(field, first) ComparableAggregator (byAggregate = true): the element with the extremal
                           field itself; ties go to the earliest element, or to the latest with
                           first = False

The device keeps, next to each count slice's aggregate, the arrival ordinal of one element (the
slice's first, or its extremal one) and tells this shim which elements to keep
(fw_first_element_events); every result row names the record it is built from by its ordinal.

Per batch the shim reads the results, applies the retains (copying records out of the batch), resolves
the result ordinals from the retained set or from the batch, applies the releases and drops the batch:
one host wait per process_batch.  Output records are appended to what collect() returns, in the
reference's emission order, with timestamp Long.MAX_VALUE.

Behind the N > 1 keyBy exchange (``record_types=[...]``, RecordCountExchangeStep) the record travels as
the packed row itself -- F fixed-width fields, LONG / INT / DOUBLE, one 8-byte word each -- and the batch
is the exchange's receive buffer on the device.  The shim never copies that buffer: the device gathers
the fields of the rows the retains and the results name (fw_count_record_rows), and the drain above runs
on those words, decoded to tuples by field type.
"""
import json
import math
import struct

import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from .count_window_operator import _KEY, _TYPE, LONG_MAX, StringKeyTable, _shape
from .window_operator import _dec_field, _enc_field

_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "minBy": abi.AGG_MINBY, "maxBy": abi.AGG_MAXBY}
_BY = ("minBy", "maxBy")


def is_gpu_eligible(assigner, trigger, aggregation, *, evictor=None, field=None, conf=None):
    """WindowOperatorBuilder's seam for record-shaped count windows: the two shapes countWindow
    builds, with sum / min / max / minBy / maxBy on a LONG / INT / DOUBLE field of the record.
    ``aggregation`` is (fn, field type) or, for minBy / maxBy, (fn, field type, first)."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    shape, why = _shape(assigner, trigger, evictor)
    if shape is None:
        return False, why
    size, slide = shape
    if size < 1 or slide < 1:
        return False, "count window size and slide must be >= 1"
    if len(aggregation) < 2 or aggregation[0] not in _AGG:
        return False, "not sum / min / max / minBy / maxBy (a count has no record-shaped form)"
    if aggregation[1] not in _TYPE:
        return False, f"field type {aggregation[1]} is not LONG / INT / DOUBLE"
    if len(aggregation) > 3 or (len(aggregation) == 3 and (aggregation[0] not in _BY or not isinstance(aggregation[2], bool))):
        return False, "only minBy / maxBy take a tie rule (field, first)"
    if not isinstance(field, int) or isinstance(field, bool) or field < 0:
        return False, "a record-shaped operator needs the aggregated field's index (field=...)"
    if size // math.gcd(size, slide) > abi.FW_COUNT_MAX_SLICES:
        return False, f"size / gcd(size, slide) exceeds {abi.FW_COUNT_MAX_SLICES} count slices"
    return True, ""


def record_to_words(rec, record_types):
    """a record's fields as the int64 words of a packed row: an INT sign-extended, a DOUBLE its bits"""
    return [struct.unpack("<q", struct.pack("<d", x))[0] if t == "DOUBLE" else int(x) for x, t in zip(rec, record_types)]


def words_to_records(words, record_types):
    """rows of F int64 words ([n, F]) as tuples: an INT narrowed to 32 bits, a DOUBLE by its bits"""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, len(record_types))
    cols = []
    for f, t in enumerate(record_types):
        c = np.ascontiguousarray(words[:, f])
        cols.append((c.view(np.float64) if t == "DOUBLE" else c.astype(np.int32) if t == "INT" else c).tolist())
    return list(zip(*cols)) if len(words) else []


def _check_record_types(record_types, field, ftype):
    if not isinstance(record_types, (list, tuple)) or not 1 <= len(record_types) <= abi.FW_MAX_COLS:
        raise ValueError(f"record_types: a record behind the exchange has 1 .. {abi.FW_MAX_COLS} fields")
    for t in record_types:
        if t not in _TYPE:
            raise ValueError(f"record_types: field type {t} is not LONG / INT / DOUBLE (fixed-width fields only)")
    if field >= len(record_types):
        raise ValueError(f"field {field} is outside the record's {len(record_types)} fields")
    if record_types[field] != ftype:
        raise ValueError(f"record_types[{field}] is {record_types[field]}, the aggregated field is {ftype}")


class RecordCountWindowOperator:
    def __init__(self, size, slide=None, aggregation=("sum", "LONG"), field=1, key_type="LONG", max_parallelism=128,
                 parallelism=1, subtask_index=0, device=0, state_capacity=1 << 16, max_batch_rows=1 << 20,
                 output_capacity=1 << 20, record_types=None):
        """countWindow(size) when ``slide`` is None, else countWindow(size, slide); ``field`` is the
        index of the aggregated field in a record.  ``record_types``: the types of the record's F
        fields (``field`` indexes into them) -- the form that runs behind the keyBy exchange, where
        the record is the packed row; None: records are any tuples and stay on the host."""
        from .windowing import CountEvictor, CountTrigger, GlobalWindows, PurgingTrigger
        trig = CountTrigger.of(size if slide is None else slide)
        ok, why = is_gpu_eligible(GlobalWindows.create(), PurgingTrigger.of(trig) if slide is None else trig, aggregation,
                                  evictor=None if slide is None else CountEvictor.of(size), field=field)
        if not ok:
            raise ValueError(f"not eligible for the GPU record count-window operator: {why}")
        fn, ftype = aggregation[:2]
        t = _TYPE[ftype]
        flags = abi.AGGF_LAST if fn in _BY and len(aggregation) > 2 and not aggregation[2] else 0
        self.size, self.slide = size, size if slide is None else slide
        self.aggregation = aggregation
        self.field = field
        self.key_type = key_type
        if record_types is not None:
            _check_record_types(record_types, field, ftype)
        self.record_types = None if record_types is None else list(record_types)
        cols = [t] if record_types is None else [_TYPE[x] for x in record_types]
        self.cfg = abi.make_config(
            api=abi.API_DATASTREAM, window_kind=abi.WIN_COUNT_RECORD, size_ms=size, slide_ms=0 if slide is None else slide,
            aggs=[(_AGG[fn], 0 if record_types is None else field, t, flags)], count_star_index=-1, value_col_types=cols,
            key_hash=_KEY[key_type],
            max_parallelism=max_parallelism, parallelism=parallelism, subtask_index=subtask_index, device=device,
            state_capacity=state_capacity, max_batch_rows=max_batch_rows, output_capacity=output_capacity,
            ds_first_ordinals=True)
        self.handle = None
        self._keys = StringKeyTable()
        self._retained = {}   # arrival ordinal -> record
        self._out = []        # (key, record, trigger ordinal, record ordinal) not yet collected

    def open(self):
        self.handle = WindowAggHandle(self.cfg)
        return self

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None

    def process_batch(self, keys, values, records, key_hashes=None):
        """processElement for a batch of elements in arrival order: ``values`` is the aggregated
        field's column, ``records`` the elements themselves (tuples).  A STRING-keyed operator takes
        its keys as Python strings.  Waits for the device once (the results and events are read)."""
        n = len(records)
        if len(keys) != n or len(values) != n:
            raise ValueError("keys, values and records must have one entry per element")
        if self.key_type == "STRING":
            keys, key_hashes = self._keys.intern_batch(keys)
        keys = np.asarray(keys, dtype=np.int64)
        seq0 = self.handle.push_seq
        self.handle.push_host(keys, np.zeros(n, np.int64), self._columns(values, records), key_hashes)
        cap = self.cfg.max_batch_rows   # push_host makes one push per max_batch_rows rows
        batch = {seq: records[i * cap:(i + 1) * cap] for i, seq in enumerate(range(seq0, self.handle.push_seq))}
        self._drain(batch)

    def _columns(self, values, records):
        """the value columns of a host batch: the aggregated field's, or -- with record_types -- the record's F fields"""
        if self.record_types is None:
            return [np.asarray(values)]
        cols = [np.array([r[f] for r in records], np.float64 if t == "DOUBLE" else np.int64) for f, t in enumerate(self.record_types)]
        cols[self.field] = np.asarray(values)
        return cols

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """Behind the N > 1 keyBy exchange: the packed padded receive buffer (a device tensor),
        len(seg_counts) segments, rows of (key, unread word, the record's F fields); the elements arrive
        in buffer position order.  One launch and one drain per call: waits for the device once, and
        ``rows`` may be reused when it returns."""
        if self.record_types is None:
            raise ValueError("the exchange form needs the record's field types (record_types=[...])")
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")
        if seg_counts.numel() == 0 or rows.numel() == 0:
            return
        self.handle.push_device_count_record_packed_segments(seg_counts, rows, row_words)
        self._drain_device(rows, row_words)

    def _drain_device(self, rows, row_words):
        """_drain's order on the gathered words: the gather goes first (it reads the unread result rows),
        then results, retains, result ordinals, releases"""
        g = self.handle.count_record_rows(rows, row_words)
        r = self.handle.results(reset=True)
        types = self.record_types
        keep = g["ev_is_retain"]
        self._retained.update(zip(g["ev_ord"][keep].tolist(), words_to_records(g["ev_words"][keep], types)))
        order = np.argsort(r["first_ord"], kind="stable")
        rords = r["values"][1][order].tolist()
        here = g["res_from_push"][order]
        fresh = iter(words_to_records(g["res_words"][order][here], types))
        firsts = [next(fresh) if h else self._retained[o] for h, o in zip(here.tolist(), rords)]
        self._emit(r, order, rords, firsts)
        for o in g["ev_ord"][~keep].tolist():
            del self._retained[o]

    def _drain(self, batch):
        """results, retains, result ordinals, releases -- in this order -- then the batch is dropped"""
        def element(o):
            rec = self._retained.get(o)
            return rec if rec is not None else batch[o >> 32][o & 0xFFFFFFFF]
        r = self.handle.results(reset=True)
        retain, release = self.handle.first_element_events()
        for o in retain.tolist():
            self._retained[o] = batch[o >> 32][o & 0xFFFFFFFF]   # a retain names a row of this batch
        order = np.argsort(r["first_ord"], kind="stable")
        rords = r["values"][1][order].tolist()
        self._emit(r, order, rords, [element(o) for o in rords])
        for o in release.tolist():
            del self._retained[o]

    def _emit(self, r, order, rords, firsts):
        """appends the result rows ``order`` of r, built from the records ``firsts``, to the output"""
        ids = r["key"][order]
        keys = self._keys.objects(ids).tolist() if self.key_type == "STRING" else ids.tolist()
        if self.aggregation[0] in _BY:   # the extremal element itself
            recs = firsts
        else:
            vals = self._field_values(r["values"][0][order])
            f = self.field
            recs = [tuple(x[:f]) + (v,) + tuple(x[f + 1:]) for x, v in zip(firsts, vals)]
        self._out += list(zip(keys, recs, r["first_ord"][order].tolist(), rords))

    def _field_values(self, words):
        ftype = self.aggregation[1]
        if ftype == "DOUBLE":
            return [struct.unpack("<d", struct.pack("<q", int(w)))[0] for w in words]
        if ftype == "INT":
            return [int(np.int32(np.int64(w))) for w in words]
        return [int(w) for w in words]

    def collect(self):
        """The records fired since the last call, in the reference's emission order."""
        out, self._out = self._out, []
        return {"key": [o[0] for o in out], "records": [o[1] for o in out],
                "timestamp": np.full(len(out), LONG_MAX, np.int64),
                "trigger_ord": np.array([o[2] for o in out], np.int64),
                "record_ord": np.array([o[3] for o in out], np.int64)}

    def retained_ordinals(self):
        """The arrival ordinals of the records the operator holds (tests compare them with the reference's)."""
        return set(self._retained)

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
        return {"key": [], "records": [], "timestamp": np.empty(0, np.int64), "trigger_ord": np.empty(0, np.int64),
                "record_ord": np.empty(0, np.int64)}

    def snapshot_state(self) -> bytes:
        """The device blob, then the retained records (floats by their bits) and, for STRING keys, the
        Strings behind the device key ids."""
        blob = self.handle.snapshot()
        side = {"retained": [[o, [_enc_field(x) for x in rec]] for o, rec in sorted(self._retained.items())]}
        if self.key_type == "STRING":
            side["strings"] = self._keys.strings
        return struct.pack("<q", len(blob)) + blob + json.dumps(side).encode()

    def initialize_state(self, blob: bytes):
        n = struct.unpack_from("<q", blob, 0)[0]
        self.handle.restore(blob[8:8 + n])
        side = json.loads(blob[8 + n:].decode())
        self._retained = {int(o): tuple(_dec_field(x) for x in rec) for o, rec in side["retained"]}
        if self.key_type == "STRING":
            self._keys = StringKeyTable(side["strings"])
        self._out = []
