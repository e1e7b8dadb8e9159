"""What the four GPU session-window operators share: the aggregation, key and field-type tables, the
common eligibility checks of their WindowOperatorBuilder seams, and a base class with everything that
does not depend on the kind -- the handle's life cycle, the push plumbing, watermarks, fired rows, the
late side output, snapshots and output records.

The kinds are two flags.  A dynamic kind (dynamic_session_window_operator, and with a lateness
late_dynamic_session_window_operator) passes a gap column beside the field and checks its gaps; a
lateness kind (late_session_window_operator and late_dynamic_session_window_operator) adds
``collect()``.  Each module keeps its own seam, refusal texts and make_config call.
"""
import json
import struct

import numpy as np

from .. import abi
from ..runtime.handle import WindowAggHandle
from ..runtime.options import gpu_enabled
from .count_window_operator import StringKeyTable
from .windowing import EventTimeTrigger

MAX_GAP = 1 << 40
_AGG = {"sum": abi.AGG_SUM, "min": abi.AGG_MIN, "max": abi.AGG_MAX, "count": abi.AGG_COUNT_STAR}
_KEY = {"LONG": abi.KEYHASH_LONG, "INT": abi.KEYHASH_INT, "HOST_HASHED": abi.KEYHASH_PRECOMPUTED,
        "STRING": abi.KEYHASH_PRECOMPUTED}
_TYPE = {"LONG": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def _common_eligibility(assigner, assigner_type, assigner_refusal, trigger, aggregation, *, evictor, conf, lateness_refusal,
                        gap, gap_refusal):
    """The checks of a session seam in their one order: configuration, assigner, trigger, evictor,
    lateness, gap, aggregation, field type.  The kind supplies the assigner it takes, its verdict on
    the lateness (``lateness_refusal``: a text or None) and the gap it bounds by MAX_GAP."""
    if conf is not None and not gpu_enabled(conf):
        return False, "gpu.window-agg.enabled is false"
    if not isinstance(assigner, assigner_type):
        return False, assigner_refusal
    if not isinstance(trigger, EventTimeTrigger):
        return False, "trigger is not EventTimeTrigger"
    if evictor is not None:
        return False, "session windows with an evictor stay on the reference operator"
    if lateness_refusal is not None:
        return False, lateness_refusal
    if gap <= 0 or gap > MAX_GAP:
        return False, gap_refusal
    if len(aggregation) != 2 or aggregation[0] not in _AGG:
        return False, "not sum / min / max / count (minBy / maxBy stay on the reference operator)"
    if aggregation[1] not in _TYPE:
        return False, f"field type {aggregation[1]} is not LONG / INT / DOUBLE"
    return True, ""


class SessionOperatorBase:
    """A subclass's constructor sets ``cfg`` (its make_config call) and calls ``_init_common``; its
    process_batch / process_batch_device / process_segments_device name the columns it takes and go
    through ``_push_host`` / ``_push_device`` / ``_push_segments``."""

    def _init_common(self, aggregation, key_type):
        self.aggregation = aggregation
        self.key_type = key_type
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

    def _push_host(self, keys, timestamps, columns, key_hashes):
        if self.key_type == "STRING":
            keys, key_hashes = self._keys.intern_batch(keys)
        keys = np.asarray(keys, dtype=np.int64)
        self.handle.push_host(keys, np.asarray(timestamps, dtype=np.int64), columns, key_hashes)

    def _refuse_string_keys(self):
        if self.key_type == "STRING":
            raise ValueError("a STRING-keyed operator interns its keys on the host (process_batch)")

    def _push_device(self, keys, timestamps, columns, key_hashes):
        self._refuse_string_keys()
        self._device_pushed = True
        self.handle.push_device(keys, timestamps, columns, key_hashes)

    # ---- behind the N > 1 keyBy exchange (parallelism > 1; a subtask of parallelism 1 has no exchange
    # in front of it and its handle refuses these)
    def _push_segments(self, seg_counts, keys, timestamps, columns, key_hashes):
        self._refuse_string_keys()
        self._device_pushed = True
        self.handle.push_device_segments(seg_counts, keys, timestamps, columns, key_hashes)

    def process_packed_segments_device(self, seg_counts, rows, row_words):
        """A packed padded exchange receive buffer (KeyByExchange.exchange_packed_async): rows of
        (key, ts, value) words, with a dynamic gap (key, ts, value, gap)."""
        self._device_pushed = True
        self.handle.push_device_packed_segments(seg_counts, rows, row_words)

    def _check_gaps(self):
        """in front of every watermark: the dynamic kinds raise for a device batch's bad gap"""

    def process_watermark(self, watermark):
        """The sessions the watermark fires, sorted by (timestamp, key, window_start)."""
        self._check_gaps()
        self.handle.advance(watermark)
        return self._fired()

    def process_watermark_device(self, wm_tensor):
        """process_watermark with the watermark in device memory (the exchange's device valve): the
        handle takes max(its watermark, wm_tensor[0]) with no host wait; a dynamic kind's gap check
        and collecting the rows wait."""
        self._check_gaps()
        self.handle.advance_device(wm_tensor)
        return self._fired()

    def _key_objects(self, ids):
        return self._keys.objects(ids) if self.key_type == "STRING" else ids

    def _fired(self):
        r = self.handle.results(reset=True)
        ts = r["window_end"] - 1
        order = np.lexsort((r["window_start"], r["key"], ts))
        return {"key": self._key_objects(r["key"][order]), "value": r["values"][0][order], "timestamp": ts[order],
                "window_start": r["window_start"][order], "window_end": r["window_end"][order]}

    def late_records(self):
        """The late side output since the last call (late_side_output): key, ts, value, push_seq, row
        (with dynamic gaps the element's gap is the one the caller passed at that push_seq, row)."""
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
