"""Every refusal of the push, advance and result entry points that an argument or a call order can
trigger, through the C entry points themselves (the Python wrappers check things of their own and would
hide null pointers): the exact return code and the exact fw_last_error() text, per kind of handle.  The
cases that break two rules at once pin which check wins.  After a handle's cases one good push is made
and read: rows, live entries, late drops, fired windows and error flags equal those of a twin handle
that made only the accepted calls of the list.

The expected literals were written down from the library as it stood before the entry points' checks
were shared, not from the code under test.  Outside the table: texts that carry a device failure, the
two result-overflow refusals (FW_E_CAPACITY) and fw_count_record_rows' refusals of what the device
wrote (a retain event or a result naming a row outside the push)."""
import ctypes as C

import numpy as np
import pytest

from flink_amd import _native, abi

pytestmark = pytest.mark.gpu

CAP = 1 << 10
T0 = 1_600_000_000_000
INV, STATE = abi.FW_E_INVALID, abi.FW_E_STATE
SMALL = dict(state_capacity=CAP, max_batch_rows=CAP, output_capacity=CAP)
I64 = abi.T_I64
SUM0 = [(abi.AGG_SUM, 0, I64)]


def _tumble(**kw):
    kw = {**dict(api=abi.API_SQL, window_kind=abi.WIN_TUMBLE, size_ms=1000, aggs=SUM0, value_col_types=[I64],
                 key_hash=abi.KEYHASH_BINROW_BIGINT), **SMALL, **kw}
    return abi.make_config(**kw)


def _ds(window_kind, size, **kw):
    kw = {**dict(api=abi.API_DATASTREAM, window_kind=window_kind, size_ms=size, aggs=SUM0, value_col_types=[I64],
                 key_hash=abi.KEYHASH_LONG), **SMALL, **kw}
    return abi.make_config(**kw)


PRE = abi.KEYHASH_PRECOMPUTED
CONFIGS = {
    "T": lambda: _tumble(nullable_cols=(0,)),
    "TP": lambda: _tumble(nullable_cols=(0,), key_hash=PRE),
    "D": lambda: _ds(abi.WIN_TUMBLE, 1000, ds_first_ordinals=True, late_side_output=True),
    "K": lambda: _tumble(nullable_cols=(0,), key_hash=abi.KEYHASH_KEYROW),
    "C1": lambda: _ds(abi.WIN_COUNT, 2),
    "C2": lambda: _ds(abi.WIN_COUNT, 2, parallelism=2),
    "CP2": lambda: _ds(abi.WIN_COUNT, 2, parallelism=2, key_hash=PRE),
    "R1": lambda: _ds(abi.WIN_COUNT_RECORD, 2, ds_first_ordinals=True),
    "R2": lambda: _ds(abi.WIN_COUNT_RECORD, 2, ds_first_ordinals=True, parallelism=2),
    "RP2": lambda: _ds(abi.WIN_COUNT_RECORD, 2, ds_first_ordinals=True, parallelism=2, key_hash=PRE),
    "S1": lambda: _ds(abi.WIN_SESSION, 100),
    "S2": lambda: _ds(abi.WIN_SESSION, 100, parallelism=2),
    "SQ": lambda: abi.make_config(api=abi.API_SQL, window_kind=abi.WIN_SESSION, size_ms=100, aggs=SUM0, value_col_types=[I64],
                                  nullable_cols=(0,), key_hash=PRE, **SMALL),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def VA(*ptrs):
    return (C.c_void_p * abi.FW_MAX_COLS)(*ptrs)


class Ctx:
    """one handle and the device columns of its good push; ``z`` is 8192 zero words, a valid column for any call
    the library accepts (zero segment counts, or rows of key 0)"""

    def __init__(self, kind, data):
        self.kind, self.L = kind, _native.lib()
        self.cfg = CONFIGS[kind]()
        self.h = C.c_void_p()
        _native.check(self.L.fw_create(C.byref(self.cfg), C.byref(self.h)))
        self.cols = abi.fw_host_cols()
        self.res, self.segs, self.dn = abi.fw_result(), abi.fw_result_segments(), C.c_void_p()
        self.ev, self.late, self.rr = abi.fw_ordinal_events(), abi.fw_late_rows(), abi.fw_record_rows()
        self.t = data   # torch tensors, kept alive
        for name, tensor in data.items():
            setattr(self, name, tensor.data_ptr())

    def close(self):
        if self.h:
            self.L.fw_destroy(self.h)
            self.h = C.c_void_p()


def _data(cfg):
    """the good push: 4 keys of this subtask twice, as columns, as two segments of 4 rows and as packed rows"""
    import torch
    from flink_amd.table.key_rows import KeyRowColumns
    L = _native.lib()
    cand = np.arange(1, 401, dtype=np.int64)
    kh = cand.astype(np.int32)
    dest = np.empty(len(cand), np.int32)
    kind = abi.KEYHASH_LONG if cfg.key_hash == abi.KEYHASH_KEYROW else cfg.key_hash
    _native.check(L.fw_host_assign_key_groups(cand.ctypes.data, kh.ctypes.data, len(cand), kind, cfg.max_parallelism, cfg.parallelism,
                                              None, dest.ctypes.data))
    own = cand[dest == cfg.subtask_index][:4]
    key = np.concatenate([own, own])
    ts = T0 + 10 * np.arange(8, dtype=np.int64)
    val = np.arange(1, 9, dtype=np.int64)
    rows = np.stack([key, ts, val], axis=1).reshape(-1)
    off, img = KeyRowColumns.from_rows([(int(k),) for k in key], ("BIGINT",)).images_host()
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    out = {"z": torch.zeros(8192, dtype=torch.int64, device="cuda"), "key": dev(key), "ts": dev(ts), "kh": dev(key.astype(np.int32)),
           "val": dev(val), "nul": dev(np.zeros(8, np.uint8)), "counts": dev(np.array([4, 4], np.int64)), "rows": dev(rows),
           "kro": dev(off), "krb": dev(np.concatenate([img, np.zeros(8, np.uint8)]))}
    torch.cuda.synchronize()
    return out


def _last_error():
    msg = _native.lib().fw_last_error()
    return msg.decode() if msg else ""


# ---- the cases: (kinds, id, call, return code, message).  A call takes the handle's Ctx; kinds is a
# space-separated list, the case runs on each.
def kind_texts(entry, texts):
    """one case per kind of handle the entry refuses by its kind: texts = {kind: message after 'name: '}"""
    return [(k, f"{entry.__name__}/kind", entry, INV, f"{entry.__name__}: {t}") for k, t in texts.items()]


COUNT, SESSION = "not for count windows", "not for session windows"
ONLY_COUNT = {"S2": "not for session windows (count windows only)",
              "R2": "not for record count windows (FW_WIN_COUNT_RECORD: retained records are not re-numbered)",
              "T": "not for time windows (count windows only)",
              "C1": "a count handle of parallelism 1 has no keyBy exchange in front of it"}
ONLY_RECORD = {"S2": "not for session windows (record count windows only)",
               "T": "not for time windows (record count windows only)",
               "C2": "not for count windows (FW_WIN_COUNT: fw_push_device_count_packed_segments)",
               "R1": "a record count handle of parallelism 1 has no keyBy exchange in front of it"}
KEYROW_PUSH = "a FW_KEYHASH_KEYROW operator takes key rows (fw_push_device_key_rows)"
KEYROW_RESULTS = "key-row operators return their rows through fw_results"
NO_SIDE = "the operator has no late side output (late_side_output = 0)"
ORDINALS = "arrival ordinals need n_segs * seg_len < 2^32 rows per call"
VAL_NULL, NEEDS_FLAGS = "value column 0 is NULL", "nullable value column 0 needs its null-flag column"


def fw_push_device_key_rows(x):
    return x.L.fw_push_device_key_rows(x.h, 8, x.z, x.z, x.z, VA(x.z), VA(x.z))


def fw_push_device_segments(x):
    return x.L.fw_push_device_segments(x.h, 2, 4, x.z, x.z, x.z, x.z, VA(x.z), VA(x.z))


def fw_push_device_packed_segments(x):
    return x.L.fw_push_device_packed_segments(x.h, 2, 4, x.z, x.z, 3)


def fw_push_device_count_segments(x):
    return x.L.fw_push_device_count_segments(x.h, 2, 4, x.z, x.z, x.z, x.z)


def fw_push_device_count_packed_segments(x):
    return x.L.fw_push_device_count_packed_segments(x.h, 2, 4, x.z, x.z, 3)


def fw_push_device_count_record_packed_segments(x):
    return x.L.fw_push_device_count_record_packed_segments(x.h, 2, 4, x.z, x.z, 3)


def fw_count_record_rows(x):
    return x.L.fw_count_record_rows(x.h, x.z, 3, 8, C.byref(x.rr))


def fw_results_async(x):
    return x.L.fw_results_async(x.h)


def fw_results_ready(x):
    return x.L.fw_results_ready(x.h, C.byref(x.res))


def fw_results_device(x):
    return x.L.fw_results_device(x.h, C.byref(x.res), C.byref(x.dn))


def fw_results_device_segments(x):
    return x.L.fw_results_device_segments(x.h, C.byref(x.segs))


def fw_first_element_events(x):
    return x.L.fw_first_element_events(x.h, C.byref(x.ev))


def fw_late_records(x):
    return x.L.fw_late_records(x.h, C.byref(x.late))


def _bad_key_row_offsets(x):
    x.cols.key_row_offsets[1] = -5
    return x.L.fw_commit(x.h, 1)


def _push(x, n=8, key="z", ts="z", kh="z", values="z", nulls="z", one_value="z", one_null="z"):
    """fw_push_device; an argument is the name of a column of the Ctx, or None for a null pointer"""
    p = lambda name: None if name is None else getattr(x, name)
    return x.L.fw_push_device(x.h, n, p(key), p(ts), p(kh), None if values is None else VA(p(one_value)),
                              None if nulls is None else VA(p(one_null)))


def _key_rows(x, n=8, off="z", img="z", ts="z", values="z", nulls="z", one_value="z", one_null="z"):
    p = lambda name: None if name is None else getattr(x, name)
    return x.L.fw_push_device_key_rows(x.h, n, p(off), p(img), p(ts), None if values is None else VA(p(one_value)),
                                       None if nulls is None else VA(p(one_null)))


def _segments(x, n_segs=2, seg_len=4, counts="z", key="z", ts="z", kh="z", values="z", nulls="z", one_value="z", one_null="z"):
    p = lambda name: None if name is None else getattr(x, name)
    return x.L.fw_push_device_segments(x.h, n_segs, seg_len, p(counts), p(key), p(ts), p(kh),
                                       None if values is None else VA(p(one_value)), None if nulls is None else VA(p(one_null)))


def _packed(entry):
    def call(x, n_segs=2, seg_len=4, counts="z", rows="z", row_words=3):
        p = lambda name: None if name is None else getattr(x, name)
        return getattr(x.L, entry)(x.h, n_segs, seg_len, p(counts), p(rows), row_words)
    return call


_tp, _cp, _rp = (_packed(e) for e in ("fw_push_device_packed_segments", "fw_push_device_count_packed_segments",
                                       "fw_push_device_count_record_packed_segments"))


def _count_segments(x, n_segs=2, seg_len=4, counts="z", key="z", kh="z", value="z"):
    p = lambda name: None if name is None else getattr(x, name)
    return x.L.fw_push_device_count_segments(x.h, n_segs, seg_len, p(counts), p(key), p(kh), p(value))


def _rec_rows(x, rows="z", row_words=3, n_rows=8, out=True):
    return x.L.fw_count_record_rows(x.h, None if rows is None else getattr(x, rows), row_words, n_rows, C.byref(x.rr) if out else None)


def case(kinds, name, call, rc, msg=""):
    return [(k, name, call, rc, msg) for k in kinds.split()]


REC = "fw_push_device_count_record_packed_segments"
CASES = sum([
    # ---- fw_reserve / fw_commit / fw_commit_delta32
    case("T", "reserve/null_out", lambda x: x.L.fw_reserve(x.h, 4, None), INV, "null argument"),
    case("T", "reserve/above_max_batch_rows", lambda x: x.L.fw_reserve(x.h, CAP + 1, C.byref(x.cols)), INV,
         "reserve 1025 rows > max_batch_rows 1024"),
    case("T", "reserve/negative", lambda x: x.L.fw_reserve(x.h, -1, C.byref(x.cols)), INV, "reserve -1 rows > max_batch_rows 1024"),
    case("T K C1 S1", "commit/without_reserve", lambda x: x.L.fw_commit(x.h, 1), STATE, "commit without matching reserve"),
    case("T", "commit_delta32/without_reserve", lambda x: x.L.fw_commit_delta32(x.h, 1, 0, None), STATE, "commit without matching reserve"),
    case("T K", "reserve/ok", lambda x: x.L.fw_reserve(x.h, 1, C.byref(x.cols)), 0),
    case("T", "commit/more_than_reserved", lambda x: x.L.fw_commit(x.h, 2), STATE, "commit without matching reserve"),
    case("T", "commit/negative", lambda x: x.L.fw_commit(x.h, -1), STATE, "commit without matching reserve"),
    case("T", "commit/zero_rows", lambda x: x.L.fw_commit(x.h, 0), 0),
    case("T", "commit/reserve_consumed", lambda x: x.L.fw_commit(x.h, 0), STATE, "commit without matching reserve"),
    case("K", "commit/bad_key_row_offsets", _bad_key_row_offsets, INV, "key row offsets must start at 0 and end within key_row_bytes_cap"),
    case("T", "commit_delta32/unknown_column", lambda x: x.L.fw_commit_delta32(x.h, 1, 8, None), INV,
         "delta_cols 0x8 names a column the operator does not have"),
    case("K", "commit_delta32/key_of_key_rows", lambda x: x.L.fw_commit_delta32(x.h, 1, 1, None), INV,
         "key-row operators have no key column to pack"),
    case("T", "commit_delta32/no_bases", lambda x: x.L.fw_commit_delta32(x.h, 1, 2, None), INV, "packed columns need their bases"),
    # ---- fw_push_device_key_rows
    kind_texts(fw_push_device_key_rows, {"C1": COUNT, "S1": SESSION}),
    case("T", "key_rows/not_a_key_row_operator", fw_push_device_key_rows, INV, "fw_push_device_key_rows needs a FW_KEYHASH_KEYROW operator"),
    case("K", "key_rows/negative_n", lambda x: _key_rows(x, n=-1), INV, "negative n"),
    case("K", "key_rows/zero_rows_null_columns", lambda x: _key_rows(x, 0, None, None, None, None, None), 0),
    case("K", "key_rows/null_offsets", lambda x: _key_rows(x, off=None), INV, "null key row / ts column"),
    case("K", "key_rows/null_bytes", lambda x: _key_rows(x, img=None), INV, "null key row / ts column"),
    case("K", "key_rows/null_ts", lambda x: _key_rows(x, ts=None), INV, "null key row / ts column"),
    case("K", "key_rows/null_values", lambda x: _key_rows(x, values=None), INV, "value columns required"),
    case("K", "key_rows/null_value_column", lambda x: _key_rows(x, one_value=None), INV, VAL_NULL),
    case("K", "key_rows/null_flags", lambda x: _key_rows(x, nulls=None), INV, NEEDS_FLAGS),
    case("K", "key_rows/null_flag_column", lambda x: _key_rows(x, one_null=None), INV, NEEDS_FLAGS),
    case("K", "key_rows/null_ts_and_values", lambda x: _key_rows(x, ts=None, values=None), INV, "null key row / ts column"),
    # ---- fw_push_device: the time-window branch, the session branch, the count branch
    case("T D K C1 S1", "push/negative_n", lambda x: _push(x, n=-1), INV, "negative n"),
    case("T D K C1 S1 SQ TP", "push/zero_rows_null_columns", lambda x: _push(x, 0, None, None, None, None, None), 0),
    case("T D S1 SQ", "push/null_key", lambda x: _push(x, key=None), INV, "null key/ts column"),
    case("T D S1 SQ K", "push/null_ts", lambda x: _push(x, ts=None), INV, "null key/ts column"),
    case("K", "push/key_row_operator", _push, INV, KEYROW_PUSH),
    case("TP SQ", "push/no_hashes", lambda x: _push(x, kh=None), INV, "key_hash column required"),
    case("TP SQ", "push/null_key_and_no_hashes", lambda x: _push(x, key=None, kh=None), INV, "null key/ts column"),
    case("TP SQ", "push/no_hashes_and_null_values", lambda x: _push(x, kh=None, values=None), INV, "key_hash column required"),
    case("T D S1 SQ", "push/null_values", lambda x: _push(x, values=None), INV, "value columns required"),
    case("T D S1 SQ", "push/null_value_column", lambda x: _push(x, one_value=None), INV, VAL_NULL),
    case("T TP SQ", "push/null_flags", lambda x: _push(x, nulls=None), INV, NEEDS_FLAGS),
    case("T TP SQ", "push/null_flag_column", lambda x: _push(x, one_null=None), INV, NEEDS_FLAGS),
    case("T SQ", "push/null_value_column_and_flags", lambda x: _push(x, one_value=None, nulls=None), INV, VAL_NULL),
    case("D S1", "push/not_nullable_null_flags", lambda x: _push(x, n=0, nulls=None), 0),
    case("C1 CP2", "push/count_null_key", lambda x: _push(x, key=None), INV, "null key column"),
    case("CP2", "push/count_no_hashes", lambda x: _push(x, kh=None), INV, "key_hash column required"),
    case("C1 CP2", "push/count_null_values", lambda x: _push(x, values=None), INV, VAL_NULL),
    case("C1", "push/count_null_value_column", lambda x: _push(x, one_value=None), INV, VAL_NULL),
    case("C1", "push/count_null_ts_accepted", lambda x: _push(x, 1, ts=None, kh=None, nulls=None), 0),
    # ---- fw_push_device_segments
    kind_texts(fw_push_device_segments, {"C2": COUNT, "C1": COUNT, "S1": SESSION}),
    case("T K S2", "segments/negative_n_segs", lambda x: _segments(x, n_segs=-1), INV, "bad segments"),
    case("T K S2", "segments/seg_len_0", lambda x: _segments(x, seg_len=0), INV, "bad segments"),
    case("T S2", "segments/null_counts", lambda x: _segments(x, counts=None), INV, "bad segments"),
    case("K", "segments/key_row_operator", _segments, INV, KEYROW_PUSH),
    case("T TP S2", "segments/no_segments_null_columns", lambda x: _segments(x, 0, 4, None, None, None, None, None, None), 0),
    case("T S2", "segments/null_key", lambda x: _segments(x, key=None), INV, "null key/ts column"),
    case("T S2", "segments/null_ts", lambda x: _segments(x, ts=None), INV, "null key/ts column"),
    case("TP", "segments/no_hashes", lambda x: _segments(x, kh=None), INV, "key_hash column required"),
    case("TP", "segments/null_ts_and_no_hashes", lambda x: _segments(x, ts=None, kh=None), INV, "null key/ts column"),
    case("T S2", "segments/null_values", lambda x: _segments(x, values=None), INV, "value columns required"),
    case("T S2", "segments/null_value_column", lambda x: _segments(x, one_value=None), INV, VAL_NULL),
    case("T TP", "segments/null_flags", lambda x: _segments(x, nulls=None), INV, NEEDS_FLAGS),
    case("T", "segments/null_flag_column", lambda x: _segments(x, one_null=None), INV, NEEDS_FLAGS),
    case("S2", "segments/session_accepted", lambda x: _segments(x, kh=None, nulls=None), 0),
    # ---- fw_push_device_packed_segments
    kind_texts(fw_push_device_packed_segments, {"C2": COUNT, "S1": SESSION}),
    case("D TP S2", "packed/negative_n_segs", lambda x: _tp(x, n_segs=-1), INV, "bad segments"),
    case("D S2", "packed/seg_len_0", lambda x: _tp(x, seg_len=0), INV, "bad segments"),
    case("D S2", "packed/null_counts", lambda x: _tp(x, counts=None), INV, "bad segments"),
    case("D TP K T S2", "packed/row_words", lambda x: _tp(x, row_words=7), INV, "row_words 7 != 2 + value columns"),
    case("TP K T", "packed/no_such_columns", _tp, INV, "packed rows carry no key-hash, key-row or null-flag columns"),
    case("D S2", "packed/no_segments_null_rows", lambda x: _tp(x, 0, 4, None, None), 0),
    case("D S2", "packed/null_rows", lambda x: _tp(x, rows=None), INV, "null rows"),
    case("S2", "packed/session_accepted", _tp, 0),
    # ---- the count handle's segment pushes
    kind_texts(fw_push_device_count_segments, ONLY_COUNT),
    kind_texts(fw_push_device_count_packed_segments, ONLY_COUNT),
    case("C2", "count_segments/negative_n_segs", lambda x: _count_segments(x, n_segs=-1), INV, "bad segments"),
    case("C2", "count_segments/seg_len_0", lambda x: _count_segments(x, seg_len=0), INV, "bad segments"),
    case("C2", "count_segments/null_counts", lambda x: _count_segments(x, counts=None), INV, "bad segments"),
    case("C2", "count_segments/seg_len_2_32", lambda x: _count_segments(x, seg_len=1 << 32), INV, ORDINALS),
    case("C2", "count_segments/rows_2_32", lambda x: _count_segments(x, n_segs=1 << 16, seg_len=1 << 16), INV, ORDINALS),
    case("C2 CP2", "count_segments/no_segments_null_columns", lambda x: _count_segments(x, 0, 4, None, None, None, None), 0),
    case("C2", "count_segments/null_key", lambda x: _count_segments(x, key=None), INV, "null key column"),
    case("CP2", "count_segments/no_hashes", lambda x: _count_segments(x, kh=None), INV, "key_hash column required"),
    case("C2", "count_segments/null_value", lambda x: _count_segments(x, value=None), INV, VAL_NULL),
    case("C2", "count_packed/negative_n_segs", lambda x: _cp(x, n_segs=-1), INV, "bad segments"),
    case("C2", "count_packed/null_counts", lambda x: _cp(x, counts=None), INV, "bad segments"),
    case("C2 CP2", "count_packed/row_words", lambda x: _cp(x, row_words=7), INV, "row_words 7 != 2 + value columns"),
    case("C2", "count_packed/row_words_and_seg_len_2_32", lambda x: _cp(x, seg_len=1 << 32, row_words=7), INV,
         "row_words 7 != 2 + value columns"),
    case("CP2", "count_packed/key_hash", _cp, INV, "packed rows carry no key-hash column"),
    case("C2", "count_packed/seg_len_2_32", lambda x: _cp(x, seg_len=1 << 32), INV, ORDINALS),
    case("C2", "count_packed/no_segments_null_rows", lambda x: _cp(x, 0, 4, None, None), 0),
    case("C2", "count_packed/null_rows", lambda x: _cp(x, rows=None), INV, "null rows"),
    # ---- the record count handle's pair
    kind_texts(fw_push_device_count_record_packed_segments, ONLY_RECORD),
    kind_texts(fw_count_record_rows, ONLY_RECORD),
    case("R2", "record/negative_n_segs", lambda x: _rp(x, n_segs=-1), INV, "bad segments"),
    case("R2", "record/seg_len_0", lambda x: _rp(x, seg_len=0), INV, "bad segments"),
    case("R2", "record/null_counts", lambda x: _rp(x, counts=None), INV, "bad segments"),
    case("R2 RP2", "record/row_words", lambda x: _rp(x, row_words=7), INV, REC + ": row_words 7 != 2 + value columns (1 record fields)"),
    case("RP2", "record/key_hash", _rp, INV, REC + ": packed rows carry no key-hash column"),
    case("R2", "record/seg_len_above_max_batch_rows", lambda x: _rp(x, seg_len=CAP + 1), INV,
         REC + ": seg_len = 1025 exceeds max_batch_rows (1024)"),
    case("R2", "record/no_segments_null_rows", lambda x: _rp(x, 0, 4, None, None), 0),
    case("R2", "record/null_rows", lambda x: _rp(x, rows=None), INV, "null rows"),
    case("R2", "record_rows/null_out", lambda x: _rec_rows(x, out=False), INV, "null argument"),
    case("R2", "record_rows/row_words", lambda x: _rec_rows(x, row_words=7), INV,
         "fw_count_record_rows: row_words 7 != 2 + value columns (1 record fields)"),
    case("R2", "record_rows/negative_n_rows", lambda x: _rec_rows(x, n_rows=-1), INV, "fw_count_record_rows: bad rows"),
    case("R2", "record_rows/n_rows_2_32", lambda x: _rec_rows(x, n_rows=1 << 32), INV, "fw_count_record_rows: bad rows"),
    case("R2", "record_rows/null_rows", lambda x: _rec_rows(x, rows=None), INV, "fw_count_record_rows: bad rows"),
    case("R2", "record_rows/before_any_push", _rec_rows, STATE, "fw_count_record_rows without a push"),
    case("R2", "record_rows/no_rows_before_any_push", lambda x: _rec_rows(x, rows=None, n_rows=0), STATE, "fw_count_record_rows without a push"),
    # ---- fw_advance_device
    case("T S1 C1", "advance_device/null_watermark", lambda x: x.L.fw_advance_device(x.h, None), INV, "null argument"),
    case("S1", "advance_device/session_of_parallelism_1", lambda x: x.L.fw_advance_device(x.h, x.z), INV,
         "fw_advance_device: not for session windows (the late test needs the watermark on the host)"),
    # ---- the result entries
    case("T C1 S1", "results/null_out", lambda x: x.L.fw_results(x.h, None, 1), INV, "null argument"),
    kind_texts(fw_results_async, {"C1": COUNT, "S1": SESSION}),
    kind_texts(fw_results_ready, {"C1": COUNT, "S1": SESSION}),
    kind_texts(fw_results_device, {"C1": COUNT, "S1": SESSION}),
    kind_texts(fw_results_device_segments, {"C1": COUNT, "S1": SESSION}),
    case("K", "results_async/key_rows", fw_results_async, INV, KEYROW_RESULTS),
    case("K", "results_device/key_rows", fw_results_device, INV, KEYROW_RESULTS),
    case("K", "results_device_segments/key_rows", fw_results_device_segments, INV, KEYROW_RESULTS),
    case("T C1", "results_ready/null_out", lambda x: x.L.fw_results_ready(x.h, None), INV, "null argument"),
    case("T C1", "results_device/null_out", lambda x: x.L.fw_results_device(x.h, None, C.byref(x.dn)), INV, "null argument"),
    case("T", "results_device/null_d_n", lambda x: x.L.fw_results_device(x.h, C.byref(x.res), None), INV, "null argument"),
    case("T C1", "results_device_segments/null_out", lambda x: x.L.fw_results_device_segments(x.h, None), INV, "null argument"),
    case("T K", "results_ready/nothing_outstanding", fw_results_ready, STATE, "fw_results_ready without an outstanding fw_results_async"),
    case("T", "results_async/first", fw_results_async, 0),
    case("T", "results_async/second", fw_results_async, 0),
    case("T", "results_async/third", fw_results_async, 0),
    case("T", "results_async/fourth", fw_results_async, STATE, "3 result collections outstanding: fw_results_ready first"),
    case("T", "results_ready/first", fw_results_ready, 0),
    case("T", "results_ready/second", fw_results_ready, 0),
    case("T", "results_ready/third", fw_results_ready, 0),
    case("T", "results_ready/all_returned", fw_results_ready, STATE, "fw_results_ready without an outstanding fw_results_async"),
    # ---- fw_first_element_events / fw_late_records
    kind_texts(fw_first_element_events, {"C1": COUNT, "S1": SESSION}),
    case("T C1", "first_element_events/null_out", lambda x: x.L.fw_first_element_events(x.h, None), INV, "null argument"),
    case("T K", "first_element_events/not_tracked", fw_first_element_events, STATE,
         "the operator does not track first elements (ds_first_ordinals = 0)"),
    case("D R1 R2", "first_element_events/accepted", fw_first_element_events, 0),
    kind_texts(fw_late_records, {"C1": COUNT}),
    case("T S1", "late_records/null_out", lambda x: x.L.fw_late_records(x.h, None), INV, "null argument"),
    case("T K S1 S2 SQ", "late_records/no_side_output", fw_late_records, STATE, NO_SIDE),
    case("D", "late_records/accepted", fw_late_records, 0),
], [])

NULL_HANDLE = [
    ("fw_reserve", lambda L: L.fw_reserve(None, 1, C.byref(abi.fw_host_cols())), "null argument"),
    ("fw_commit", lambda L: L.fw_commit(None, 1), "null handle"),
    ("fw_commit_delta32", lambda L: L.fw_commit_delta32(None, 1, 0, None), "null handle"),
    ("fw_push_device_key_rows", lambda L: L.fw_push_device_key_rows(None, 1, None, None, None, None, None), "null handle"),
    ("fw_push_device", lambda L: L.fw_push_device(None, 1, None, None, None, None, None), "null handle"),
    ("fw_push_device_segments", lambda L: L.fw_push_device_segments(None, -1, 0, None, None, None, None, None, None), "null handle"),
    ("fw_push_device_packed_segments", lambda L: L.fw_push_device_packed_segments(None, -1, 0, None, None, 0), "null handle"),
    ("fw_push_device_count_segments", lambda L: L.fw_push_device_count_segments(None, -1, 0, None, None, None, None), "null handle"),
    ("fw_push_device_count_packed_segments", lambda L: L.fw_push_device_count_packed_segments(None, -1, 0, None, None, 0), "null handle"),
    ("fw_push_device_count_record_packed_segments",
     lambda L: L.fw_push_device_count_record_packed_segments(None, -1, 0, None, None, 0), "null handle"),
    ("fw_count_record_rows", lambda L: L.fw_count_record_rows(None, None, 0, 0, C.byref(abi.fw_record_rows())), "null argument"),
    ("fw_advance", lambda L: L.fw_advance(None, 0), "null handle"),
    ("fw_advance_device", lambda L: L.fw_advance_device(None, None), "null argument"),
    ("fw_flush", lambda L: L.fw_flush(None), "null handle"),
    ("fw_results", lambda L: L.fw_results(None, C.byref(abi.fw_result()), 1), "null argument"),
    ("fw_results_async", lambda L: L.fw_results_async(None), "null handle"),
    ("fw_results_ready", lambda L: L.fw_results_ready(None, C.byref(abi.fw_result())), "null argument"),
    ("fw_results_device", lambda L: L.fw_results_device(None, C.byref(abi.fw_result()), C.byref(C.c_void_p())), "null argument"),
    ("fw_results_device_segments", lambda L: L.fw_results_device_segments(None, C.byref(abi.fw_result_segments())), "null argument"),
    ("fw_first_element_events", lambda L: L.fw_first_element_events(None, C.byref(abi.fw_ordinal_events())), "null argument"),
    ("fw_late_records", lambda L: L.fw_late_records(None, C.byref(abi.fw_late_rows())), "null argument"),
    ("fw_results_reset", lambda L: L.fw_results_reset(None), "null handle"),
]


@pytest.mark.parametrize("name,call,msg", NULL_HANDLE, ids=[c[0] for c in NULL_HANDLE])
def test_null_handle(name, call, msg):
    assert (call(_native.lib()), _last_error()) == (INV, msg)


# ---- the good push of each kind, and what it leaves
def _good_push(x):
    L, k = x.L, x.kind
    kh = x.kh if x.cfg.key_hash == PRE else None
    nul = VA(x.nul) if x.cfg.nullable_cols else None
    if k == "K":
        _native.check(L.fw_push_device_key_rows(x.h, 8, x.kro, x.krb, x.ts, VA(x.val), nul))
    elif k in ("C2", "CP2"):
        _native.check(L.fw_push_device_count_segments(x.h, 2, 4, x.counts, x.key, kh, x.val))
    elif k == "R2":
        _native.check(L.fw_push_device_count_record_packed_segments(x.h, 2, 4, x.counts, x.rows, 3))
        _native.check(L.fw_count_record_rows(x.h, x.rows, 3, 8, C.byref(x.rr)))
        assert (x.rr.n_fields, x.rr.n_res) == (1, 4)
    elif k == "S2":
        _native.check(L.fw_push_device_segments(x.h, 2, 4, x.counts, x.key, x.ts, None, VA(x.val), None))
    else:
        _native.check(L.fw_push_device(x.h, 8, x.key, x.ts, kh, VA(x.val), nul))
    _native.check(L.fw_advance(x.h, T0 + 10**6))


def _column(ptr, n):
    if n == 0 or not ptr:
        return [None] * n
    return np.ctypeslib.as_array(ptr, shape=(n,)).tolist()


def _read(x):
    """(sorted rows, counters) through fw_results' host copy and fw_get_stats"""
    r, s = abi.fw_result(), abi.fw_stats()
    _native.check(x.L.fw_results(x.h, C.byref(r), 1))
    n = int(r.n)
    rows = sorted(zip(_column(r.key, n), _column(r.window_start, n), _column(r.window_end, n), _column(r.values[0], n),
                      _column(r.null_mask, n), [repr(v) for v in _column(r.first_ord, n)]))
    _native.check(x.L.fw_get_stats(x.h, C.byref(s)))
    return rows, {f: getattr(s, f) for f in ("live_state_entries", "error_flags", "num_late_records_dropped", "num_fired_windows")}


@pytest.mark.parametrize("kind", list(CONFIGS))
def test_entry_refusals(kind):
    data = _data(CONFIGS[kind]())
    dirty, twin = Ctx(kind, data), Ctx(kind, data)
    try:
        cases = [c for c in CASES if c[0] == kind]
        assert cases
        got = []
        for _, name, call, rc, msg in cases:
            r = call(dirty)
            got.append((name, r, _last_error() if r else ""))
            if rc == 0:   # the twin makes the accepted calls only
                assert call(twin) == 0, name
        assert got == [(name, rc, msg) for _, name, _, rc, msg in cases]
        _good_push(dirty)
        _good_push(twin)
        rows, counters = _read(dirty)
        assert (rows, counters) == _read(twin)
        assert len(rows) == 4 and counters["error_flags"] == 0 and counters["num_late_records_dropped"] == 0
    finally:
        dirty.close()
        twin.close()


def test_every_kind_and_entry_has_cases():
    assert {c[0] for c in CASES} == set(CONFIGS)
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)
