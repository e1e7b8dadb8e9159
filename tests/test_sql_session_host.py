"""The SQL SESSION window TVF aggregate without a device: the checker against the DataStream
checker, the host entry points (the arithmetic the session kernels run: fw_host_sql_session_words /
_add / _result) against the checker, the result rules at their edges, and validation."""
import ctypes as C
import random
import struct

import pytest
from session_window_reference import SessionWindowReference
from sql_session_reference import SqlSessionReference

from flink_amd import _native, abi
from flink_amd.table.session_window_agg import SessionWindowAggOperator, is_gpu_eligible

REL_TOL = 1e-9   # DESIGN.md 4 "Float order": DOUBLE sums
T = {"BIGINT": abi.T_I64, "INT": abi.T_I32, "DOUBLE": abi.T_F64}


def _cfg(gap, aggs, value_types, nullable=(), **kw):
    d = dict(api=abi.API_SQL, window_kind=abi.WIN_SESSION, size_ms=gap,
             aggs=[(abi.AGG_NAMES[k], c, T[t]) for k, c, t in aggs], value_col_types=[T[t] for t in value_types],
             key_hash=abi.KEYHASH_BINROW_BIGINT, nullable_cols=nullable)
    d.update(kw)
    return abi.make_config(**d)


def _bits(v, typ):
    if v is None:
        return 0
    return struct.unpack("<q", struct.pack("<d", v))[0] if typ == "DOUBLE" else int(v)


def _unbits(b, is_double):
    return struct.unpack("<d", struct.pack("<q", b))[0] if is_double else b


# one layout per accumulator word count; (aggs, value types, nullable columns, words)
LAYOUTS = {
    1: ([("SUM", 0, "BIGINT")], ["BIGINT"], ()),
    2: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT")], ["BIGINT"], (0,)),
    4: ([("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT"), ("MIN", 1, "INT"), ("COUNT_STAR", 0, "BIGINT"), ("AVG", 0, "BIGINT")],
        ["BIGINT", "INT"], (0,)),
    8: ([("SUM", 0, "BIGINT"), ("AVG", 1, "DOUBLE"), ("MIN", 2, "INT"), ("MAX", 2, "INT"), ("COUNT", 1, "DOUBLE"),
         ("COUNT_STAR", 0, "BIGINT"), ("SUM", 1, "DOUBLE")], ["BIGINT", "DOUBLE", "INT"], (0, 1, 2)),
}


class HostSqlSessions:
    """one key's session list in host arrays, driven only through the fw_host_sql_session_* entry points"""

    def __init__(self, cfg, aggs, value_types, capacity=64):
        self.cfg, self.aggs, self.types, self.cap = cfg, aggs, value_types, capacity
        self.nw = abi.host_sql_session_words(cfg)
        self.s = (C.c_int64 * capacity)()
        self.e = (C.c_int64 * capacity)()
        self.a = (C.c_int64 * (capacity * self.nw))()
        self.n = 0

    def add(self, watermark, ts, row):
        vals = [_bits(v, t) for v, t in zip(row, self.types)]
        out, self.n = abi.host_sql_session_add(self.cfg, watermark, ts, vals, [v is None for v in row], self.s, self.e, self.a,
                                               self.n, self.cap)
        assert out in (0, 1)
        return bool(out)

    def result(self, i):
        vals, nm = abi.host_sql_session_result(self.cfg, [self.a[i * self.nw + w] for w in range(self.nw)])
        out = []
        for g, (kind, _, typ) in enumerate(self.aggs):
            dbl = abi.result_is_double(abi.AGG_NAMES[kind], T[typ])
            out.append(None if nm >> g & 1 else _unbits(vals[g], dbl))
        return out

    def sessions(self):
        return [(self.s[i], self.e[i], self.result(i)) for i in range(self.n)]

    def fire(self, watermark):
        """what fw_advance does to the list: sessions with end - 1 <= watermark leave"""
        rows = self.sessions()
        words = [[self.a[i * self.nw + w] for w in range(self.nw)] for i in range(self.n)]
        keep = [i for i in range(self.n) if rows[i][1] - 1 > watermark]
        fired = [rows[i] for i in range(self.n) if rows[i][1] - 1 <= watermark]
        for j, i in enumerate(keep):
            self.s[j], self.e[j] = rows[i][0], rows[i][1]
            for w in range(self.nw):
                self.a[j * self.nw + w] = words[i][w]
        self.n = len(keep)
        return fired


def _same(got, want):
    if isinstance(want, float) and got is not None:
        return abs(got - want) <= REL_TOL * max(abs(want), 1e-300)
    return got == want


def _check_sessions(h, r, key):
    want = [(w[0], w[1], [a.value(x) for a, x in zip(r.aggs, w[2])]) for w in r.windows.get(key, [])]
    got = h.sessions()
    assert [(s, e) for s, e, _ in got] == [(s, e) for s, e, _ in want]
    for (_, _, gv), (_, _, wv) in zip(got, want):
        assert all(_same(g, w) for g, w in zip(gv, wv)), (gv, wv)


def _random_row(rng, types, nullable, p_null=0.3):
    row = []
    for c, t in enumerate(types):
        if c in nullable and rng.random() < p_null:
            row.append(None)
        elif t == "DOUBLE":
            row.append(rng.uniform(0.5, 100.0))
        elif t == "INT":
            row.append(rng.randint(-1000, 1000))
        else:
            row.append(rng.randint(-10**12, 10**12))
    return row


# ---- the checker against the DataStream checker -------------------------------------------------------
@pytest.mark.parametrize("kind,fn", [("SUM", "sum"), ("MIN", "min"), ("MAX", "max"), ("COUNT_STAR", "count")])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_agrees_with_datastream_reference(kind, fn, seed):
    """one NOT NULL BIGINT aggregate: both restatements emit the same rows, late rows in both orders included"""
    rng = random.Random(seed)
    gap = 50
    sql, ds = SqlSessionReference(gap, [(kind, 0, "BIGINT")]), SessionWindowReference(gap, (fn, "LONG"))
    t0 = 0
    for _ in range(12):
        keys = [rng.randint(0, 5) for _ in range(60)]
        # rows around and below the watermark: late ones that join a live session, and ones that do not
        ts = [t0 + rng.randint(-150, 300) for _ in range(60)]
        vals = [rng.randint(-1000, 1000) for _ in range(60)]
        assert sql.process(keys, ts, [[v] for v in vals]) == ds.process(keys, ts, vals)
        t0 += rng.randint(20, 200)
        assert sql.process_watermark(t0) == ds.process_watermark(t0)
    assert sql.late_dropped == ds.late_dropped > 0
    # "late A then B" keeps B only; "B then A" keeps both (A joins B's session)
    for order, kept in (((100, 140), [False, True]), ((140, 100), [True, True])):
        r = SqlSessionReference(gap, [(kind, 0, "BIGINT")])
        r.process_watermark(160)                       # ts 100: window [100, 150) is late; ts 140: [140, 190) is not
        assert [r.add(1, ts, [5]) for ts in order] == kept


# ---- the host arithmetic against the checker -----------------------------------------------------------
@pytest.mark.parametrize("nw", sorted(LAYOUTS))
@pytest.mark.parametrize("seed", [11, 12])
def test_host_session_arithmetic_matches_reference(nw, seed):
    aggs, types, nullable = LAYOUTS[nw]
    cfg = _cfg(40, aggs, types, nullable)
    h, r = HostSqlSessions(cfg, aggs, types), SqlSessionReference(40, aggs)
    assert h.nw == nw
    rng = random.Random(seed)
    t0, key, merges3 = 0, 9, 0
    for step in range(300):
        ts = t0 + rng.choice([rng.randint(-900, 600), rng.randint(0, 60)])
        before = len(r.windows.get(key, []))
        row = _random_row(rng, types, nullable)
        assert h.add(r.watermark, ts, row) == r.add(key, ts, row)
        merges3 += before - len(r.windows.get(key, [])) >= 1   # a bridge: the row joined two sessions or more
        _check_sessions(h, r, key)
        if step % 25 == 24:
            t0 += rng.randint(30, 150)
            fired = h.fire(t0)
            want = r.process_watermark(t0)
            assert [(s, e) for s, e, _ in fired] == [(row[-2], row[-1]) for row in want]
            for (_, _, gv), wrow in zip(fired, want):
                assert all(_same(g, w) for g, w in zip(gv, wrow[1:-2]))
    assert merges3 > 0 and r.late_dropped > 0


@pytest.mark.parametrize("nw", sorted(LAYOUTS))
def test_host_bridge_touching_and_late_candidates(nw):
    aggs, types, nullable = LAYOUTS[nw]
    gap = 10
    h, r = HostSqlSessions(_cfg(gap, aggs, types, nullable), aggs, types), SqlSessionReference(gap, aggs)
    rng = random.Random(nw)

    def add(ts):
        row = _random_row(rng, types, nullable)
        got, want = h.add(r.watermark, ts, row), r.add(3, ts, row)
        assert got == want
        _check_sessions(h, r, 3)
        return got
    for ts in (100, 130, 160):                 # three sessions
        assert add(ts)
    assert len(h.sessions()) == 3
    assert add(110) and len(h.sessions()) == 3   # [110, 120) touches [100, 110): they merge
    assert add(120) and len(h.sessions()) == 2   # a bridge: [120, 130) touches [100, 120) and [130, 140), three windows merge
    assert add(150) and len(h.sessions()) == 2   # [150, 160) touches [160, 170) only
    assert add(140) and len(h.sessions()) == 1   # a bridge again
    assert h.sessions()[0][:2] == (100, 170)
    h.fire(200)
    r.process_watermark(200)
    assert h.n == 0
    assert not add(150)                          # late, alone: dropped
    assert add(195) and not add(170)             # [195, 205) is live; [170, 180) does not reach it
    assert add(185) and add(176) and add(170)    # a backward chain of late candidates, each joining the live session
    assert h.sessions()[0][:2] == (170, 205) and r.late_dropped == 2


def test_host_capacity():
    aggs, types, nullable = LAYOUTS[4]
    h = HostSqlSessions(_cfg(10, aggs, types, nullable), aggs, types, capacity=3)
    for ts in (0, 100, 200):
        assert h.add(-1, ts, [1, 1])
    with pytest.raises(_native.FlinkWinError) as e:
        h.add(-1, 300, [1, 1])
    assert e.value.code == abi.FW_E_CAPACITY and h.n == 3
    assert h.add(-1, 105, [1, 1]) and h.n == 3      # a row that joins a session still fits


# ---- result rules at the edges ------------------------------------------------------------------------------
def _one_session(aggs, types, nullable, rows, gap=1000):
    h, r = HostSqlSessions(_cfg(gap, aggs, types, nullable), aggs, types), SqlSessionReference(gap, aggs)
    for i, row in enumerate(rows):
        assert h.add(r.watermark, i, row) and r.add(1, i, row)
    assert h.n == 1
    want = r.process_watermark(10**9)[0][1:-2]
    got = h.result(0)
    assert list(want) == got
    return got


def test_session_of_only_null_values():
    aggs = [("SUM", 0, "BIGINT"), ("COUNT", 0, "BIGINT"), ("MIN", 0, "BIGINT"), ("MAX", 0, "BIGINT"), ("AVG", 0, "BIGINT"),
            ("COUNT_STAR", 0, "BIGINT")]
    assert _one_session(aggs, ["BIGINT"], (0,), [[None]] * 3) == [None, 0, None, None, None, 3]   # COUNT(col) = 0 next to SUM = NULL
    assert _one_session(aggs, ["BIGINT"], (0,), [[None], [7], [None]]) == [7, 1, 7, 7, 7, 3]       # a non-NULL row joins it


def test_sum_int_wraps_at_32_bits():
    aggs = [("SUM", 0, "INT"), ("AVG", 0, "INT")]
    got = _one_session(aggs, ["INT"], (), [[2**31 - 1], [1]])
    assert got == [-2**31, 2**30]       # SUM(INT) wraps; AVG(INT) divides the BIGINT sum 2^31 by 2


def test_avg_truncates_toward_zero():
    assert _one_session([("AVG", 0, "BIGINT")], ["BIGINT"], (), [[-7], [0]]) == [-3]     # -7 / 2 = -3 in Java, not -4
    assert _one_session([("AVG", 0, "INT")], ["INT"], (), [[-7], [0], [0]]) == [-2]
    # the BIGINT sum wraps at 64 bits before the division: 3 * -2^62 = 2^62 (mod 2^64)
    assert _one_session([("AVG", 0, "BIGINT")], ["BIGINT"], (), [[-2**62], [-2**62], [-2**62]]) == [2**62 // 3]


def test_avg_int_result_width():
    # the sum of AVG(INT) is a BIGINT: 3 * (2^31 - 1) does not wrap; the quotient is an INT
    assert _one_session([("AVG", 0, "INT")], ["INT"], (), [[2**31 - 1]] * 3) == [2**31 - 1]


def test_avg_double_and_sum_double():
    got = _one_session([("AVG", 0, "DOUBLE"), ("SUM", 0, "DOUBLE")], ["DOUBLE"], (0,), [[1.5], [None], [2.5]])
    assert got == [2.0, 4.0]


# ---- validation without a device -----------------------------------------------------------------------------
_OK = dict(gap=3000, aggs=[("SUM", 0, "BIGINT")], types=["BIGINT"])
_REJECTED = [
    (dict(aggs=[("MIN", 0, "DOUBLE")], types=["DOUBLE"]), "MIN / MAX over DOUBLE"),
    (dict(aggs=[("SUM", 0, "BIGINT"), ("MAX", 1, "DOUBLE")], types=["BIGINT", "DOUBLE"]), "MIN / MAX over DOUBLE"),
    (dict(shift_zone="Europe/Berlin"), "TIMESTAMP_LTZ"),
    (dict(agg_phase=abi.PHASE_LOCAL), "agg_phase"),
    (dict(agg_phase=abi.PHASE_GLOBAL), "agg_phase"),
    (dict(key_hash=abi.KEYHASH_KEYROW), "KEYROW"),
    (dict(key_hash=abi.KEYHASH_LONG), "DataStream"),
    (dict(key_hash=abi.KEYHASH_INT), "DataStream"),
    (dict(late_side_output=True), "late_side_output"),
    (dict(allowed_lateness_ms=5), "allowed_lateness_ms"),
    (dict(ds_first_ordinals=True), "ds_first_ordinals"),
    (dict(offset_ms=1), "offset_ms"),
    (dict(slide_ms=1), "slide_ms"),
    (dict(gap=0), "gap (size_ms) must be > 0"),
    (dict(gap=(1 << 40) + 1), "2^40"),
    (dict(aggs=[("SUM", c, "BIGINT") for c in range(5)], types=["BIGINT"] * 5, nullable_cols=(0, 1, 2, 3, 4)),
     "too many accumulator words"),   # five (sum, non-NULL count) pairs: ten words
]


@pytest.mark.parametrize("overrides,message", _REJECTED, ids=[m.split()[0] + str(i) for i, (_, m) in enumerate(_REJECTED)])
def test_invalid_sql_session_configs_fail_without_device(overrides, message):
    kw = dict(_OK)
    kw.update(overrides)
    cfg = _cfg(kw.pop("gap"), kw.pop("aggs"), kw.pop("types"), kw.pop("nullable_cols", ()), **kw)
    L = _native.lib()
    h = C.c_void_p()
    assert L.fw_create(C.byref(cfg), C.byref(h)) == abi.FW_E_INVALID and not h.value
    assert message in L.fw_last_error().decode()
    nw, n, out, nm = C.c_int32(), C.c_int32(0), C.c_int32(), C.c_uint32()
    a = (C.c_int64 * 64)()
    f = (C.c_uint8 * 8)()
    assert L.fw_host_sql_session_words(C.byref(cfg), C.byref(nw)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()
    assert L.fw_host_sql_session_add(C.byref(cfg), 0, 0, a, f, a, a, a, C.byref(n), 4, C.byref(out)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()
    assert L.fw_host_sql_session_result(C.byref(cfg), a, a, C.byref(nm)) == abi.FW_E_INVALID
    assert message in L.fw_last_error().decode()


def test_count_star_index_is_accepted_and_ignored():
    aggs = [("SUM", 0, "BIGINT"), ("COUNT_STAR", 0, "BIGINT")]
    assert abi.host_sql_session_words(_cfg(10, aggs, ["BIGINT"], count_star_index=1)) == 2
    assert abi.host_sql_session_words(_cfg(10, aggs, ["BIGINT"], (0,), count_star_index=1)) == 3


def test_host_entry_points_keep_to_their_form():
    L = _native.lib()
    sql = _cfg(10, [("SUM", 0, "BIGINT")], ["BIGINT"])
    ds = abi.make_config(api=abi.API_DATASTREAM, window_kind=abi.WIN_SESSION, size_ms=10, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                         value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_LONG)
    s, n, out, nw = (C.c_int64 * 4)(), C.c_int32(0), C.c_int32(), C.c_int32()
    assert L.fw_host_session_add(C.byref(sql), 0, 0, 1, s, s, s, C.byref(n), 4, C.byref(out)) == abi.FW_E_INVALID
    assert "DataStream" in L.fw_last_error().decode()
    assert L.fw_host_sql_session_words(C.byref(ds), C.byref(nw)) == abi.FW_E_INVALID
    assert "FW_API_SQL" in L.fw_last_error().decode()
    for name in ("fw_host_sql_session_words", "fw_host_sql_session_add", "fw_host_sql_session_result"):
        assert hasattr(L, name) and name in _native.EXPORTED
    assert L.fw_abi_version() == 11


def test_python_eligibility_gives_the_same_verdicts():
    aggs, types = [("SUM", 0, "BIGINT"), ("AVG", 1, "DOUBLE")], ["BIGINT", "DOUBLE"]
    assert is_gpu_eligible(3000, aggs, types) == (True, "")
    assert is_gpu_eligible(3000, aggs, types, key_type="HOST_HASHED", conf={"gpu.window-agg.enabled": "true"}) == (True, "")
    cases = [
        (dict(aggs=[("MIN", 1, "DOUBLE")]), "MIN(DOUBLE)"),
        (dict(aggs=[("MAX", 1, "DOUBLE")]), "MAX(DOUBLE)"),
        (dict(shift_time_zone="Europe/Berlin"), "TIMESTAMP_LTZ"),
        (dict(is_event_time=False), "processing-time"),
        (dict(has_distinct=True), "DISTINCT"),
        (dict(needs_retraction=True), "retraction"),
        (dict(key_type=("BIGINT", "VARCHAR")), "key rows"),
        (dict(key_type="VARCHAR"), "host-hashed"),
        (dict(gap_ms=0), "gap"),
        (dict(gap_ms=(1 << 40) + 1), "gap"),
        (dict(aggs=[("LISTAGG", 0, "BIGINT")]), "not a built-in"),
        (dict(aggs=[("SUM", 0, "DECIMAL")]), "not supported"),
        (dict(conf={}), "gpu.window-agg.enabled"),
    ]
    for over, reason in cases:
        kw = dict(gap_ms=3000, aggs=aggs, value_types=types)
        kw.update(over)
        gap, a, t = kw.pop("gap_ms"), kw.pop("aggs"), kw.pop("value_types")
        ok, why = is_gpu_eligible(gap, a, t, **kw)
        assert not ok and reason in why, (over, why)
    with pytest.raises(ValueError, match="MIN\\(DOUBLE\\)"):
        SessionWindowAggOperator(3000, [("MIN", 1, "DOUBLE")], types)
    # an eligible operator's configuration is one fw_create accepts up to the device: its plan exists
    op = SessionWindowAggOperator(3000, aggs, types, nullable_cols=(1,))
    assert abi.host_sql_session_words(op.cfg) == 3
