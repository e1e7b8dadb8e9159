"""Every refusal of the session planner, per kind: one table of broken configurations crossed with the
four DataStream session kinds and the SQL form, each through a fw_host_* entry point that plans without
a device, asserting the exact return code and message.  The cases that break two rules at once pin
which check wins, which differs between the kinds.  A second table does the same for the four
fw_host_session_add* wrappers' own argument checks.  The expected literals were written down from the
library as it stood when each kind had a planner and a host routine of its own, not from the code
under test."""
import ctypes as C

import pytest

from flink_amd import _native, abi

BIG = (1 << 40) + 1
KINDS = ("static", "dynamic", "late", "dynamic_late", "sql")
WINDOW_KIND = {"static": abi.WIN_SESSION, "dynamic": abi.WIN_SESSION_DYNAMIC, "late": abi.WIN_SESSION_LATENESS,
               "dynamic_late": abi.WIN_SESSION_DYNAMIC_LATENESS, "sql": abi.WIN_SESSION}


def good_config(kind):
    if kind == "sql":
        return abi.make_config(api=abi.API_SQL, window_kind=abi.WIN_SESSION, size_ms=100, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                               value_col_types=[abi.T_I64], key_hash=abi.KEYHASH_BINROW_BIGINT, state_capacity=1 << 10,
                               max_batch_rows=1 << 10, output_capacity=1 << 10)
    cols = [abi.T_I64, abi.T_I64] if "dynamic" in kind else [abi.T_I64]
    return abi.make_config(api=abi.API_DATASTREAM, window_kind=WINDOW_KIND[kind], size_ms=100, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                           value_col_types=cols, key_hash=abi.KEYHASH_LONG, allowed_lateness_ms=10 if "late" in kind else 0,
                           state_capacity=1 << 10, max_batch_rows=1 << 10, output_capacity=1 << 10)


def _set(**fields):
    def breaker(c):
        for name, v in fields.items():
            setattr(c, name, v)
    return breaker


def _agg(**fields):
    def breaker(c):
        for name, v in fields.items():
            setattr(c.aggs[0], name, v)
    return breaker


def _wrong_api(c):
    c.api = abi.API_DATASTREAM if c.api == abi.API_SQL else abi.API_SQL


def _type_mismatch(c):
    c.aggs[0].type = abi.T_F64   # the value column stays T_I64


def _gap_column_type(c):
    c.value_col_types[1] = abi.T_F64


def _input_col_1(c):   # (two columns of the aggregate's type, so that only the dynamic rule can object)
    c.aggs[0].input_col = 1
    c.n_value_cols = 2
    c.value_col_types[1] = abi.T_I64


def _both(*breakers):
    def breaker(c):
        for b in breakers:
            b(c)
    return breaker


BROKEN = {
    "none": _set(),
    "wrong_api": _wrong_api,
    "n_aggs_0": _set(n_aggs=0),
    "n_aggs_2": _set(n_aggs=2),
    "min_by": _agg(kind=abi.AGG_MINBY),
    "bad_type": _agg(type=7),
    "type_mismatch": _type_mismatch,
    "gap_0": _set(size_ms=0),
    "gap_big": _set(size_ms=BIG),
    "slide": _set(slide_ms=5),
    "offset": _set(offset_ms=5),
    "lateness_neg": _set(allowed_lateness_ms=-1),
    "lateness_big": _set(allowed_lateness_ms=BIG),
    "late_side_output_2": _set(late_side_output=2),
    "nullable_cols": _set(nullable_cols=1),
    "tz_n": _set(tz_n=1),
    "two_phase": _set(agg_phase=abi.PHASE_LOCAL),
    "keyrow_key": _set(key_hash=abi.KEYHASH_KEYROW),
    "max_batch_rows_0": _set(max_batch_rows=0),
    "output_capacity_0": _set(output_capacity=0),
    # the dynamic kinds' own rules
    "one_value_col": _set(n_value_cols=1),
    "gap_col_not_i64": _gap_column_type,
    "input_col_1": _input_col_1,
    # two rules at once: which check wins
    "wrong_api_and_lateness_big": _both(_wrong_api, _set(allowed_lateness_ms=BIG)),
    "lateness_big_and_slide": _both(_set(allowed_lateness_ms=BIG), _set(slide_ms=5)),
    "lateness_big_and_one_value_col": _both(_set(allowed_lateness_ms=BIG), _set(n_value_cols=1)),
    "lateness_neg_and_output_capacity_0": _both(_set(allowed_lateness_ms=-1), _set(output_capacity=0)),
    "n_aggs_2_and_gap_0": _both(_set(n_aggs=2), _set(size_ms=0)),
    "gap_col_not_i64_and_input_col_1": _both(_gap_column_type, _input_col_1),
}


def _last_error():
    msg = _native.lib().fw_last_error()
    return msg.decode() if msg else ""


def plan(kind, cfg):
    """(return code, message) of planning ``cfg`` through the kind's host entry point; no device call"""
    L = _native.lib()
    s, e, a = ((C.c_int64 * 4)() for _ in range(3))
    n, out, at = C.c_int32(0), C.c_int32(-7), C.c_int32(-7)
    if kind == "sql":
        rc = L.fw_host_sql_session_words(C.byref(cfg), C.byref(n))
    elif kind == "static":
        rc = L.fw_host_session_add(C.byref(cfg), 0, 0, 1, s, e, a, C.byref(n), 4, C.byref(out))
    elif kind == "dynamic":
        rc = L.fw_host_session_add_gap(C.byref(cfg), 0, 0, 1, 1, s, e, a, C.byref(n), 4, C.byref(out))
    elif kind == "late":
        rc = L.fw_host_session_add_late(C.byref(cfg), 0, 0, 1, s, e, a, C.byref(n), 4, C.byref(out), C.byref(at))
    else:
        rc = L.fw_host_session_add_gap_late(C.byref(cfg), 0, 0, 1, 1, s, e, a, C.byref(n), 4, C.byref(out), C.byref(at))
    return rc, (_last_error() if rc else "")


def plan_case(kind, case):
    cfg = good_config(kind)
    BROKEN[case](cfg)
    return plan(kind, cfg)


# PLAN_EXPECTED[case][kind] = (return code, message)
PLAN_EXPECTED = {'none': {'static': (0, ''), 'dynamic': (0, ''), 'late': (0, ''), 'dynamic_late': (0, ''), 'sql': (0, '')},
 'wrong_api': {'static': (-1,
                          'FW_KEYHASH_LONG / FW_KEYHASH_INT are DataStream key hashes; a SQL session takes BINROW_BIGINT / BINROW_INT / PRECOMPUTED '
                          'keys'),
               'dynamic': (-1, 'FW_WIN_SESSION (EventTimeSessionWindows) is a DataStream window: api must be FW_API_DATASTREAM'),
               'late': (-1,
                        'FW_WIN_SESSION_LATENESS (EventTimeSessionWindows with allowedLateness) is a DataStream window: api must be '
                        'FW_API_DATASTREAM'),
               'dynamic_late': (-1, 'FW_WIN_SESSION (EventTimeSessionWindows) is a DataStream window: api must be FW_API_DATASTREAM'),
               'sql': (-1, 'fw_host_sql_session_words needs a FW_WIN_SESSION configuration with api FW_API_SQL')},
 'n_aggs_0': {'static': (-1, 'n_aggs 0 out of range'),
              'dynamic': (-1, 'n_aggs 0 out of range'),
              'late': (-1, 'n_aggs 0 out of range'),
              'dynamic_late': (-1, 'n_aggs 0 out of range'),
              'sql': (-1, 'n_aggs 0 out of range')},
 'n_aggs_2': {'static': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
              'dynamic': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
              'late': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
              'dynamic_late': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
              'sql': (0, '')},
 'min_by': {'static': (-1, 'session windows: minBy / maxBy run on the reference operator'),
            'dynamic': (-1, 'session windows: minBy / maxBy run on the reference operator'),
            'late': (-1, 'session windows: minBy / maxBy run on the reference operator'),
            'dynamic_late': (-1, 'session windows: minBy / maxBy run on the reference operator'),
            'sql': (-1, 'SQL session windows: agg 0: kind 6 is not COUNT(*) / COUNT / SUM / MIN / MAX / AVG')},
 'bad_type': {'static': (-1, 'session windows: bad aggregate type 7'),
              'dynamic': (-1, 'session windows: bad aggregate type 7'),
              'late': (-1, 'session windows: bad aggregate type 7'),
              'dynamic_late': (-1, 'session windows: bad aggregate type 7'),
              'sql': (-1, 'SQL session windows: agg 0: bad type 7')},
 'type_mismatch': {'static': (-1, 'session windows: type does not match value column type'),
                   'dynamic': (-1, 'session windows: type does not match value column type'),
                   'late': (-1, 'session windows: type does not match value column type'),
                   'dynamic_late': (-1, 'session windows: type does not match value column type'),
                   'sql': (-1, 'agg 0: type does not match value column type')},
 'gap_0': {'static': (-1, 'session gap (size_ms) must be > 0'),
           'dynamic': (-1, 'session gap (size_ms) must be > 0'),
           'late': (-1, 'session gap (size_ms) must be > 0'),
           'dynamic_late': (-1, 'session gap (size_ms) must be > 0'),
           'sql': (-1, 'session gap (size_ms) must be > 0')},
 'gap_big': {'static': (-1, 'session gap (size_ms) must be <= 2^40'),
             'dynamic': (-1, 'session gap (size_ms) must be <= 2^40'),
             'late': (-1, 'session gap (size_ms) must be <= 2^40'),
             'dynamic_late': (-1, 'session gap (size_ms) must be <= 2^40'),
             'sql': (-1, 'session gap (size_ms) must be <= 2^40')},
 'slide': {'static': (-1, 'session windows have no slide (slide_ms must be 0)'),
           'dynamic': (-1, 'session windows have no slide (slide_ms must be 0)'),
           'late': (-1, 'session windows have no slide (slide_ms must be 0)'),
           'dynamic_late': (-1, 'session windows have no slide (slide_ms must be 0)'),
           'sql': (-1, 'session windows have no slide (slide_ms must be 0)')},
 'offset': {'static': (-1, 'session windows have no offset (offset_ms must be 0)'),
            'dynamic': (-1, 'session windows have no offset (offset_ms must be 0)'),
            'late': (-1, 'session windows have no offset (offset_ms must be 0)'),
            'dynamic_late': (-1, 'session windows have no offset (offset_ms must be 0)'),
            'sql': (-1, 'session windows have no offset (offset_ms must be 0)')},
 'lateness_neg': {'static': (-1, 'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)'),
                  'dynamic': (-1, 'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)'),
                  'late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                  'dynamic_late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                  'sql': (-1, 'SQL session windows have no allowed lateness (allowed_lateness_ms must be 0)')},
 'lateness_big': {'static': (-1, 'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)'),
                  'dynamic': (-1, 'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)'),
                  'late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                  'dynamic_late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                  'sql': (-1, 'SQL session windows have no allowed lateness (allowed_lateness_ms must be 0)')},
 'late_side_output_2': {'static': (-1, 'late_side_output must be 0 or 1'),
                        'dynamic': (-1, 'late_side_output must be 0 or 1'),
                        'late': (-1, 'late_side_output must be 0 or 1'),
                        'dynamic_late': (-1, 'late_side_output must be 0 or 1'),
                        'sql': (-1, 'SQL session windows have no late side output (late_side_output must be 0)')},
 'nullable_cols': {'static': (-1, 'session windows take no NULL inputs (nullable_cols must be 0)'),
                   'dynamic': (-1, 'session windows take no NULL inputs (nullable_cols must be 0)'),
                   'late': (-1, 'session windows take no NULL inputs (nullable_cols must be 0)'),
                   'dynamic_late': (-1, 'session windows take no NULL inputs (nullable_cols must be 0)'),
                   'sql': (0, '')},
 'tz_n': {'static': (-1, 'session windows have no time zone (tz_n must be 0)'),
          'dynamic': (-1, 'session windows have no time zone (tz_n must be 0)'),
          'late': (-1, 'session windows have no time zone (tz_n must be 0)'),
          'dynamic_late': (-1, 'session windows have no time zone (tz_n must be 0)'),
          'sql': (-1, 'SQL session windows over TIMESTAMP_LTZ (shift time zones) run on the reference operator (tz_n must be 0)')},
 'two_phase': {'static': (-1, 'session windows are one-phase (agg_phase must be FW_PHASE_ONE)'),
               'dynamic': (-1, 'session windows are one-phase (agg_phase must be FW_PHASE_ONE)'),
               'late': (-1, 'session windows are one-phase (agg_phase must be FW_PHASE_ONE)'),
               'dynamic_late': (-1, 'session windows are one-phase (agg_phase must be FW_PHASE_ONE)'),
               'sql': (-1, 'SQL session windows are one-phase (agg_phase must be FW_PHASE_ONE)')},
 'keyrow_key': {'static': (-1, 'session windows take LONG, INT or PRECOMPUTED keys (key_hash 5: KEYROW / BINROW keys are not supported)'),
                'dynamic': (-1, 'session windows take LONG, INT or PRECOMPUTED keys (key_hash 5: KEYROW / BINROW keys are not supported)'),
                'late': (-1, 'session windows take LONG, INT or PRECOMPUTED keys (key_hash 5: KEYROW / BINROW keys are not supported)'),
                'dynamic_late': (-1, 'session windows take LONG, INT or PRECOMPUTED keys (key_hash 5: KEYROW / BINROW keys are not supported)'),
                'sql': (-1, 'SQL session windows: key rows (FW_KEYHASH_KEYROW) run on the reference operator')},
 'max_batch_rows_0': {'static': (-1, 'max_batch_rows must be in (0, 2^31)'),
                      'dynamic': (-1, 'max_batch_rows must be in (0, 2^31)'),
                      'late': (-1, 'max_batch_rows must be in (0, 2^31)'),
                      'dynamic_late': (-1, 'max_batch_rows must be in (0, 2^31)'),
                      'sql': (-1, 'max_batch_rows must be in (0, 2^31)')},
 'output_capacity_0': {'static': (-1, 'output_capacity must be > 0'),
                       'dynamic': (-1, 'output_capacity must be > 0'),
                       'late': (-1, 'output_capacity must be > 0'),
                       'dynamic_late': (-1, 'output_capacity must be > 0'),
                       'sql': (-1, 'output_capacity must be > 0')},
 'one_value_col': {'static': (0, ''),
                   'dynamic': (-1, 'dynamic-gap session windows take two value columns, the aggregated field and the gap (n_value_cols == 2), got 1'),
                   'late': (0, ''),
                   'dynamic_late': (-1,
                                    'dynamic-gap session windows take two value columns, the aggregated field and the gap (n_value_cols == 2), got '
                                    '1'),
                   'sql': (0, '')},
 'gap_col_not_i64': {'static': (0, ''),
                     'dynamic': (-1, 'dynamic-gap session windows: the gap column (value column 1) must be FW_T_I64'),
                     'late': (0, ''),
                     'dynamic_late': (-1, 'dynamic-gap session windows: the gap column (value column 1) must be FW_T_I64'),
                     'sql': (0, '')},
 'input_col_1': {'static': (0, ''),
                 'dynamic': (-1, 'dynamic-gap session windows: the aggregate reads value column 0 (input_col 1: column 1 is the gap)'),
                 'late': (0, ''),
                 'dynamic_late': (-1, 'dynamic-gap session windows: the aggregate reads value column 0 (input_col 1: column 1 is the gap)'),
                 'sql': (0, '')},
 'wrong_api_and_lateness_big': {'static': (-1,
                                           'FW_KEYHASH_LONG / FW_KEYHASH_INT are DataStream key hashes; a SQL session takes BINROW_BIGINT / '
                                           'BINROW_INT / PRECOMPUTED keys'),
                                'dynamic': (-1, 'FW_WIN_SESSION (EventTimeSessionWindows) is a DataStream window: api must be FW_API_DATASTREAM'),
                                'late': (-1,
                                         'FW_WIN_SESSION_LATENESS (EventTimeSessionWindows with allowedLateness) is a DataStream window: api must be '
                                         'FW_API_DATASTREAM'),
                                'dynamic_late': (-1,
                                                 'FW_WIN_SESSION (EventTimeSessionWindows) is a DataStream window: api must be FW_API_DATASTREAM'),
                                'sql': (-1, 'fw_host_sql_session_words needs a FW_WIN_SESSION configuration with api FW_API_SQL')},
 'lateness_big_and_slide': {'static': (-1, 'session windows have no slide (slide_ms must be 0)'),
                            'dynamic': (-1, 'session windows have no slide (slide_ms must be 0)'),
                            'late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                            'dynamic_late': (-1, 'session windows have no slide (slide_ms must be 0)'),
                            'sql': (-1, 'session windows have no slide (slide_ms must be 0)')},
 'lateness_big_and_one_value_col': {'static': (-1,
                                               'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)'),
                                    'dynamic': (-1,
                                                'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be '
                                                '0)'),
                                    'late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                                    'dynamic_late': (-1,
                                                     'dynamic-gap session windows take two value columns, the aggregated field and the gap '
                                                     '(n_value_cols == 2), got 1'),
                                    'sql': (-1, 'SQL session windows have no allowed lateness (allowed_lateness_ms must be 0)')},
 'lateness_neg_and_output_capacity_0': {'static': (-1,
                                                   'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be '
                                                   '0)'),
                                        'dynamic': (-1,
                                                    'session windows with allowed lateness run on the reference operator (allowed_lateness_ms must '
                                                    'be 0)'),
                                        'late': (-1, 'session windows: allowed_lateness_ms must be in [0, 2^40]'),
                                        'dynamic_late': (-1, 'output_capacity must be > 0'),
                                        'sql': (-1, 'SQL session windows have no allowed lateness (allowed_lateness_ms must be 0)')},
 'n_aggs_2_and_gap_0': {'static': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
                        'dynamic': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
                        'late': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
                        'dynamic_late': (-1, 'session windows take one aggregation (n_aggs == 1), got 2'),
                        'sql': (-1, 'session gap (size_ms) must be > 0')},
 'gap_col_not_i64_and_input_col_1': {'static': (0, ''),
                                     'dynamic': (-1,
                                                 'dynamic-gap session windows: the aggregate reads value column 0 (input_col 1: column 1 is the '
                                                 'gap)'),
                                     'late': (0, ''),
                                     'dynamic_late': (-1,
                                                      'dynamic-gap session windows: the aggregate reads value column 0 (input_col 1: column 1 is the '
                                                      'gap)'),
                                     'sql': (0, '')}}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(BROKEN))
def test_plan_refusal(case, kind):
    assert plan_case(kind, case) == PLAN_EXPECTED[case][kind]


# ---- the four wrappers' own checks: the window kind they accept, null arguments, the caller's gap and
# the session count, in that order
WRAPPERS = ("fw_host_session_add", "fw_host_session_add_late", "fw_host_session_add_gap", "fw_host_session_add_gap_late")
CONFIGS = ("static", "dynamic", "late", "dynamic_late", "sql", "tumble")
ARGUMENTS = {
    "good": {},
    "null_cfg": {"cfg": None},
    "null_n": {"n": None},
    "null_outcome": {"outcome": None},
    "null_fired_index": {"fired_index": None},
    "null_starts": {"starts": None},
    "null_ends_and_accs": {"ends": None, "accs": None},
    "null_lists_capacity_0": {"starts": None, "ends": None, "accs": None, "capacity": 0},
    "gap_0": {"gap": 0},
    "gap_above_size_ms": {"gap": 101},
    "count_negative": {"count": -1},
    "count_above_capacity": {"count": 5},
    "gap_0_and_count_negative": {"gap": 0, "count": -1},
    "null_n_and_wrong_gap": {"n": None, "gap": 0},
}


def call_wrapper(name, config, *, cfg=True, n=True, outcome=True, fired_index=True, starts=True, ends=True, accs=True, capacity=4,
                 gap=1, count=0):
    L = _native.lib()
    c = abi.make_config(window_kind=abi.WIN_TUMBLE, size_ms=100, aggs=[(abi.AGG_SUM, 0, abi.T_I64)],
                        value_col_types=[abi.T_I64]) if config == "tumble" else good_config(config)
    lists = [(C.c_int64 * 4)() if given else None for given in (starts, ends, accs)]
    nn, out, at = C.c_int32(count), C.c_int32(-7), C.c_int32(-7)
    args = [C.byref(c) if cfg else None, 0, 0]
    if "gap" in name:
        args.append(gap)
    args += [1, *lists, C.byref(nn) if n else None, capacity, C.byref(out) if outcome else None]
    if "late" in name:
        args.append(C.byref(at) if fired_index else None)
    rc = getattr(L, name)(*args)
    return rc, (_last_error() if rc else "")


OWN_CONFIG = dict(zip(WRAPPERS, ("static", "late", "dynamic", "dynamic_late")))

# KIND_EXPECTED[wrapper][config] = (return code, message): good arguments, every kind of configuration
KIND_EXPECTED = {'fw_host_session_add': {'static': (0, ''),
                         'dynamic': (-1, 'fw_host_session_add needs a FW_WIN_SESSION configuration'),
                         'late': (-1, 'fw_host_session_add needs a FW_WIN_SESSION configuration'),
                         'dynamic_late': (-1, 'fw_host_session_add needs a FW_WIN_SESSION configuration'),
                         'sql': (-1, 'fw_host_session_add needs a DataStream session configuration (SQL: fw_host_sql_session_add)'),
                         'tumble': (-1, 'fw_host_session_add needs a FW_WIN_SESSION configuration')},
 'fw_host_session_add_late': {'static': (-1, 'fw_host_session_add_late needs a FW_WIN_SESSION_LATENESS configuration'),
                              'dynamic': (-1, 'fw_host_session_add_late needs a FW_WIN_SESSION_LATENESS configuration'),
                              'late': (0, ''),
                              'dynamic_late': (-1, 'fw_host_session_add_late needs a FW_WIN_SESSION_LATENESS configuration'),
                              'sql': (-1, 'fw_host_session_add_late needs a FW_WIN_SESSION_LATENESS configuration'),
                              'tumble': (-1, 'fw_host_session_add_late needs a FW_WIN_SESSION_LATENESS configuration')},
 'fw_host_session_add_gap': {'static': (-1, 'fw_host_session_add_gap needs a FW_WIN_SESSION_DYNAMIC configuration'),
                             'dynamic': (0, ''),
                             'late': (-1, 'fw_host_session_add_gap needs a FW_WIN_SESSION_DYNAMIC configuration'),
                             'dynamic_late': (-1, 'fw_host_session_add_gap needs a FW_WIN_SESSION_DYNAMIC configuration'),
                             'sql': (-1, 'fw_host_session_add_gap needs a FW_WIN_SESSION_DYNAMIC configuration'),
                             'tumble': (-1, 'fw_host_session_add_gap needs a FW_WIN_SESSION_DYNAMIC configuration')},
 'fw_host_session_add_gap_late': {'static': (-1, 'fw_host_session_add_gap_late needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration'),
                                  'dynamic': (-1, 'fw_host_session_add_gap_late needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration'),
                                  'late': (-1, 'fw_host_session_add_gap_late needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration'),
                                  'dynamic_late': (0, ''),
                                  'sql': (-1, 'fw_host_session_add_gap_late needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration'),
                                  'tumble': (-1, 'fw_host_session_add_gap_late needs a FW_WIN_SESSION_DYNAMIC_LATENESS configuration')}}
# ARGUMENT_EXPECTED[arguments][wrapper] = (return code, message): the wrapper's own kind of configuration
ARGUMENT_EXPECTED = {'good': {'fw_host_session_add': (0, ''),
          'fw_host_session_add_late': (0, ''),
          'fw_host_session_add_gap': (0, ''),
          'fw_host_session_add_gap_late': (0, '')},
 'null_cfg': {'fw_host_session_add': (-1, 'null argument'),
              'fw_host_session_add_late': (-1, 'null argument'),
              'fw_host_session_add_gap': (-1, 'null argument'),
              'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_n': {'fw_host_session_add': (-1, 'null argument'),
            'fw_host_session_add_late': (-1, 'null argument'),
            'fw_host_session_add_gap': (-1, 'null argument'),
            'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_outcome': {'fw_host_session_add': (-1, 'null argument'),
                  'fw_host_session_add_late': (-1, 'null argument'),
                  'fw_host_session_add_gap': (-1, 'null argument'),
                  'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_fired_index': {'fw_host_session_add': (0, ''),
                      'fw_host_session_add_late': (-1, 'null argument'),
                      'fw_host_session_add_gap': (0, ''),
                      'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_starts': {'fw_host_session_add': (-1, 'null argument'),
                 'fw_host_session_add_late': (-1, 'null argument'),
                 'fw_host_session_add_gap': (-1, 'null argument'),
                 'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_ends_and_accs': {'fw_host_session_add': (-1, 'null argument'),
                        'fw_host_session_add_late': (-1, 'null argument'),
                        'fw_host_session_add_gap': (-1, 'null argument'),
                        'fw_host_session_add_gap_late': (-1, 'null argument')},
 'null_lists_capacity_0': {'fw_host_session_add': (-3, 'the session list is full (0 sessions)'),
                           'fw_host_session_add_late': (-3, 'the session list is full (0 sessions)'),
                           'fw_host_session_add_gap': (0, ''),
                           'fw_host_session_add_gap_late': (-3, 'the session list is full (0 sessions)')},
 'gap_0': {'fw_host_session_add': (0, ''),
           'fw_host_session_add_late': (0, ''),
           'fw_host_session_add_gap': (-1, 'session gap 0 is outside (0, size_ms = 100]'),
           'fw_host_session_add_gap_late': (-1, 'session gap 0 is outside (0, size_ms = 100]')},
 'gap_above_size_ms': {'fw_host_session_add': (0, ''),
                       'fw_host_session_add_late': (0, ''),
                       'fw_host_session_add_gap': (-1, 'session gap 101 is outside (0, size_ms = 100]'),
                       'fw_host_session_add_gap_late': (-1, 'session gap 101 is outside (0, size_ms = 100]')},
 'count_negative': {'fw_host_session_add': (-1, 'bad session count -1 (capacity 4)'),
                    'fw_host_session_add_late': (-1, 'bad session count -1 (capacity 4)'),
                    'fw_host_session_add_gap': (-1, 'bad session count -1 (capacity 4)'),
                    'fw_host_session_add_gap_late': (-1, 'bad session count -1 (capacity 4)')},
 'count_above_capacity': {'fw_host_session_add': (-1, 'bad session count 5 (capacity 4)'),
                          'fw_host_session_add_late': (-1, 'bad session count 5 (capacity 4)'),
                          'fw_host_session_add_gap': (-1, 'bad session count 5 (capacity 4)'),
                          'fw_host_session_add_gap_late': (-1, 'bad session count 5 (capacity 4)')},
 'gap_0_and_count_negative': {'fw_host_session_add': (-1, 'bad session count -1 (capacity 4)'),
                              'fw_host_session_add_late': (-1, 'bad session count -1 (capacity 4)'),
                              'fw_host_session_add_gap': (-1, 'session gap 0 is outside (0, size_ms = 100]'),
                              'fw_host_session_add_gap_late': (-1, 'session gap 0 is outside (0, size_ms = 100]')},
 'null_n_and_wrong_gap': {'fw_host_session_add': (-1, 'null argument'),
                          'fw_host_session_add_late': (-1, 'null argument'),
                          'fw_host_session_add_gap': (-1, 'null argument'),
                          'fw_host_session_add_gap_late': (-1, 'null argument')}}


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_window_kind(name, config):
    assert call_wrapper(name, config) == KIND_EXPECTED[name][config]


@pytest.mark.parametrize("name", WRAPPERS)
@pytest.mark.parametrize("arguments", list(ARGUMENTS))
def test_wrapper_arguments(arguments, name):
    assert call_wrapper(name, OWN_CONFIG[name], **ARGUMENTS[arguments]) == ARGUMENT_EXPECTED[arguments][name]
