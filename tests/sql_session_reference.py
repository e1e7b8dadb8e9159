"""Pure-Python restatement of the SQL SESSION window TVF aggregate

    SELECT k, <aggs> FROM TABLE(SESSION(TABLE t PARTITION BY k, DESCRIPTOR(rowtime), gap))
    GROUP BY k, window_start, window_end

for event time, a static gap and a TIMESTAMP rowtime: the checker of the SQL session tests.

RECALLED, PARITY UNPINNED.  The Flink sources were not at hand; the rules below are recalled from
UnsliceWindowAggProcessor, UnsliceAssigners.SessionUnsliceAssigner, the table runtime's
MergingWindowProcessFunction.assignActualWindows / MergingFunctionImpl.merge and
WindowAggOperator.processWatermark, and from the built-in aggregate functions' accumulate / merge /
getValue expressions.  Parity with Flink rests on this restatement.

Element by element, per key a plain list of [start, end, accs]:
  1. a row with rowtime ts gets the window [ts, ts + gap); it is merged with every window of its key
     it intersects (TimeWindow.intersects is inclusive: touching windows merge); the merged
     accumulator is the aggregates' merge of the members' accumulators, then the row is accumulated;
  2. if the merged window is late (end - 1 <= currentWatermark) the row is dropped, counted in
     numLateRecordsDropped, and the window set is left as it was (rule 4 of
     session_window_reference.py, order dependence included);
  3. a watermark W' > W fires every session with end - 1 <= W' once, as
     key ++ aggs ++ (window_start, window_end), and clears it;
  4. a row whose value is NULL (None) still opens or extends its session; only its aggregates skip it;
  5. results: COUNT(*) counts rows, COUNT(col) non-NULL rows (0, never NULL); SUM / MIN / MAX are
     NULL (None) without a non-NULL input; SUM(INT) wraps at 32 bits, SUM(BIGINT) at 64; AVG is NULL
     on a zero count, Java's truncating division for BIGINT / INT (an INT result for INT, over a
     BIGINT sum), IEEE division for DOUBLE.
Aggregates are (kind, input column, type) with kind in COUNT_STAR / COUNT / SUM / MIN / MAX / AVG and
type in BIGINT / INT / DOUBLE; DOUBLE values are Python floats.  This module is not vectorised and
shares no code with flink_amd; it borrows the integer wrap and the interval test of
session_window_reference.py.
"""
from session_window_reference import LONG_MIN, _intersects, _wrap

KINDS = ("COUNT_STAR", "COUNT", "SUM", "MIN", "MAX", "AVG")


def _java_div(a, b):
    """Java long division: truncation toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _sum_add(typ, a, b):
    if typ == "DOUBLE":
        return a + b
    return _wrap(a + b, 32 if typ == "INT" else 64)


class _Agg:
    """one aggregate's accumulator functions: create / accumulate / merge / value"""

    def __init__(self, kind, col, typ):
        if kind not in KINDS:
            raise ValueError(kind)
        self.kind, self.col, self.typ = kind, col, typ

    def create(self):
        if self.kind in ("COUNT_STAR", "COUNT"):
            return 0
        if self.kind == "AVG":
            return [0.0 if self.typ == "DOUBLE" else 0, 0]      # (sum, count); the sum of AVG(INT) is a BIGINT
        return None                                             # SUM / MIN / MAX: NULL until a non-NULL input

    def accumulate(self, acc, row):
        if self.kind == "COUNT_STAR":
            return acc + 1
        v = row[self.col]
        if v is None:
            return acc
        if self.kind == "COUNT":
            return acc + 1
        if self.kind == "SUM":
            return v if acc is None else _sum_add(self.typ, acc, v)
        if self.kind == "MIN":
            return v if acc is None or v < acc else acc
        if self.kind == "MAX":
            return v if acc is None or v > acc else acc
        return [_sum_add("DOUBLE" if self.typ == "DOUBLE" else "BIGINT", acc[0], v), acc[1] + 1]

    def merge(self, a, b):
        if self.kind in ("COUNT_STAR", "COUNT"):
            return a + b
        if self.kind == "AVG":
            return [_sum_add("DOUBLE" if self.typ == "DOUBLE" else "BIGINT", a[0], b[0]), a[1] + b[1]]
        if a is None or b is None:
            return b if a is None else a
        if self.kind == "SUM":
            return _sum_add(self.typ, a, b)
        if self.kind == "MIN":
            return b if b < a else a
        return b if b > a else a

    def value(self, acc):
        if self.kind != "AVG":
            return acc
        s, c = acc
        if c == 0:
            return None
        if self.typ == "DOUBLE":
            return s / c
        q = _java_div(s, c)
        return _wrap(q, 32) if self.typ == "INT" else q


class SqlSessionReference:
    """``aggs``: (kind, input column, type) triples.  process(keys, rowtimes, rows) applies the rows
    in order (``rows[i]`` the value columns of row i, None for NULL) and returns the indices of the
    rows dropped as late; process_watermark(w) returns the fired rows
    (key, *agg values, window_start, window_end) sorted by (end - 1, key, start)."""

    def __init__(self, gap, aggs):
        if gap <= 0:
            raise ValueError("gap must be > 0")
        self.gap = gap
        self.aggs = [_Agg(*a) for a in aggs]
        self.windows = {}   # key -> list of [start, end, accs]
        self.watermark = LONG_MIN
        self.late_dropped = 0
        self.fired = 0

    def add(self, key, ts, row):
        """one row; True if it was kept"""
        new = [ts, ts + self.gap, None]
        lst = self.windows.get(key, [])
        cover, members = [new[0], new[1]], [new]
        changed = True
        while changed:                                       # every window the growing cover intersects
            changed = False
            for w in lst:
                if not any(m is w for m in members) and _intersects(cover, w):
                    cover = [min(cover[0], w[0]), max(cover[1], w[1])]
                    members.append(w)
                    changed = True
        if cover[1] - 1 <= self.watermark:                   # the merged window is late
            assert len(members) == 1
            self.late_dropped += 1
            return False
        accs = None
        for m in sorted(members[1:], key=lambda w: w[0]):    # merge of the members' accumulators
            accs = list(m[2]) if accs is None else [a.merge(x, y) for a, x, y in zip(self.aggs, accs, m[2])]
        if accs is None:
            accs = [a.create() for a in self.aggs]
        accs = [a.accumulate(x, row) for a, x in zip(self.aggs, accs)]
        kept = [w for w in lst if not any(m is w for m in members)]
        kept.append([cover[0], cover[1], accs])
        kept.sort(key=lambda w: w[0])
        self.windows[key] = kept
        return True

    def process(self, keys, rowtimes, rows):
        late = []
        for i, (k, ts, row) in enumerate(zip(keys, rowtimes, rows)):
            if not self.add(int(k), int(ts), row):
                late.append(i)
        return late

    def process_watermark(self, watermark):
        if watermark <= self.watermark:
            return []
        self.watermark = watermark
        out = []
        for k in list(self.windows):
            keep = []
            for s, e, accs in self.windows[k]:
                if e - 1 <= watermark:
                    out.append((k, *[a.value(x) for a, x in zip(self.aggs, accs)], s, e))
                else:
                    keep.append([s, e, accs])
            if keep:
                self.windows[k] = keep
            else:
                del self.windows[k]
        out.sort(key=lambda r: (r[-1] - 1, r[0], r[-2]))
        self.fired += len(out)
        return out

    def live_sessions(self):
        return sum(len(v) for v in self.windows.values())

    def snapshot(self):
        return ({k: [[w[0], w[1], [list(x) if isinstance(x, list) else x for x in w[2]]] for w in v]
                 for k, v in self.windows.items()}, self.watermark, self.late_dropped, self.fired)

    def restore(self, snap):
        self.windows = {k: [[w[0], w[1], [list(x) if isinstance(x, list) else x for x in w[2]]] for w in v]
                        for k, v in snap[0].items()}
        self.watermark, self.late_dropped, self.fired = snap[1], snap[2], snap[3]
