"""Pure-Python restatement of keyBy(...).window(EventTimeSessionWindows.withGap(gap)) with the default
EventTimeTrigger, no evictor and allowedLateness = 0: the checker of the session-window tests.

Written from WindowOperator.processElement (merging branch), MergingWindowSet.addWindow,
TimeWindow.intersects / mergeWindows, EventTimeSessionWindows and EventTimeTrigger; the reference
Java was not at hand, so parity rests on this restatement and the transcribed testSessionWindows case.

Element by element, per key a plain list of (start, end, acc):
  1. the element's window is [ts, ts + gap);
  2. TimeWindow.mergeWindows: all windows of the key plus the new one are sorted by start and swept;
     a window that intersects the running one (a.start <= b.end and a.end >= b.start: touching
     counts) is covered into it;
  3. the group that holds the new window becomes one window whose state is the reduce of the merged
     windows' states, then the element's value is folded in;
  4. if that window is late (end - 1 <= watermark) the element is dropped and the state is left as
     it was -- with lateness 0 this can only be the element alone, every kept window has
     end - 1 > watermark;
  5. a watermark W' > W fires every window with end - 1 <= W' (its timer's timestamp) and clears it.
This module is not vectorised and shares no code with flink_amd.
"""
import struct

LONG_MIN = -(1 << 63)


def _wrap(v, bits):
    m = 1 << bits
    v &= m - 1
    return v - m if v >= m >> 1 else v


def _bits_to_double(b):
    return struct.unpack("<d", struct.pack("<q", _wrap(int(b), 64)))[0]


def _double_to_bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _double_compare(a, b):
    """Double.compare on bit patterns: numeric order, then -0.0 < 0.0 < NaN with all NaNs equal"""
    x, y = _bits_to_double(a), _bits_to_double(b)
    if x < y:
        return -1
    if x > y:
        return 1

    def canon(v, bits):
        return 0x7FF8000000000000 if v != v else _wrap(int(bits), 64)
    ca, cb = canon(x, a), canon(y, b)
    return 0 if ca == cb else (-1 if ca < cb else 1)


def _reduce(fn, ftype, a, b):
    """reduce(value1 = a, value2 = b) on the aggregated field; DOUBLE fields travel as bits"""
    if fn == "count":
        return a + b
    if fn == "sum":
        if ftype == "DOUBLE":
            return _double_to_bits(_bits_to_double(a) + _bits_to_double(b))
        return _wrap(a + b, 32 if ftype == "INT" else 64)
    cmp = _double_compare(a, b) if ftype == "DOUBLE" else (a > b) - (a < b)
    if fn == "max":
        return a if cmp > 0 else b
    if fn == "min":
        return a if cmp < 0 else b
    raise ValueError(fn)


def _intersects(a, b):
    return a[0] <= b[1] and a[1] >= b[0]


class SessionWindowReference:
    """``aggregation`` = (fn, ftype).  process(keys, timestamps, values) applies the elements in order
    and returns the indices (in that call) of the elements dropped as late; process_watermark(w)
    returns the fired rows (key, value, window_start, window_end) sorted by (end - 1, key, start)."""

    def __init__(self, gap, aggregation=("sum", "LONG")):
        if gap <= 0:
            raise ValueError("gap must be > 0")
        self.gap = gap
        self.fn, self.ftype = aggregation[:2]
        self.windows = {}   # key -> list of [start, end, acc]
        self.watermark = LONG_MIN
        self.late_dropped = 0

    def add(self, key, ts, value):
        """one element; True if it was kept"""
        v = 1 if self.fn == "count" else int(value)
        new = [ts, ts + self.gap, None]
        lst = self.windows.get(key, [])
        swept = sorted(lst + [new], key=lambda w: w[0])     # TimeWindow.mergeWindows
        groups, cur, members = [], None, []
        for w in swept:
            if cur is None:
                cur, members = [w[0], w[1]], [w]
            elif _intersects(cur, w):
                cur = [min(cur[0], w[0]), max(cur[1], w[1])]
                members.append(w)
            else:
                groups.append((cur, members))
                cur, members = [w[0], w[1]], [w]
        groups.append((cur, members))
        for cover, members in groups:
            if any(m is new for m in members):
                break
        if cover[1] - 1 <= self.watermark:                   # isWindowLate(actualWindow)
            assert len(members) == 1 and members[0] is new
            self.late_dropped += 1
            return False
        acc = None
        for m in members:                                    # mergeNamespaces, then windowState.add
            if m is not new:
                acc = m[2] if acc is None else _reduce(self.fn, self.ftype, acc, m[2])
        acc = v if acc is None else _reduce(self.fn, self.ftype, acc, v)
        kept = [w for w in lst if not any(m is w for m in members)]
        kept.append([cover[0], cover[1], acc])
        kept.sort(key=lambda w: w[0])
        self.windows[key] = kept
        return True

    def process(self, keys, timestamps, values):
        late = []
        for i, (k, ts, v) in enumerate(zip(keys, timestamps, values)):
            if not self.add(k, int(ts), v):
                late.append(i)
        return late

    def process_watermark(self, watermark):
        if watermark <= self.watermark:
            return []
        self.watermark = watermark
        out = []
        for k in list(self.windows):
            keep = []
            for s, e, acc in self.windows[k]:
                if e - 1 <= watermark:                       # the timer at maxTimestamp fires
                    out.append((k, acc, s, e))
                else:
                    keep.append([s, e, acc])
            if keep:
                self.windows[k] = keep
            else:
                del self.windows[k]
        out.sort(key=lambda r: (r[3] - 1, r[0], r[2]))
        return out

    def live_sessions(self):
        return sum(len(v) for v in self.windows.values())

    def snapshot(self):
        return ({k: [list(w) for w in v] for k, v in self.windows.items()}, self.watermark, self.late_dropped)

    def restore(self, snap):
        self.windows = {k: [list(w) for w in v] for k, v in snap[0].items()}
        self.watermark, self.late_dropped = snap[1], snap[2]
