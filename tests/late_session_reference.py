"""Pure-Python restatement of keyBy(...).window(EventTimeSessionWindows.withGap(g)).allowedLateness(L)
with the default EventTimeTrigger and no evictor: the checker of the late-session tests.

Written from what is recalled of WindowOperator.processElement (merging branch),
MergingWindowSet.addWindow, TimeWindow.intersects / cover, EventTimeTrigger.onElement / onEventTime
and WindowOperator.cleanupTime; the reference Java was not at hand, so parity rests on this
restatement and the worked case of the tests.  Gap g, lateness L, watermark W, element by element,
per key a plain list of [start, end, acc]:
  1. the element's window is [ts, ts + g); it merges with every session of its key it intersects
     (a.start <= b.end and a.end >= b.start: touching counts); the merged session is the cover, its
     accumulator the fold of theirs, then the element's value;
  2. an element that intersects nothing and has ts + g - 1 + L <= W is dropped, the state untouched
     (a merge result is never late: every held session has end - 1 + L > W);
  3. otherwise it is kept, and if the resulting session has end - 1 <= W it is emitted at once with
     the accumulator after this element (EventTimeTrigger.onElement: FIRE); nothing is purged;
  4. an advance from W to W' > W emits every session with W < end - 1 <= W' and removes every session
     with end - 1 + L <= W' (emitted in this advance or earlier);
  5. a session held with end - 1 <= W has been emitted with exactly its contents: the watermark says
     which sessions have fired;
  6. an element with ts + g - 1 > W may merge with a fired session; the result is unfired.
This module is not vectorised and shares no code with flink_amd.
"""
import struct

LONG_MIN = -(1 << 63)
CLASSES = ("dropped", "fired_at_once", "fired_at_once_new", "candidate_into_unfired", "ontime_into_fired", "cleaned_silent")


def _wrap(v, bits):
    m = 1 << bits
    v &= m - 1
    return v - m if v >= m >> 1 else v


def _b2d(b):
    return struct.unpack("<d", struct.pack("<q", _wrap(int(b), 64)))[0]


def _d2b(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _dcmp(a, b):
    """Double.compare on bit patterns: numeric order, then -0.0 < 0.0 < NaN, all NaNs equal"""
    x, y = _b2d(a), _b2d(b)
    if x < y:
        return -1
    if x > y:
        return 1
    ca = 0x7FF8000000000000 if x != x else _wrap(int(a), 64)
    cb = 0x7FF8000000000000 if y != y else _wrap(int(b), 64)
    return (ca > cb) - (ca < cb)


def _fold(fn, ftype, a, b):
    if fn == "count":
        return a + b
    if fn == "sum":
        if ftype == "DOUBLE":
            return _d2b(_b2d(a) + _b2d(b))
        return _wrap(a + b, 32 if ftype == "INT" else 64)
    c = _dcmp(a, b) if ftype == "DOUBLE" else (a > b) - (a < b)
    if fn == "max":
        return a if c > 0 else b
    if fn == "min":
        return a if c < 0 else b
    raise ValueError(fn)


class LateSessionReference:
    """``aggregation`` = (fn, ftype); DOUBLE values travel as bit patterns.  process(keys, timestamps,
    values) applies the elements in order and returns (indices dropped, rows fired at once in arrival
    order); process_watermark(w) returns the timer rows sorted by (end - 1, key, start).  Rows are
    (key, value, window_start, window_end).  ``counts`` has one counter per class of CLASSES."""

    def __init__(self, gap, lateness, aggregation=("sum", "LONG")):
        if gap <= 0 or lateness < 0:
            raise ValueError("gap must be > 0 and lateness >= 0")
        self.gap, self.lateness = gap, lateness
        self.fn, self.ftype = aggregation[:2]
        self.windows = {}   # key -> [[start, end, acc]] sorted by start
        self.watermark = LONG_MIN
        self.late_dropped = 0
        self.fired = 0      # every emitted row
        self.counts = dict.fromkeys(CLASSES, 0)
        self.max_live = 0

    def add(self, key, ts, value):
        """one element: (kept, the row it fired at once or None)"""
        W, g = self.watermark, self.gap
        v = 1 if self.fn == "count" else int(value)
        s, e = ts, ts + g
        lst = self.windows.get(key, [])
        hit = [w for w in lst if s <= w[1] and e >= w[0]]
        candidate = ts + g - 1 <= W
        if not hit and ts + g - 1 + self.lateness <= W:
            self.late_dropped += 1
            self.counts["dropped"] += 1
            return False, None
        acc = None
        for w in hit:   # by start: the list is sorted
            s, e = min(s, w[0]), max(e, w[1])
            acc = w[2] if acc is None else _fold(self.fn, self.ftype, acc, w[2])
        acc = v if acc is None else _fold(self.fn, self.ftype, acc, v)
        kept = [w for w in lst if not any(h is w for h in hit)] + [[s, e, acc]]
        kept.sort(key=lambda w: w[0])
        self.windows[key] = kept
        self.max_live = max(self.max_live, self.live_sessions())
        row = None
        if e - 1 <= W:
            row = (key, acc, s, e)
            self.fired += 1
            self.counts["fired_at_once"] += 1
            if not hit:
                self.counts["fired_at_once_new"] += 1
        elif candidate and hit:
            self.counts["candidate_into_unfired"] += 1
        if not candidate and any(w[1] - 1 <= W for w in hit):
            self.counts["ontime_into_fired"] += 1
        return True, row

    def process(self, keys, timestamps, values):
        late, rows = [], []
        for i, (k, ts, v) in enumerate(zip(keys, timestamps, values)):
            kept, row = self.add(k, int(ts), v)
            if not kept:
                late.append(i)
            if row is not None:
                rows.append(row)
        return late, rows

    def process_watermark(self, watermark):
        if watermark <= self.watermark:
            return []
        W0, self.watermark = self.watermark, watermark
        out = []
        for k in list(self.windows):
            keep = []
            for s, e, acc in self.windows[k]:
                fires = W0 < e - 1 <= watermark
                if fires:
                    out.append((k, acc, s, e))
                if e - 1 + self.lateness <= watermark:
                    if not fires:
                        self.counts["cleaned_silent"] += 1
                else:
                    keep.append([s, e, acc])
            if keep:
                self.windows[k] = keep
            else:
                del self.windows[k]
        self.fired += len(out)
        out.sort(key=lambda r: (r[3] - 1, r[0], r[2]))
        return out

    def live_sessions(self):
        return sum(len(v) for v in self.windows.values())

    def sessions(self):
        return sorted((k, s, e, a) for k, v in self.windows.items() for s, e, a in v)
