"""Pure-Python restatement of
keyBy(...).window(EventTimeSessionWindows.withDynamicGap(extractor)).allowedLateness(L) with the
default EventTimeTrigger and no evictor: the checker of the dynamic-gap late-session tests.

Written from what is recalled of DynamicEventTimeSessionWindows.assignWindows,
WindowOperator.processElement (merging branch), MergingWindowSet.addWindow, TimeWindow.intersects /
cover, EventTimeTrigger.onElement / onEventTime and WindowOperator.cleanupTime; the reference Java was
not at hand, so parity rests on this restatement and the worked case of the tests (recalled, parity
unpinned).  The rules are those of late_session_reference.LateSessionReference with the gap an
argument of every element.  Lateness L, watermark W, element by element, per key a plain list of
[start, end, acc]:
  1. the element's window is [ts, ts + g) with its own gap g > 0; it merges with every session of its
     key it intersects (touching counts); the merged session is the cover, its accumulator the fold of
     theirs, then the element's value.  A window may lie wholly inside a held session;
  2. an element that intersects nothing and has ts + g - 1 + L <= W is dropped, the state untouched:
     of two elements with one timestamp the longer gap may stay where the shorter is dropped;
  3. otherwise it is kept, and if the resulting session has end - 1 <= W it is emitted at once with
     the accumulator after this element; nothing is purged;
  4. an advance from W to W' > W emits every session with W < end - 1 <= W' and removes every session
     with end - 1 + L <= W';
  5. a session held with end - 1 <= W has been emitted with exactly its contents;
  6. an element with ts + g - 1 > W may merge with a fired session; the result is unfired.
This module is not vectorised and shares no code with flink_amd; the fold helpers are
late_session_reference's.
"""
from late_session_reference import CLASSES, LONG_MIN, _fold  # noqa: F401

GAP_MESSAGE = "Dynamic session time gap must satisfy 0 < gap"


class DynamicLateSessionReference:
    """``aggregation`` = (fn, ftype); DOUBLE values travel as bit patterns.  add(key, ts, value, gap)
    returns (kept, the row it fired at once or None); process(keys, timestamps, values, gaps) applies
    the elements in order and returns (indices dropped, rows fired at once in arrival order);
    process_watermark(w) returns the timer rows sorted by (end - 1, key, start).  Rows are (key,
    value, window_start, window_end).  ``counts`` has one counter per class of CLASSES;
    ``inside_held`` counts the kept elements whose window lies inside one held session,
    ``own_gap_only`` (given ``max_gap``) the elements that are late candidates by their own gap
    but would not be by the largest."""

    def __init__(self, lateness, aggregation=("sum", "LONG"), max_gap=None):
        if lateness < 0:
            raise ValueError("lateness must be >= 0")
        self.lateness, self.max_gap = lateness, max_gap
        self.fn, self.ftype = aggregation[:2]
        self.windows = {}   # key -> [[start, end, acc]] sorted by start
        self.watermark = LONG_MIN
        self.late_dropped = 0
        self.fired = 0      # every emitted row
        self.counts = dict.fromkeys(CLASSES, 0)
        self.max_live = 0
        self.inside_held = 0
        self.own_gap_only = 0
        self.candidates = 0

    def add(self, key, ts, value, gap):
        if gap <= 0:
            raise ValueError(GAP_MESSAGE)
        W = self.watermark
        v = 1 if self.fn == "count" else int(value)
        s, e = ts, ts + gap
        lst = self.windows.get(key, [])
        hit = [w for w in lst if s <= w[1] and e >= w[0]]
        candidate = ts + gap - 1 <= W
        self.candidates += candidate
        if candidate and self.max_gap is not None and ts + self.max_gap - 1 > W:
            self.own_gap_only += 1
        if not hit and ts + gap - 1 + self.lateness <= W:
            self.late_dropped += 1
            self.counts["dropped"] += 1
            return False, None
        if len(hit) == 1 and hit[0][0] <= s and hit[0][1] >= e:
            self.inside_held += 1
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

    def process(self, keys, timestamps, values, gaps):
        late, rows = [], []
        for i, (k, ts, v, g) in enumerate(zip(keys, timestamps, values, gaps)):
            kept, row = self.add(k, int(ts), v, int(g))
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
