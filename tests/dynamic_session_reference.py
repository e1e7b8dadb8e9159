"""Pure-Python restatement of keyBy(...).window(EventTimeSessionWindows.withDynamicGap(extractor))
with the default EventTimeTrigger, no evictor and allowedLateness = 0: the checker of the dynamic-gap
session-window tests.

Written from DynamicEventTimeSessionWindows.assignWindows and, for everything behind the assignment,
the same sources as session_window_reference.py (WindowOperator.processElement's merging branch,
MergingWindowSet.addWindow, TimeWindow.intersects / mergeWindows, EventTimeTrigger); the reference
Java was not at hand, so parity rests on this restatement.

Element by element, per key a plain list of [start, end, acc]:
  1. g = extractor.extract(element); g <= 0 throws IllegalArgumentException("Dynamic session time gap
     must satisfy 0 < gap") -- here ValueError with that message; the element's window is [ts, ts + g);
  2. TimeWindow.mergeWindows: all windows of the key plus the new one are sorted by start and swept; a
     window that intersects the running one (touching counts) is covered into it;
  3. the group that holds the new window becomes one window whose state is the reduce of the merged
     windows' states, then the element's value is folded in;
  4. if that window is late (end - 1 <= watermark) the element is dropped and the state is left as it
     was -- with lateness 0 this can only be the element alone;
  5. a watermark W' > W fires every window with end - 1 <= W' and clears it.
The class also counts what a stream exercised (``seen``), for the tests' coverage assertions.
This module is not vectorised and shares no code with flink_amd.
"""
from session_window_reference import LONG_MIN, _reduce

GAP_MESSAGE = "Dynamic session time gap must satisfy 0 < gap"


def _intersects(a, b):
    return a[0] <= b[1] and a[1] >= b[0]


class DynamicSessionReference:
    """``aggregation`` = (fn, ftype).  add(key, ts, value, gap) applies one element and returns True
    if it was kept; process(keys, timestamps, values, gaps) applies the elements in order and returns
    the indices of the dropped ones; process_watermark(w) returns the fired rows (key, value,
    window_start, window_end) sorted by (end - 1, key, start)."""

    def __init__(self, aggregation=("sum", "LONG")):
        self.fn, self.ftype = aggregation[:2]
        self.windows = {}   # key -> list of [start, end, acc]
        self.watermark = LONG_MIN
        self.late_dropped = 0
        # nested: the element's window lies inside a session that started before it and ends after it
        # touch: merged with a session it only touches; bridge3: the merged group held >= 3 sessions
        self.seen = {"nested": 0, "touch": 0, "bridge3": 0, "late_drop": 0, "late_kept": 0}

    def add(self, key, ts, value, gap):
        if gap <= 0:
            raise ValueError(GAP_MESSAGE)
        v = 1 if self.fn == "count" else int(value)
        new = [ts, ts + gap, None]
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
        late_candidate = new[1] - 1 <= self.watermark
        if cover[1] - 1 <= self.watermark:                   # isWindowLate(actualWindow)
            assert len(members) == 1 and members[0] is new
            self.late_dropped += 1
            self.seen["late_drop"] += 1
            return False
        old = [m for m in members if m is not new]
        self.seen["late_kept"] += late_candidate
        self.seen["nested"] += any(m[0] < new[0] and m[1] > new[1] for m in old)
        self.seen["touch"] += any(m[1] == new[0] or m[0] == new[1] for m in old)
        self.seen["bridge3"] += len(old) >= 3
        acc = None
        for m in old:                                        # mergeNamespaces, then windowState.add
            acc = m[2] if acc is None else _reduce(self.fn, self.ftype, acc, m[2])
        acc = v if acc is None else _reduce(self.fn, self.ftype, acc, v)
        kept = [w for w in lst if not any(m is w for m in members)]
        kept.append([cover[0], cover[1], acc])
        kept.sort(key=lambda w: w[0])
        self.windows[key] = kept
        return True

    def process(self, keys, timestamps, values, gaps):
        late = []
        for i, (k, ts, v, g) in enumerate(zip(keys, timestamps, values, gaps)):
            if not self.add(k, int(ts), v, int(g)):
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
