"""Mirrors of the DataStream window assigners and trigger that the GPU operator accepts.

TumblingEventTimeWindows  flink-runtime/.../windowing/assigners/TumblingEventTimeWindows.java:69-87
SlidingEventTimeWindows   flink-runtime/.../windowing/assigners/SlidingEventTimeWindows.java:77-90
EventTimeTrigger          flink-runtime/.../windowing/triggers/EventTimeTrigger.java:37-52
"""
from .._native import lib


class TumblingEventTimeWindows:
    def __init__(self, size, offset=0):
        if abs(offset) >= size or size <= 0:
            raise ValueError("TumblingEventTimeWindows parameters must satisfy abs(offset) < size")
        self.size, self.offset = size, offset

    @staticmethod
    def of(size_ms, offset_ms=0):
        return TumblingEventTimeWindows(size_ms, offset_ms)

    def assign_windows(self, timestamp):
        start = lib().fw_host_window_start(int(timestamp), self.offset % self.size, self.size)
        return [(start, start + self.size)]

    def is_event_time(self):
        return True


class SlidingEventTimeWindows:
    MAX_WINDOW_NUM = 10_000_000  # SlidingEventTimeWindows.java:50

    def __init__(self, size, slide, offset=0):
        if abs(offset) >= slide or size <= 0:
            raise ValueError("SlidingEventTimeWindows parameters must satisfy abs(offset) < slide and size > 0")
        if size // slide > self.MAX_WINDOW_NUM:
            raise ValueError("Number of windows per element exceeds MAX_WINDOW_NUM")
        self.size, self.slide, self.offset = size, slide, offset

    @staticmethod
    def of(size_ms, slide_ms, offset_ms=0):
        return SlidingEventTimeWindows(size_ms, slide_ms, offset_ms)

    def assign_windows(self, timestamp):
        last = lib().fw_host_window_start(int(timestamp), self.offset, self.slide)
        out = []
        s = last
        while s > timestamp - self.size:
            out.append((s, s + self.size))
            s -= self.slide
        return out

    def is_event_time(self):
        return True


class EventTimeTrigger:
    @staticmethod
    def create():
        return EventTimeTrigger()


# ---- count windows: what KeyedStream.countWindow builds (KeyedStream.java countWindow(size) /
# countWindow(size, slide)): GlobalWindows with a CountTrigger, purging for the tumbling form, and a
# CountEvictor for the sliding form
class GlobalWindows:
    """GlobalWindows.create(): every element goes to the one GlobalWindow
    (flink-runtime/.../windowing/assigners/GlobalWindows.java); its maxTimestamp is Long.MAX_VALUE."""

    @staticmethod
    def create():
        return GlobalWindows()

    def is_event_time(self):
        return False


class CountTrigger:
    """CountTrigger.of(maxCount) (triggers/CountTrigger.java): FIRE once the count reaches maxCount."""

    def __init__(self, max_count):
        self.max_count = int(max_count)

    @staticmethod
    def of(max_count):
        return CountTrigger(max_count)


class PurgingTrigger:
    """PurgingTrigger.of(nestedTrigger) (triggers/PurgingTrigger.java): FIRE becomes FIRE_AND_PURGE."""

    def __init__(self, nested):
        if nested is None:
            raise ValueError("nested trigger must not be null")
        self.nested = nested

    @staticmethod
    def of(nested):
        return PurgingTrigger(nested)


class CountEvictor:
    """CountEvictor.of(maxCount[, doEvictAfter]) (evictors/CountEvictor.java): keeps up to maxCount
    elements, evicting from the beginning of the window before (or after) the window function."""

    def __init__(self, max_count, do_evict_after=False):
        self.max_count, self.do_evict_after = int(max_count), bool(do_evict_after)

    @staticmethod
    def of(max_count, do_evict_after=False):
        return CountEvictor(max_count, do_evict_after)


# ---- session windows: keyBy(...).window(EventTimeSessionWindows.withGap(gap))
class EventTimeSessionWindows:
    """EventTimeSessionWindows.withGap(size) (assigners/EventTimeSessionWindows.java): a merging
    assigner; every element gets the window [ts, ts + gap), and MergingWindowSet merges the windows
    of a key that intersect."""

    def __init__(self, gap_ms):
        if gap_ms <= 0:
            raise ValueError("EventTimeSessionWindows parameters must satisfy 0 < size")
        self.gap = int(gap_ms)

    @staticmethod
    def with_gap(gap_ms):
        return EventTimeSessionWindows(gap_ms)

    def assign_windows(self, ts):
        return [(ts, ts + self.gap)]

    def is_event_time(self):
        return True

    @staticmethod
    def with_dynamic_gap(extractor):
        return DynamicEventTimeSessionWindows(extractor)


class DynamicEventTimeSessionWindows:
    """EventTimeSessionWindows.withDynamicGap(extractor)
    (assigners/DynamicEventTimeSessionWindows.java): a merging assigner; every element gets the
    window [ts, ts + extractor.extract(element)), and a gap <= 0 throws."""

    def __init__(self, extractor):
        if not callable(extractor):
            raise ValueError("the session gap extractor must be callable")
        self.extractor = extractor

    @staticmethod
    def with_dynamic_gap(extractor):
        return DynamicEventTimeSessionWindows(extractor)

    def assign_windows(self, element, ts):
        gap = int(self.extractor(element))
        if gap <= 0:
            raise ValueError("Dynamic session time gap must satisfy 0 < gap")
        return [(ts, ts + gap)]

    def is_event_time(self):
        return True
