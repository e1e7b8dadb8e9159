"""Pure-Python restatement of KeyedStream.countWindow, the checker of the count-window tests.

countWindow(size, slide) = GlobalWindows + CountTrigger.of(slide) + CountEvictor.of(size), run by
EvictingWindowOperator: per key the operator keeps the ELEMENTS of the window and the trigger's count.
CountTrigger.onElement adds 1 to the count; at >= slide it clears the count and FIREs.
EvictingWindowOperator.emitWindowContents then lets CountEvictor.evictBefore drop the oldest
len - size elements (when len > size), reduces what remains in arrival order, emits the result and
writes the remaining elements back as the window's state.

countWindow(size) = GlobalWindows + PurgingTrigger.of(CountTrigger.of(size)), run by WindowOperator
with reducing state: FIRE_AND_PURGE at every size-th element of a key.

Nothing fires on a watermark (CountTrigger.onEventTime: CONTINUE).  This module deliberately keeps
element lists -- it knows nothing of count slices, the device path's representation.

Reduce rules (SumAggregator / ComparableAggregator on the field): sum(INT) wraps at 32 bits, sum(LONG)
at 64; DOUBLE sums add left to right; min / max replace the accumulator unless it is strictly
extremal by compareTo (Double.compareTo for DOUBLE: -0.0 < 0.0 < NaN, all NaNs equal).
"""
import struct

LONG_MAX = (1 << 63) - 1


def _wrap(v, bits):
    m = 1 << bits
    v &= m - 1
    return v - m if v >= m >> 1 else v


def _bits_to_double(b):
    return struct.unpack("<d", struct.pack("<q", _wrap(int(b), 64)))[0]


def _double_to_bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _double_compare(a, b):
    """Double.compareTo on bit patterns"""
    x, y = _bits_to_double(a), _bits_to_double(b)
    if x < y:
        return -1
    if x > y:
        return 1
    # equal, or a NaN is involved: Double.doubleToLongBits order (NaN canonical, -0.0 < 0.0)
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
        return a if cmp > 0 else b   # MaxComparator.isExtremal: o1.compareTo(o2) > 0
    if fn == "min":
        return a if cmp < 0 else b
    raise ValueError(fn)


class CountWindowReference:
    """``aggregation`` = (fn, ftype): fn in sum / min / max / count, ftype in LONG / INT / DOUBLE.
    process(keys, values) returns the rows fired by those elements, in emission order:
    (key, value, window_start, window_end, arrival index of the triggering element)."""

    def __init__(self, size, slide=None, aggregation=("sum", "LONG")):
        if size < 1 or (slide is not None and slide < 1):
            raise ValueError("size and slide must be >= 1")
        self.size, self.slide, self.purging = size, size if slide is None else slide, slide is None
        self.fn, self.ftype = aggregation[:2]
        self.elements = {}   # key -> window contents (field values)
        self.trigger = {}    # key -> CountTrigger's count
        self.seen = {}       # key -> elements so far (for window_start / window_end only)
        self.arrived = 0

    def process(self, keys, values):
        out = []
        for k, v in zip(keys, values):
            v = 1 if self.fn == "count" else int(v)
            lst = self.elements.setdefault(k, [])
            lst.append(v)
            self.seen[k] = self.seen.get(k, 0) + 1
            c = self.trigger.get(k, 0) + 1
            if c >= self.slide:
                self.trigger[k] = 0
                if not self.purging and len(lst) > self.size:   # CountEvictor.evictBefore
                    del lst[:len(lst) - self.size]
                acc = lst[0]
                for x in lst[1:]:
                    acc = _reduce(self.fn, self.ftype, acc, x)
                n = self.seen[k]
                out.append((k, acc, n - len(lst), n, self.arrived))
                if self.purging:
                    lst.clear()
            else:
                self.trigger[k] = c
            self.arrived += 1
        return out

    def process_watermark(self, watermark):
        return []   # CountTrigger.onEventTime: CONTINUE, also for Long.MAX_VALUE
