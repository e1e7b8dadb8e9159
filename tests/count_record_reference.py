"""Pure-Python restatement of KeyedStream.countWindow programs that emit whole records, the checker of
the record count-window tests (recalled from the reference; nothing else pins these semantics).

At a key's c-th element with c % slide == 0 the window is that key's last min(c, size) elements in
arrival order (EvictingWindowOperator with CountEvictor.of(size), or reducing state with
PurgingTrigger for size == slide -- both amount to this), reduced left to right:
cur = reduce(cur, next), with the reducers WindowedStream / KeyedStream install:

sum(field)      SumAggregator: value1 with field = value1.field + value2.field (INT wraps at 32 bits,
                LONG at 64, DOUBLE adds left to right)
min / max       ComparableAggregator, byAggregate = false: value1, its field replaced by value2's
                unless value1's is strictly extremal (isExtremal: compareTo > 0 for max, < 0 for min)
minBy / maxBy   ComparableAggregator, byAggregate = true: value1 if its field is strictly extremal,
                on a tie value1 when ``first`` else value2, otherwise value2
DOUBLE fields compare by Double.compareTo (-0.0 < 0.0 < NaN, all NaNs equal).

So sum / min / max emit the window's OLDEST element with the aggregated field set, minBy / maxBy the
extremal element itself.  Nothing fires on a watermark.  The module keeps element lists and knows
nothing of ring slots; only held() speaks of count slices, because that is how the set of records an
operator must hold is defined: for a key with c elements, g = gcd(size, slide), R = size / g and
S = (c - 1) // g, one element of every slice in [max(0, S - R + 1), S] -- the slice's first element
(sum / min / max), or its extremal element under the tie rule (minBy / maxBy).
"""
import math
import struct

from count_window_reference import _double_compare, _wrap

BY = ("minBy", "maxBy")


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def double_of(b):
    return struct.unpack("<d", struct.pack("<q", _wrap(int(b), 64)))[0]


def field_compare(ftype, a, b):
    """compareTo of two field values (DOUBLE fields are Python floats)"""
    if ftype == "DOUBLE":
        return _double_compare(bits_of(a), bits_of(b))
    return (a > b) - (a < b)


def reduce_records(fn, ftype, first, field, v1, v2):
    """reduce(value1, value2) on records (tuples)"""
    a, b = v1[field], v2[field]
    put = lambda x: v1[:field] + (x,) + v1[field + 1:]
    if fn == "sum":
        if ftype == "DOUBLE":
            return put(a + b)
        return put(_wrap(a + b, 32 if ftype == "INT" else 64))
    c = field_compare(ftype, a, b)
    if fn in ("min", "max"):
        extremal = c < 0 if fn == "min" else c > 0
        return v1 if extremal else put(b)
    return v2 if by_takes_newer(fn, first, c) else v1


def by_takes_newer(fn, first, c):
    """minBy / maxBy: whether reduce(value1, value2) returns value2, c = value1.field.compareTo(value2.field)"""
    extremal = c < 0 if fn == "minBy" else c > 0
    if extremal:
        return False
    if c == 0:
        return not first
    return True


def record_image(rec):
    """a record with its floats as bit patterns: equality on images is bit-for-bit equality"""
    return tuple(("f64", bits_of(x)) if isinstance(x, float) else x for x in rec)


class CountRecordReference:
    """``aggregation`` = (fn, ftype[, first]); ``field`` the aggregated field's index in a record.
    process(keys, records, ordinals) returns the fired rows in emission order:
    (key, output record, ordinal of the triggering element, ordinal of the element the output is built
    from).  held() is the set of ordinals an operator must hold now."""

    def __init__(self, size, slide=None, aggregation=("sum", "LONG"), field=1):
        self.size, self.slide = size, size if slide is None else slide
        self.fn, self.ftype = aggregation[:2]
        self.first = aggregation[2] if len(aggregation) > 2 else True
        self.field = field
        self.g = math.gcd(self.size, self.slide)
        self.R = self.size // self.g
        self.elements = {}   # key -> every (ordinal, record) of the key, in arrival order

    def _reduce(self, cur, nxt):
        """on (ordinal, record): the ordinal of the element the result is built from travels along"""
        if self.fn in BY:
            c = field_compare(self.ftype, cur[1][self.field], nxt[1][self.field])
            return nxt if by_takes_newer(self.fn, self.first, c) else cur
        return (cur[0], reduce_records(self.fn, self.ftype, self.first, self.field, cur[1], nxt[1]))

    def _fold(self, elems):
        cur = elems[0]
        for nxt in elems[1:]:
            cur = self._reduce(cur, nxt)
        return cur

    def process(self, keys, records, ordinals):
        out = []
        for k, rec, o in zip(keys, records, ordinals):
            lst = self.elements.setdefault(k, [])
            lst.append((o, rec))
            c = len(lst)
            if c % self.slide == 0:
                ro, r = self._fold(lst[max(0, c - self.size):])
                out.append((k, r, o, ro))
        return out

    def held(self):
        out = set()
        for lst in self.elements.values():
            c = len(lst)
            S = (c - 1) // self.g
            for s in range(max(0, S - self.R + 1), S + 1):
                sl = lst[s * self.g:min((s + 1) * self.g, c)]
                out.add(self._fold(sl)[0] if self.fn in BY else sl[0][0])
        return out
