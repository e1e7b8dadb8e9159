// fw_session.h -- DataStream event-time session windows (EventTimeSessionWindows.withGap) as a
// sorted, dense list of sessions per superbucket.
//
// keyBy(...).window(EventTimeSessionWindows.withGap(gap)) runs WindowOperator.processElement's
// merging branch: the element's window [ts, ts + gap) goes through MergingWindowSet.addWindow, which
// merges it (TimeWindow.mergeWindows) with every window of the key it intersects
// (TimeWindow.intersects, inclusive: touching windows merge); EventTimeTrigger fires a window once
// the watermark reaches its maxTimestamp = end - 1.  With allowedLateness = 0 a batch's result per
// key is a union of intervals, independent of arrival order except for elements that are already
// late when they arrive (DESIGN.md "Session windows").
//
// This header holds the interval arithmetic the kernels and fw_host_session_add share (FW_HD), the
// per-handle state of a session operator (SessionOp) and the entry points fw_api.hip dispatches to.
#pragma once
#include "fw_count.h"

namespace fw {

struct SessionDesc {
    int64_t gap;       // EventTimeSessionWindows.withGap(gap)
    int32_t op;        // CountWordOp of the one accumulator word
    int32_t vtype;     // fw_value_type of the aggregated field
    int32_t is_count;  // COUNT_STAR: every element counts 1
    int32_t dbl_cmp;   // DOUBLE min / max: the accumulator holds dkey(value) (Double.compare order)
};

constexpr int64_t SW_MAX_GAP = (int64_t)1 << 40;
constexpr int SW_WORDS = 4;               // words per session: key, start, end, acc
constexpr int64_t SW_DEAD = INT64_MIN;    // end word of a scratch slot that holds no session

// TimeWindow.intersects: inclusive on both sides, so windows that merely touch merge
FW_HD bool session_intersects(int64_t a_start, int64_t a_end, int64_t b_start, int64_t b_end) {
    return a_start <= b_end && a_end >= b_start;
}
// TimeWindow.cover
FW_HD void session_cover(int64_t* start, int64_t* end, int64_t b_start, int64_t b_end) {
    if (b_start < *start) *start = b_start;
    if (b_end > *end) *end = b_end;
}
// WindowOperator.isWindowLate with allowedLateness 0, for the element's own window [ts, ts + gap)
FW_HD bool session_late(int64_t ts, int64_t gap, int64_t watermark) { return ts + gap - 1 <= watermark; }
// EventTimeTrigger: the window's timer at maxTimestamp = end - 1 fires once the watermark reaches it
FW_HD bool session_due(int64_t end, int64_t watermark) { return end - 1 <= watermark; }

// an element's value as an accumulator word, and a fired accumulator as the result value
FW_HD uint64_t session_word(const SessionDesc& d, uint64_t v) {
    if (d.is_count) return 1ull;
    return d.dbl_cmp ? (uint64_t)dkey(v) : v;
}
FW_HD uint64_t session_result(const SessionDesc& d, uint64_t acc) {
    if (d.dbl_cmp) return dkey_inv((int64_t)acc);
    if (d.vtype == FW_T_I32 && !d.is_count && d.op == CW_ADD_I) return (uint64_t)(int64_t)(int32_t)(uint32_t)acc;
    return acc;
}
// a result value back as the accumulator word it came from (fw_host_session_add keeps result values)
FW_HD uint64_t session_word_of_result(const SessionDesc& d, uint64_t r) { return d.dbl_cmp ? (uint64_t)dkey(r) : r; }
// the accumulator of no element: session_fold(op, identity, x) == x bit for bit
FW_HD uint64_t session_identity(int32_t op) {
    switch (op) {
        case CW_ADD_I: return 0ull;
        case CW_ADD_F: return 0x8000000000000000ull;  // -0.0: x + -0.0 == x for every x, -0.0 included
        case CW_MIN: return (uint64_t)INT64_MAX;
        default: return (uint64_t)INT64_MIN;
    }
}
FW_HD uint64_t session_fold(int32_t op, uint64_t older, uint64_t newer) { return count_fold(op, older, newer); }

// One element (ts, word) of one key against the key's sessions: n sessions sorted by start, pairwise
// non-touching, session i at start[i * stride], end[i * stride], acc[i * stride].  The element's
// window and every session it intersects become one session (MergingWindowSet.addWindow); an
// element that intersects nothing and is late is dropped and leaves the list untouched.
// Returns 1 merged or added, 0 dropped as late, -1 the list is full (capacity sessions).
FW_HD int session_add(const SessionDesc& d, int64_t watermark, int64_t ts, uint64_t word, int64_t* start, int64_t* end,
                      uint64_t* acc, int stride, int32_t* n, int32_t capacity) {
    const int32_t m = *n;
    const int64_t we = ts + d.gap;
    int32_t i = 0;
    while (i < m && !session_intersects(ts, we, start[(size_t)i * stride], end[(size_t)i * stride]) &&
           end[(size_t)i * stride] < ts)
        i++;
    int32_t j = i;
    while (j < m && session_intersects(ts, we, start[(size_t)j * stride], end[(size_t)j * stride])) j++;
    if (i == j) {
        if (session_late(ts, d.gap, watermark)) return 0;
        if (m >= capacity) return -1;
        for (int32_t k = m; k > i; k--) {
            start[(size_t)k * stride] = start[(size_t)(k - 1) * stride];
            end[(size_t)k * stride] = end[(size_t)(k - 1) * stride];
            acc[(size_t)k * stride] = acc[(size_t)(k - 1) * stride];
        }
        start[(size_t)i * stride] = ts;
        end[(size_t)i * stride] = we;
        acc[(size_t)i * stride] = word;
        *n = m + 1;
        return 1;
    }
    int64_t s = ts, e = we;
    uint64_t a = acc[(size_t)i * stride];
    for (int32_t k = i; k < j; k++) {
        session_cover(&s, &e, start[(size_t)k * stride], end[(size_t)k * stride]);
        if (k > i) a = session_fold(d.op, a, acc[(size_t)k * stride]);
    }
    start[(size_t)i * stride] = s;
    end[(size_t)i * stride] = e;
    acc[(size_t)i * stride] = session_fold(d.op, a, word);
    const int32_t gone = j - i - 1;
    if (gone > 0) {
        for (int32_t k = j; k < m; k++) {
            start[(size_t)(k - gone) * stride] = start[(size_t)k * stride];
            end[(size_t)(k - gone) * stride] = end[(size_t)k * stride];
            acc[(size_t)(k - gone) * stride] = acc[(size_t)k * stride];
        }
        *n = m - gone;
    }
    return 1;
}

constexpr int SW_TILE = CW_TILE;                   // rows per tile = threads per workgroup
constexpr int64_t SW_MAX_HIST = CW_MAX_HIST;       // [superbucket][chunk] partition counters a handle may hold
constexpr int64_t SW_SIDE_WORDS = 4;               // late side-output row: key, ts, push_seq << 32 | row, value

// Per-handle state of a session operator.  Superbucket sb's sessions are the first n_s[sb] entries of
// state[(sb * cap_s + i) * SW_WORDS ..]: key, start, end, acc, sorted by (key as uint64, start) and
// dense -- no tombstones: a fold rewrites the list, a fire compacts it.
struct SessionOp {
    bool on = false;
    SessionDesc d{};
    KeySpace ks{};
    int32_t val_col = 0;
    int32_t cap_s = 0;        // sessions per superbucket
    int32_t late_side = 0;    // late_side_output
    int64_t cap_rows = 0;     // rows per launch (max_batch_rows)
    int64_t max_nch = 0;      // partition chunks per launch
    int64_t out_cap = 0;
    int64_t side_cap = 0;     // late side-output rows: 2 * max_batch_rows
    uint64_t fingerprint = 0; // semantics fingerprint of the snapshot blobs
    hipStream_t stream = nullptr;
    Ctrl* ctrl = nullptr;     // out_count[0], fired, live_entries, late_dropped, n_side, error
    uint64_t* state = nullptr;
    uint64_t* scratch = nullptr;   // [n_sb][cap_s + SW_TILE] sessions: the merged list of one tile's fold
    int32_t* n_s = nullptr;        // [n_sb] sessions held
    int64_t* min_end = nullptr;    // [n_sb] a lower bound of the superbucket's smallest session end
    // partition scratch of one launch (as the count path's)
    int32_t* hist = nullptr;
    int32_t* seg = nullptr;
    int32_t* s_sb = nullptr;
    uint32_t* s_row = nullptr;
    int32_t* s_rank = nullptr;
    uint32_t* perm = nullptr;
    // result rows and the late side output
    int64_t* out_key = nullptr;
    int64_t* out_ws = nullptr;
    int64_t* out_we = nullptr;
    uint64_t* out_val = nullptr;
    uint32_t* out_null = nullptr;  // zeros
    int64_t* side = nullptr;       // [side_cap][SW_SIDE_WORDS]
    int64_t push_seq = 0;
};

// validation + plan of a FW_WIN_SESSION configuration; no device call
int sw_plan(const fw_config& c, SessionOp* op);
int sw_allocate(SessionOp* op, hipStream_t stream, Ctrl* ctrl);
void sw_free(SessionOp* op);
// folds n rows into the state under the watermark `watermark` (stream-ordered, asynchronous)
int sw_push(SessionOp* op, int64_t watermark, int64_t n, const int64_t* d_key, const int64_t* d_ts, const int32_t* d_khash,
            const uint64_t* d_val);
// fires every session with end - 1 <= watermark and compacts the rest (stream-ordered, asynchronous)
int sw_advance(SessionOp* op, int64_t watermark);
int sw_snapshot(SessionOp* op, int64_t watermark, int32_t key_group, void* buf, int64_t capacity, int64_t* size);
int sw_restore(SessionOp* op, bool key_group, const void* buf, int64_t size, int64_t* watermark);

}  // namespace fw
