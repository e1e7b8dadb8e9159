// fw_session.h -- event-time session windows as a sorted, dense list of sessions per superbucket:
// DataStream EventTimeSessionWindows.withGap and the SQL SESSION window TVF aggregate.
//
// keyBy(...).window(EventTimeSessionWindows.withGap(gap)) runs WindowOperator.processElement's
// merging branch: the element's window [ts, ts + gap) goes through MergingWindowSet.addWindow, which
// merges it (TimeWindow.mergeWindows) with every window of the key it intersects
// (TimeWindow.intersects, inclusive: touching windows merge); EventTimeTrigger fires a window once
// the watermark reaches its maxTimestamp = end - 1.  With allowedLateness = 0 a batch's result per
// key is a union of intervals, independent of arrival order except for elements that are already
// late when they arrive (DESIGN.md "Session windows").
//
// The SQL form, SESSION(TABLE t PARTITION BY k, DESCRIPTOR(rowtime), gap) aggregated per (k,
// window_start, window_end), runs the same interval rules on the Table side (recalled, parity
// unpinned: UnsliceWindowAggProcessor, UnsliceAssigners.SessionUnsliceAssigner, the table runtime's
// MergingWindowProcessFunction.assignActualWindows / MergingFunctionImpl.merge and
// WindowAggOperator.processWatermark).  It differs in what a session carries: the accumulator words
// of a list of aggregates over NULL-able columns (the planner's WordDesc / AggDesc), 1 to 8 words
// rounded up to 1, 2, 4 or 8; a late row is dropped and counted, there is no side output.
//
// EventTimeSessionWindows.withDynamicGap(extractor) (FW_WIN_SESSION_DYNAMIC; recalled, parity
// unpinned: DynamicEventTimeSessionWindows.assignWindows) differs only in the element's window,
// [ts, ts + g) with g = extractor.extract(element) > 0: the gap arrives as a value column.  Window
// ends are then no longer ordered like the starts -- a window may lie inside an earlier, longer one.
// With an allowed lateness on top (FW_WIN_SESSION_DYNAMIC_LATENESS; recalled, parity unpinned) the
// lateness rules below hold with g in place of the gap wherever the element's own window is named.
//
// This header holds the interval arithmetic the kernels and fw_host_session_add share (FW_HD), the
// per-handle state of a session operator (SessionOp) and the entry points fw_api.hip dispatches to.
#pragma once
#include "fw_count.h"

namespace fw {

constexpr int SW_MAX_NW = MAX_WORDS;      // accumulator words of a session
constexpr int32_t SW_COL_ONE = -1;        // SessionDesc::col of a count word: every row counts 1
constexpr int32_t SW_COL_PAD = -2;        // ... of a padding word: an integer add of 0

struct SessionDesc {
    int64_t gap;       // EventTimeSessionWindows.withGap(gap) / the SESSION TVF's gap
    int32_t op;        // DataStream: CountWordOp of the one accumulator word (= ops[0])
    int32_t vtype;     // DataStream: fw_value_type of the aggregated field
    int32_t is_count;  // DataStream: COUNT_STAR, every element counts 1
    int32_t dbl_cmp;   // DataStream DOUBLE min / max: the accumulator holds dkey(value) (Double.compare order)
    int32_t sql;       // the SQL form: words from the planner's WordDesc, results through sql_agg_result
    int32_t nw;        // words the plan uses; the kernels carry sw_round_nw(nw)
    int32_t ops[SW_MAX_NW];   // CountWordOp per word (the word's merge class)
    int32_t col[SW_MAX_NW];   // value column the word reads, SW_COL_ONE or SW_COL_PAD
    int32_t gate[SW_MAX_NW];  // value column whose NULL rows the word skips, -1: none
};

constexpr int64_t SW_MAX_GAP = (int64_t)1 << 40;
constexpr int SW_WORDS = 4;               // words per one-word session: key, start, end, acc
FW_HD constexpr int sw_stride(int nw) { return 3 + nw; }  // words per session: key, start, end, acc[nw]
FW_HD constexpr int sw_round_nw(int nw) { return nw <= 1 ? 1 : nw <= 2 ? 2 : nw <= 4 ? 4 : 8; }
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
// The same with allowedLateness = L > 0 (FW_WIN_SESSION_LATENESS; recalled, parity unpinned:
// WindowOperator.isWindowLate / cleanupTime, EventTimeTrigger.onElement).  A window is late once its
// cleanup time maxTimestamp + L has passed; a session is held until then and fires when the
// watermark first reaches end - 1, so a held session with end - 1 <= W has fired with exactly its
// contents and the watermark alone tells which sessions have (no per-session bit).
FW_HD bool session_late_l(int64_t ts, int64_t gap, int64_t lateness, int64_t watermark) {
    return ts + gap - 1 + lateness <= watermark;
}
// the session's timer fires in an advance of the watermark from w0 to w1 > w0
FW_HD bool session_fires(int64_t end, int64_t w0, int64_t w1) { return w0 < end - 1 && end - 1 <= w1; }
// the session's cleanup timer at end - 1 + L has run at `watermark`: the session is removed
FW_HD bool session_cleaned(int64_t end, int64_t lateness, int64_t watermark) { return end - 1 + lateness <= watermark; }

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

// the merge class of a planner word as the CountWordOp that folds it, -1 outside the four classes
FW_HD int32_t session_op_of_word(int32_t wop) {
    switch (wop) {
        case W_CNT:
        case W_SUM_I: return CW_ADD_I;
        case W_SUM_F: return CW_ADD_F;
        case W_MIN_I: return CW_MIN;
        case W_MAX_I: return CW_MAX;
        default: return -1;
    }
}

// One element (ts, its NW words at words[w * wstride]) of one key against the key's sessions: n
// sessions sorted by start, pairwise non-touching, session i at start[i * stride], end[i * stride]
// and its NW accumulator words at acc[i * astride ..], word w folded under ops[w] (the word count is
// a template parameter so the device's copies unroll).  The element's window and every session
// it intersects become one session (MergingWindowSet.addWindow); an element that intersects nothing
// and is late is dropped and leaves the list untouched.  `gap` is the element's own: the handle's for
// a static-gap session, the row's for a dynamic-gap one.
// Returns 1 merged or added, 0 dropped as late, -1 the list is full (capacity sessions).
// LATE: the form with an allowed lateness.  The drop test is the window's cleanup time
// (session_late_l) and *at is the list index of the session the element produced, so that the caller
// can apply EventTimeTrigger.onElement: a resulting session with end - 1 <= watermark fires at once.
// The form without LATE reads neither `lateness` nor `at`.
template <int NW, bool LATE = false>
FW_HD int session_add(int64_t gap, const int32_t* ops, int64_t watermark, int64_t ts, const uint64_t* words, int wstride,
                      int64_t* start, int64_t* end, uint64_t* acc, int stride, int astride, int32_t* n, int32_t capacity,
                      int64_t lateness = 0, int32_t* at = nullptr) {
    const int32_t m = *n;
    const int64_t we = ts + gap;
    int32_t i = 0;
    while (i < m && !session_intersects(ts, we, start[(size_t)i * stride], end[(size_t)i * stride]) &&
           end[(size_t)i * stride] < ts)
        i++;
    int32_t j = i;
    while (j < m && session_intersects(ts, we, start[(size_t)j * stride], end[(size_t)j * stride])) j++;
    if (i == j) {
        if (LATE ? session_late_l(ts, gap, lateness, watermark) : session_late(ts, gap, watermark)) return 0;
        if (m >= capacity) return -1;
        for (int32_t k = m; k > i; k--) {
            start[(size_t)k * stride] = start[(size_t)(k - 1) * stride];
            end[(size_t)k * stride] = end[(size_t)(k - 1) * stride];
            for (int w = 0; w < NW; w++) acc[(size_t)k * astride + w] = acc[(size_t)(k - 1) * astride + w];
        }
        start[(size_t)i * stride] = ts;
        end[(size_t)i * stride] = we;
        for (int w = 0; w < NW; w++) acc[(size_t)i * astride + w] = words[(size_t)w * wstride];
        *n = m + 1;
        if (LATE) *at = i;
        return 1;
    }
    if (LATE) *at = i;
    int64_t s = ts, e = we;
    for (int32_t k = i; k < j; k++) {
        session_cover(&s, &e, start[(size_t)k * stride], end[(size_t)k * stride]);
        if (k > i)
            for (int w = 0; w < NW; w++)
                acc[(size_t)i * astride + w] = session_fold(ops[w], acc[(size_t)i * astride + w], acc[(size_t)k * astride + w]);
    }
    start[(size_t)i * stride] = s;
    end[(size_t)i * stride] = e;
    for (int w = 0; w < NW; w++) acc[(size_t)i * astride + w] = session_fold(ops[w], acc[(size_t)i * astride + w], words[(size_t)w * wstride]);
    const int32_t gone = j - i - 1;
    if (gone > 0) {
        for (int32_t k = j; k < m; k++) {
            start[(size_t)(k - gone) * stride] = start[(size_t)k * stride];
            end[(size_t)(k - gone) * stride] = end[(size_t)k * stride];
            for (int w = 0; w < NW; w++) acc[(size_t)(k - gone) * astride + w] = acc[(size_t)k * astride + w];
        }
        *n = m - gone;
    }
    return 1;
}

constexpr int SW_TILE = FD_TILE;                   // rows per tile = threads per workgroup
constexpr int64_t SW_SIDE_WORDS = 4;               // late side-output row: key, ts, push_seq << 32 | row, value

// Per-handle state of a session operator.  Superbucket sb's sessions are the first n_s[sb] entries of
// state[(sb * cap_s + i) * sw_stride(nw_t) ..]: key, start, end, acc[nw_t], sorted by (key as uint64,
// start) and dense -- no tombstones: a fold rewrites the list, a fire compacts it.
struct SessionOp {
    bool on = false;
    bool dyn = false;         // FW_WIN_SESSION_DYNAMIC: value column 1 is the row's gap, d.gap the largest allowed
    // (FW_WIN_SESSION_DYNAMIC_LATENESS sets both dyn and late)
    // Ctrl::cur in device memory is the watermark of record (a handle of parallelism > 1 that was
    // advanced from the device, sw_advance_device): every fold and advance reads it there, and the
    // host's mirror (fw_handle::host_cur) is only a lower bound until a reader synchronises
    bool wm_dev = false;
    // FW_WIN_SESSION_LATENESS: sessions are held until end - 1 + lateness, late elements into a held
    // session re-fire it (DESIGN.md "Session windows", Lateness)
    bool late = false;
    int64_t lateness = 0;
    SessionDesc d{};
    AggDesc ad{};             // SQL: the aggregates over the words (sql_agg_result)
    KeySpace ks{};
    int32_t nw_t = 1;         // sw_round_nw(d.nw): the kernels' instance
    int32_t n_out = 1;        // result value columns (SQL: one per aggregate)
    int32_t n_slots = 0;      // SQL: value columns the plan loads, slot_col[0 .. n_slots)
    int32_t slot_col[MAX_KCOLS] = {};
    int32_t val_col = 0;
    int32_t cap_s = 0;        // sessions per superbucket
    int32_t late_side = 0;    // late_side_output
    int64_t out_cap = 0;
    int64_t side_cap = 0;     // late side-output rows: 2 * max_batch_rows
    uint64_t fingerprint = 0; // semantics fingerprint of the snapshot blobs
    hipStream_t stream = nullptr;
    Ctrl* ctrl = nullptr;     // out_count[0], fired, live_entries, late_dropped, n_side, error
    uint64_t* state = nullptr;
    uint64_t* scratch = nullptr;   // [n_sb][cap_s + SW_TILE] sessions: the merged list of one tile's fold
    int32_t* n_s = nullptr;        // [n_sb] sessions held
    int64_t* min_end = nullptr;    // [n_sb] a lower bound of the superbucket's smallest session end
    // (late) min_end bounds every held session's end, so min_end - 1 + lateness the smallest cleanup
    // time; min_fire bounds the smallest end of a session that has not fired
    int64_t* min_fire = nullptr;   // [n_sb]
    int64_t* prev_wm = nullptr;    // (late) Ctrl::cur as it stood in front of the last device advance
    FoldedPart part{};             // the superbucket partition's buffers
    // result rows and the late side output
    int64_t* out_key = nullptr;
    int64_t* out_ws = nullptr;
    int64_t* out_we = nullptr;
    uint64_t* out_val[FW_MAX_AGGS] = {};  // [n_out] columns
    uint32_t* out_null = nullptr;  // DataStream: zeros
    int64_t* side = nullptr;       // [side_cap][SW_SIDE_WORDS]
    int64_t push_seq = 0;
};

// fw_api.hip: the aggregate planner of the time windows (fw_config.aggs -> WordDesc / AggDesc, the
// value slots the words read); the SQL session plan calls it too
int plan_aggs(const fw_config& c, WordDesc* wd, AggDesc* ad, int32_t* slot_col, int32_t* n_slots);
// validation + plan of a FW_WIN_SESSION configuration; no device call
int sw_plan(const fw_config& c, SessionOp* op);
int sw_allocate(SessionOp* op, hipStream_t stream, Ctrl* ctrl);
void sw_free(SessionOp* op);
// folds n rows into the state under the watermark `watermark` (stream-ordered, asynchronous)
// (DataStream: d_vals[val_col] is the one value column, d_nulls is not read)
int sw_push(SessionOp* op, int64_t watermark, int64_t n, const int64_t* d_key, const int64_t* d_ts, const int32_t* d_khash,
            const void* const* d_vals, const uint8_t* const* d_nulls);
// (op->wm_dev: under Ctrl::cur as it stands at that point of the stream; `watermark` is not read)
// The same for a padded exchange receive buffer behind the N > 1 keyBy exchange: n_segs segments of
// seg_len rows, segment s holding min(d_seg_counts[s], seg_len) live rows; row i's key, ts and value
// words at col[i * stride] (1: SoA columns; row_words: packed rows, the columns at rows + 0, 1, 2 + c),
// its hash and null flags at [i].  Padding rows are never read by the fold.  Folds under Ctrl::cur,
// which every advance of either kind keeps current.  A late side-output record's row is the row's
// position in the buffer.
int sw_push_segments(SessionOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_key,
                     const int64_t* d_ts, int32_t stride, const int32_t* d_khash, const void* const* d_vals,
                     const uint8_t* const* d_nulls);
// fires every session with end - 1 <= watermark and compacts the rest (stream-ordered, asynchronous)
// (lateness: the sessions with prev_watermark < end - 1 <= watermark fire, the ones with
// end - 1 + lateness <= watermark leave; the other kinds do not read prev_watermark)
int sw_advance(SessionOp* op, int64_t watermark, int64_t prev_watermark = 0);
// Ctrl::cur = W' = max(Ctrl::cur, *d_watermark or, with d_watermark NULL, watermark), then every session
// with end - 1 <= W' fires: two stream-ordered launches, no host wait.  Sets op->wm_dev.
int sw_advance_device(SessionOp* op, const int64_t* d_watermark, int64_t watermark);
// *watermark = Ctrl::cur behind everything queued on the handle's stream (synchronises)
int sw_read_watermark(SessionOp* op, int64_t* watermark);
int sw_snapshot(SessionOp* op, int64_t watermark, int32_t key_group, void* buf, int64_t capacity, int64_t* size);
int sw_restore(SessionOp* op, bool key_group, const void* buf, int64_t size, int64_t* watermark);

}  // namespace fw
