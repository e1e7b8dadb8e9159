// fw_api.hip -- C-ABI of libflinkwin (include/flinkwin.h): one handle per operator subtask.
//
// The handle owns a HIP stream, the device control block, the partial buffer that stands in
// for RecordsWindowBuffer (TR/operators/aggregate/window/buffers/RecordsWindowBuffer.java), the
// HBM slice-state table that replaces HeapKeyedStateBackend for this operator
// (FR/runtime/state/heap/HeapKeyedStateBackend.java:85) together with its timers
// (InternalTimerServiceImpl), and the result buffer.  Calls are asynchronous on the handle's
// stream except where a host value is needed (results, stats, snapshot).  This file plans, allocates,
// pushes, advances and reports; fw_results.hip delivers the rows, fw_checkpoint.hip the state.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fw_handle.h"

using namespace fw;

// this file's spellings of the library's one error function and one HIP check (fw_folded.h)
#define fail(...) fw::set_error(__VA_ARGS__)
#define HIP_TRY(expr) FD_TRY(expr)

namespace {

thread_local std::string g_err;

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        int64_t t = a % b;
        a = b;
        b = t;
    }
    return a < 0 ? -a : a;
}

int round_nw(int nw) { return nw <= 1 ? 1 : nw <= 2 ? 2 : nw <= 4 ? 4 : 8; }

// hipEvent pairs recorded around launches on the handle stream; resolved by fw_get_kernel_times
struct EvTimer final : KTimer {
    struct Rec {
        int kind;
        hipEvent_t b, e;
    };
    std::vector<hipEvent_t> pool;
    std::vector<Rec> recs;
    hipEvent_t open[FW_KT_N] = {};
    double ms[FW_KT_N] = {};
    int64_t n[FW_KT_N] = {};
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        // timing-only events: no system-scope fence (cache write-back + invalidate) at each
        // record, which would otherwise add ~10 us of idle stream time around every launch
        hipEvent_t e = nullptr;
        (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
        return e;
    }
    bool all = false;  // also the small bookkeeping launches (FW_KT_OTHER)
    void mark(int kind, bool end, hipStream_t s) override {
        if (kind == FW_KT_OTHER && !all) return;  // each event record costs the stream a few us
        hipEvent_t ev = get();
        (void)hipEventRecord(ev, s);
        if (!end) {
            open[kind] = ev;
        } else {
            recs.push_back({kind, open[kind], ev});
            open[kind] = nullptr;
        }
    }
    hipError_t resolve() {
        for (const Rec& r : recs) {
            hipError_t e = hipEventSynchronize(r.e);
            if (e != hipSuccess) return e;
            float t = 0.f;
            e = hipEventElapsedTime(&t, r.b, r.e);
            if (e != hipSuccess) return e;
            ms[r.kind] += t;
            n[r.kind]++;
            pool.push_back(r.b);
            pool.push_back(r.e);
        }
        recs.clear();
        return hipSuccess;
    }
    ~EvTimer() override {
        for (const Rec& r : recs) {
            hipEventDestroy(r.b);
            hipEventDestroy(r.e);
        }
        for (hipEvent_t e : pool) hipEventDestroy(e);
    }
};

}  // namespace

// fw_last_error's text, for every translation unit of the library: returns code
int fw::set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// pushes k_ingest_pack took, over every handle of the process (fw_ingest_pack_launches(NULL))
static std::atomic<int64_t> g_ig_pack_launches{0};
// superbuckets the GF_TAG merge variants served on the old path [0] and on the tag path [1], over the
// handles destroyed so far (fw_merge_path_superbuckets(NULL, .))
static std::atomic<int64_t> g_mg_path[2];

// The aggregate planner: fw_config.aggs -> accumulator words (WordDesc: op, value slot and NULL gate
// per word, shared words deduplicated) and the aggregates over them (AggDesc: w0, w1, nn, ...).
// slot_col[0 .. *n_slots) receives the value columns the words read.  The time windows and the SQL
// session plan (fw_session.hip) share it.
int fw::plan_aggs(const fw_config& c, WordDesc* wd_out, AggDesc* ad_out, int32_t* slot_col, int32_t* n_slots) {
    WordDesc& wd = *wd_out;
    AggDesc& ad = *ad_out;
    // ---- aggregates -> accumulator words
    if (c.api == FW_API_DATASTREAM && c.nullable_cols)
        return fail(FW_E_INVALID, "DataStream field aggregations have no NULL inputs");
    if (c.agg_phase != FW_PHASE_ONE && c.agg_phase != FW_PHASE_LOCAL && c.agg_phase != FW_PHASE_GLOBAL)
        return fail(FW_E_INVALID, "bad agg_phase %d", c.agg_phase);
    if (c.agg_phase != FW_PHASE_ONE && c.api != FW_API_SQL) return fail(FW_E_INVALID, "two-phase aggregation is SQL only");
    wd.nw = 0;
    wd.has_q = 0;
    int nslot = 0;
    auto nullable = [&](int col) { return ((c.nullable_cols >> col) & 1u) != 0; };
    auto slot_of = [&](int col) -> int {
        for (int s = 0; s < nslot; s++)
            if (slot_col[s] == col) return s;
        if (nslot >= MAX_KCOLS) return -1;
        slot_col[nslot] = col;
        return nslot++;
    };
    // one word per (op, slot, gate); COUNT words are identified by their gate alone
    auto word_of = [&](int op, int slot, int gate) -> int {
        for (int i = 0; i < wd.nw; i++)
            if (wd.op[i] == op && wd.gate[i] == gate && (op == W_CNT || wd.col[i] == slot)) return i;
        if (wd.nw >= MAX_WORDS) return -1;
        wd.op[wd.nw] = op;
        wd.col[wd.nw] = op == W_CNT ? 0 : slot;
        wd.gate[wd.nw] = gate;
        wd.qfirst[wd.nw] = -1;
        return wd.nw++;
    };
    ad.n = c.n_aggs;
    ad.count_star_word = -1;
    ad.first_word = -1;
    ad.by_prev = -1;
    for (int g = 0; g < FW_MAX_AGGS; g++) ad.dn_hi[g] = ad.dn_lo[g] = -1;
    if (c.ds_first_ordinals && c.api != FW_API_DATASTREAM)
        return fail(FW_E_INVALID, "ds_first_ordinals is a DataStream option (SQL output rows carry no input fields)");
    bool nn_star[FW_MAX_AGGS] = {};
    for (int g = 0; g < c.n_aggs; g++) {
        const fw_agg_desc& d = c.aggs[g];
        ad.kind[g] = d.kind;
        ad.type[g] = d.type;
        ad.w1[g] = ad.nn[g] = ad.qf[g] = ad.qn[g] = ad.qz[g] = -1;
        if (d.type < FW_T_I64 || d.type > FW_T_I32) return fail(FW_E_INVALID, "agg %d: bad type", g);
        const bool by = d.kind == FW_AGG_MINBY || d.kind == FW_AGG_MAXBY;
        if (d.flags & ~(by ? FW_AGGF_LAST : 0)) return fail(FW_E_INVALID, "agg %d: bad flags %d", g, d.flags);
        if (by && (c.api != FW_API_DATASTREAM || !c.ds_first_ordinals || c.n_aggs != 1))
            return fail(FW_E_INVALID, "minBy / maxBy are the one aggregation of a record-shaped DataStream operator (ds_first_ordinals)");
        int slot = 0, gate = -1;
        const bool global = c.agg_phase == FW_PHASE_GLOBAL;
        if (global) {
            // GLOBAL phase (GlobalAggCombiner.combine :77-110): the value columns are the local
            // accumulator fields the LOCAL phase emits, and every aggregate folds them with its
            // mergeExpressions: counts add, sums add (NULL-able), MIN/MAX compare, AVG adds its
            // (sum, count) pair.  Local counts and AVG sums are never NULL.
            if (d.input_col < 0 || d.input_col >= c.n_value_cols) return fail(FW_E_INVALID, "agg %d: bad input_col", g);
            const int sc = d.input_col;
            const bool fl = d.type == FW_T_F64;
            int w0 = -1;
            auto slot_chk = [&](int col) { const int sl = slot_of(col); return sl; };
            switch (d.kind) {
                case FW_AGG_COUNT_STAR:
                case FW_AGG_COUNT:
                    if (c.value_col_types[sc] != FW_T_I64 || nullable(sc))
                        return fail(FW_E_INVALID, "agg %d: a local count column is a NOT NULL BIGINT", g);
                    if ((slot = slot_chk(sc)) < 0) return fail(FW_E_INVALID, "more than %d distinct value columns", MAX_KCOLS);
                    w0 = word_of(W_CNTV, slot, -1);
                    break;
                case FW_AGG_AVG: {
                    if (sc + 1 >= c.n_value_cols || c.value_col_types[sc] != (fl ? FW_T_F64 : FW_T_I64) ||
                        c.value_col_types[sc + 1] != FW_T_I64 || nullable(sc) || nullable(sc + 1))
                        return fail(FW_E_INVALID, "agg %d: a local AVG is a NOT NULL (sum, BIGINT count) column pair", g);
                    const int s0 = slot_chk(sc), s1 = slot_chk(sc + 1);
                    if (s0 < 0 || s1 < 0) return fail(FW_E_INVALID, "more than %d distinct value columns", MAX_KCOLS);
                    w0 = word_of(fl ? W_SUM_F : W_SUM_I, s0, -1);
                    ad.w1[g] = word_of(W_CNTV, s1, -1);
                    if (ad.w1[g] < 0) return fail(FW_E_INVALID, "too many accumulator words");
                    break;
                }
                default: w0 = -2; break;  // SUM / MIN / MAX: as in one phase, below
            }
            if (w0 != -2) {
                if (w0 < 0) return fail(FW_E_INVALID, "too many accumulator words");
                ad.w0[g] = w0;
                continue;
            }
        }
        if (d.kind != FW_AGG_COUNT_STAR) {
            if (d.input_col < 0 || d.input_col >= c.n_value_cols) return fail(FW_E_INVALID, "agg %d: bad input_col", g);
            if (c.value_col_types[d.input_col] != d.type)
                return fail(FW_E_INVALID, "agg %d: type does not match value column type", g);
            if (d.kind != FW_AGG_COUNT || nullable(d.input_col)) {
                slot = slot_of(d.input_col);
                if (slot < 0) return fail(FW_E_INVALID, "more than %d distinct value columns", MAX_KCOLS);
                if (nullable(d.input_col)) gate = slot;
            }
        }
        if (c.api == FW_API_DATASTREAM && (d.kind == FW_AGG_AVG || d.kind == FW_AGG_COUNT))
            return fail(FW_E_INVALID, "DataStream built-in aggregations are sum/min/max (and COUNT_STAR)");
        const bool f = d.type == FW_T_F64;
        // non-NULL count of the input: gated COUNT for a nullable column, else COUNT(*)
        const int cnt_op = W_CNT;
        int w0 = -1;
        switch (d.kind) {
            case FW_AGG_COUNT_STAR: w0 = word_of(cnt_op, 0, -1); break;
            case FW_AGG_COUNT: w0 = word_of(cnt_op, slot, gate); break;
            case FW_AGG_SUM:
                w0 = word_of(f ? W_SUM_F : W_SUM_I, slot, gate);
                if (gate >= 0) ad.nn[g] = word_of(cnt_op, slot, gate);
                else nn_star[g] = true;
                break;
            case FW_AGG_MIN:
            case FW_AGG_MAX: {
                const bool mx = d.kind == FW_AGG_MAX;
                if (f && c.api == FW_API_SQL) {  // strict comparison in arrival order: word group
                    w0 = word_of(mx ? W_QMAX : W_QMIN, slot, gate);
                    ad.qf[g] = word_of(W_QFIRST, slot, gate);
                    ad.qn[g] = word_of(W_QNANLO, slot, gate);
                    ad.qz[g] = word_of(W_QZERO, slot, gate);
                    if (w0 < 0 || ad.qf[g] < 0 || ad.qn[g] < 0 || ad.qz[g] < 0) return fail(FW_E_INVALID, "too many accumulator words");
                    wd.qfirst[w0] = wd.qfirst[ad.qn[g]] = ad.qf[g];
                    wd.has_q = 1;
                    break;
                }
                w0 = word_of(f ? (mx ? W_MAX_D : W_MIN_D) : (mx ? W_MAX_I : W_MIN_I), slot, gate);
                if (gate >= 0) ad.nn[g] = word_of(cnt_op, slot, gate);
                else nn_star[g] = true;
                if (f && c.api == FW_API_DATASTREAM) {  // the last NaN's bits (Comparator ties)
                    ad.dn_hi[g] = word_of(W_DNHI, slot, gate);
                    ad.dn_lo[g] = word_of(W_DNLO, slot, gate);
                    if (ad.dn_hi[g] < 0 || ad.dn_lo[g] < 0) return fail(FW_E_INVALID, "too many accumulator words");
                }
                break;
            }
            case FW_AGG_AVG:
                w0 = word_of(f ? W_SUM_F : W_SUM_I, slot, gate);
                ad.w1[g] = word_of(cnt_op, slot, gate);
                break;
            case FW_AGG_MINBY:
            case FW_AGG_MAXBY: {  // the arg's field key, its ordinal, the ordinal the host retains
                const bool mx = d.kind == FW_AGG_MAXBY;
                w0 = word_of(f ? (mx ? W_BYMAX_D : W_BYMIN_D) : (mx ? W_BYMAX_I : W_BYMIN_I), slot, gate);
                ad.first_word = word_of((d.flags & FW_AGGF_LAST) ? W_BYO_LAST : W_BYO_FIRST, 0, -1);
                ad.by_prev = word_of(W_BYPREV, 0, -1);
                if (ad.first_word < 0 || ad.by_prev < 0) return fail(FW_E_INVALID, "too many accumulator words");
                break;
            }
            default: return fail(FW_E_INVALID, "agg %d: unsupported kind %d", g, d.kind);
        }
        if (w0 < 0 || (d.kind == FW_AGG_AVG && ad.w1[g] < 0)) return fail(FW_E_INVALID, "too many accumulator words");
        if ((d.kind == FW_AGG_SUM || d.kind == FW_AGG_MIN || d.kind == FW_AGG_MAX) && gate >= 0 && ad.nn[g] < 0 && ad.qf[g] < 0)
            return fail(FW_E_INVALID, "too many accumulator words");
        ad.w0[g] = w0;
    }
    if (c.count_star_index >= 0) {
        if (c.count_star_index >= c.n_aggs) return fail(FW_E_INVALID, "count_star_index out of range");
        const int k = c.aggs[c.count_star_index].kind;
        if (k != FW_AGG_COUNT_STAR && k != FW_AGG_COUNT) return fail(FW_E_INVALID, "count_star_index is not a COUNT");
        ad.count_star_word = ad.w0[c.count_star_index];
    } else if (c.window_kind == FW_WIN_HOP) {
        if (c.api == FW_API_SQL) return fail(FW_E_INVALID, "Hopping window requires a COUNT(*) in the aggregate functions.");
        // DataStream sliding windows emit a window iff it received an element: hidden COUNT(*)
        ad.count_star_word = word_of(W_CNT, 0, -1);
        if (ad.count_star_word < 0) return fail(FW_E_INVALID, "too many accumulator words");
    }
    if (c.ds_first_ordinals && ad.by_prev < 0) {
        ad.first_word = word_of(W_FIRST, 0, -1);
        if (ad.first_word < 0) return fail(FW_E_INVALID, "too many accumulator words");
    }
    wd.has_ord = wd.has_q;
    for (int i = 0; i < wd.nw; i++) wd.has_ord |= wd.op[i] == W_FIRST || is_dnword(wd.op[i]) || is_byword(wd.op[i]);
    // NOT NULL inputs: SUM / MIN / MAX are NULL only for an entry without rows (COUNT(*) == 0),
    // which needs a COUNT(*) word to be observable; without one such an entry never fires
    int star = -1;
    for (int i = 0; i < wd.nw; i++)
        if (wd.op[i] == W_CNT && wd.gate[i] < 0) star = i;
    for (int g = 0; g < c.n_aggs; g++)
        if (nn_star[g]) ad.nn[g] = star;
    *n_slots = nslot;
    return FW_OK;
}

namespace {

int validate_and_plan(fw_handle* h) {
    const fw_config& c = h->cfg;
    if (c.abi_version != FW_ABI_VERSION) return fail(FW_E_INVALID, "abi_version %d != %d", c.abi_version, FW_ABI_VERSION);
    if (c.api != FW_API_SQL && c.api != FW_API_DATASTREAM) return fail(FW_E_INVALID, "bad api %d", c.api);
    if (c.n_aggs < 1 || c.n_aggs > FW_MAX_AGGS) return fail(FW_E_INVALID, "n_aggs %d out of range", c.n_aggs);
    if (c.n_value_cols < 0 || c.n_value_cols > FW_MAX_COLS) return fail(FW_E_INVALID, "n_value_cols out of range");
    if (c.max_parallelism < 1 || c.max_parallelism > 32768) return fail(FW_E_INVALID, "max_parallelism out of range");
    if (c.parallelism < 1 || c.parallelism > c.max_parallelism) return fail(FW_E_INVALID, "parallelism out of range");
    if (c.subtask_index < 0 || c.subtask_index >= c.parallelism) return fail(FW_E_INVALID, "subtask_index out of range");
    if (c.key_hash < FW_KEYHASH_LONG || c.key_hash > FW_KEYHASH_KEYROW) return fail(FW_E_INVALID, "bad key_hash");
    if (c.window_kind == FW_WIN_COUNT || c.window_kind == FW_WIN_COUNT_RECORD) {  // count windows: a plan of their own (fw_count.hip)
        int rc = cw_plan(c, &h->cw);
        if (rc) return rc;
        h->ks = h->cw.ks;
        h->nv = h->cw.is_count ? 0 : 1;
        h->slot_col[0] = h->cw.val_col;
        h->n_out = 1;
        h->out_cap = c.output_capacity;
        h->stage_cap = c.max_batch_rows;
        return FW_OK;
    }
    if (c.window_kind == FW_WIN_SESSION || c.window_kind == FW_WIN_SESSION_DYNAMIC || c.window_kind == FW_WIN_SESSION_LATENESS ||
        c.window_kind == FW_WIN_SESSION_DYNAMIC_LATENESS) {  // session windows: a plan of their own (fw_session.hip)
        int rc = sw_plan(c, &h->sw);
        if (rc) return rc;
        h->ks = h->sw.ks;
        if (h->sw.d.sql) {  // the value columns the plan's words read (staged and checked per push)
            h->nv = h->sw.n_slots;
            for (int s = 0; s < h->nv; s++) h->slot_col[s] = h->sw.slot_col[s];
            h->ad = h->sw.ad;
        } else if (h->sw.dyn) {  // the aggregated field (unless a count) and the gap column
            h->nv = 0;
            if (!h->sw.d.is_count) h->slot_col[h->nv++] = 0;
            h->slot_col[h->nv++] = 1;
        } else {
            h->nv = h->sw.d.is_count ? 0 : 1;
            h->slot_col[0] = h->sw.val_col;
        }
        h->n_out = h->sw.n_out;
        h->out_cap = c.output_capacity;
        h->stage_cap = c.max_batch_rows;
        return FW_OK;
    }
    h->keyrow = c.key_hash == FW_KEYHASH_KEYROW;
    if (h->keyrow) {
        if (c.api != FW_API_SQL) return fail(FW_E_INVALID, "key rows (FW_KEYHASH_KEYROW) are SQL keys");
        const int32_t mb = c.key_row_max_bytes ? c.key_row_max_bytes : 120;  // 120: one 128-B line per id
        if (mb < 16 || mb > 4096 || (mb & 7)) return fail(FW_E_INVALID, "key_row_max_bytes must be a multiple of 8 in [16, 4096]");
        h->kr.stride_words = (int32_t)(((8 + mb) + 127) / 128 * 16);  // meta word + image, whole 128-B lines
        h->kr.max_len = mb;
    }
    if (c.size_ms <= 0) return fail(FW_E_INVALID, "window size must be > 0");
    // ---- window (SliceAssigners constructors' argument checks)
    WinDesc& w = h->win;
    w.kind = c.window_kind;
    w.size = c.size_ms;
    w.offset = c.offset_ms;
    switch (c.window_kind) {
        case FW_WIN_TUMBLE:
            if (!(c.offset_ms > -c.size_ms && c.offset_ms < c.size_ms))
                return fail(FW_E_INVALID, "Tumbling Window parameters must satisfy abs(offset) < size");
            w.interval = c.size_ms;
            w.n_slices = 1;
            if (c.api == FW_API_DATASTREAM) w.offset = c.offset_ms % c.size_ms;
            break;
        case FW_WIN_HOP:
            if (c.slide_ms <= 0) return fail(FW_E_INVALID, "Hopping Window must satisfy slide > 0 and size > 0");
            // SQL slices need slide | size (SliceAssigners.HoppingSliceAssigner); DataStream sliding
            // windows do not (SlidingEventTimeWindows.java:77-90): panes of gcd(size, slide) ms, each in
            // floor or ceil(size / slide) windows
            if (c.api != FW_API_DATASTREAM && c.size_ms % c.slide_ms != 0)
                return fail(FW_E_INVALID, "Slicing Hopping Window requires size must be an integral multiple of slide");
            if (c.api == FW_API_DATASTREAM && c.size_ms < c.slide_ms)  // gaps: panes in no window (not eligible)
                return fail(FW_E_INVALID, "sliding windows with size < slide run on the reference operator");
            if (c.api == FW_API_DATASTREAM && !(c.offset_ms > -c.slide_ms && c.offset_ms < c.slide_ms))
                return fail(FW_E_INVALID, "SlidingEventTimeWindows parameters must satisfy abs(offset) < slide and size > 0");
            w.interval = gcd64(c.size_ms, c.slide_ms);
            w.n_slices = (int32_t)(c.size_ms / w.interval);
            break;
        case FW_WIN_CUMULATE:
            if (c.api != FW_API_SQL) return fail(FW_E_INVALID, "CUMULATE is a SQL window");
            if (c.slide_ms <= 0 || c.size_ms % c.slide_ms != 0)
                return fail(FW_E_INVALID, "Cumulative Window requires maxSize must be an integral multiple of step");
            w.interval = c.slide_ms;
            w.n_slices = (int32_t)(c.size_ms / c.slide_ms);
            break;
        default: return fail(FW_E_INVALID, "bad window kind %d", c.window_kind);
    }
    w.ds = c.api == FW_API_DATASTREAM;
    w.slide = c.window_kind == FW_WIN_HOP ? c.slide_ms : c.size_ms;
    w.n_win = (w.ds && c.window_kind == FW_WIN_HOP) ? (int32_t)((c.size_ms + c.slide_ms - 1) / c.slide_ms) : 1;
    w.slide_div = make_udiv((uint64_t)w.slide);
    // ---- lateness (DataStream) and shift time zone (SQL TIMESTAMP_LTZ)
    if (c.allowed_lateness_ms < 0) return fail(FW_E_INVALID, "The allowed lateness cannot be negative.");
    if (c.api == FW_API_SQL && (c.allowed_lateness_ms != 0 || c.late_side_output))
        return fail(FW_E_INVALID, "allowed lateness and late side outputs are DataStream WindowOperator features");
    w.lateness = c.allowed_lateness_ms;
    if (c.tz_n < 0) return fail(FW_E_INVALID, "tz_n must be >= 0");
    if (c.tz_n > 0) {
        if (c.api != FW_API_SQL) return fail(FW_E_INVALID, "shift time zones belong to SQL TIMESTAMP_LTZ windows");
        if (!c.tz_utc || !c.tz_offset_ms) return fail(FW_E_INVALID, "tz_utc / tz_offset_ms required when tz_n > 0");
        if (c.tz_utc[0] != INT64_MIN) return fail(FW_E_INVALID, "tz_utc[0] must be Long.MIN_VALUE");
        h->tz_utc.assign(c.tz_utc, c.tz_utc + c.tz_n);
        h->tz_off.assign(c.tz_offset_ms, c.tz_offset_ms + c.tz_n);
        h->tz_bound.assign(c.tz_n, INT64_MIN);
        for (int i = 1; i < c.tz_n; i++) {
            if (h->tz_utc[i] <= h->tz_utc[i - 1]) return fail(FW_E_INVALID, "tz_utc must be strictly ascending");
            if (h->tz_off[i] < -18 * 3600000ll || h->tz_off[i] > 18 * 3600000ll) return fail(FW_E_INVALID, "offset out of range");
            h->tz_bound[i] = h->tz_utc[i] + std::max(h->tz_off[i - 1], h->tz_off[i]);
            if (h->tz_bound[i] <= h->tz_bound[i - 1]) return fail(FW_E_INVALID, "tz transitions too close together");
        }
    }
    w.tz = TzTable{h->tz_utc.data(), h->tz_off.data(), h->tz_bound.data(), c.tz_n, c.tz_use_dst ? 1 : 0};
    w.slice_div = make_udiv((uint64_t)w.interval);
    w.size_div = make_udiv((uint64_t)w.size);
    w.fast32 = w.interval < (1ll << 30) && w.offset < (1ll << 61) && w.offset > -(1ll << 61);
    w.slice_div32 = make_udiv32(w.fast32 ? (uint32_t)w.interval : 1u);
    h->always_flush = c.api == FW_API_DATASTREAM;

    // ---- aggregates -> accumulator words
    WordDesc& wd = h->wd;
    AggDesc& ad = h->ad;
    int32_t nslot = 0;
    if (int rc = plan_aggs(c, &wd, &ad, h->slot_col, &nslot)) return rc;
    h->nv = nslot;
    h->nw_t = round_nw(wd.nw);
    h->n_out = c.n_aggs + (ad.first_word >= 0 ? 1 : 0);  // + value1's ordinal (fw_result.first_ord)
    if (c.agg_phase == FW_PHASE_LOCAL) {  // output = local accumulator fields (AVG: sum, count)
        h->n_out = 0;
        for (int g = 0; g < c.n_aggs; g++) h->n_out += c.aggs[g].kind == FW_AGG_AVG ? 2 : 1;
        if (h->n_out > FW_MAX_AGGS) return fail(FW_E_INVALID, "LOCAL phase: more than %d accumulator fields", FW_MAX_AGGS);
    }
    for (int i = wd.nw; i < MAX_WORDS; i++) {
        wd.op[i] = W_CNT;
        wd.col[i] = 0;
        wd.gate[i] = -1;
        wd.qfirst[i] = -1;
    }

    // ---- key space: this subtask's key groups, split into superbuckets
    KeySpace& ks = h->ks;
    ks.hash_kind = h->keyrow ? FW_KEYHASH_PRECOMPUTED : c.key_hash;  // key rows route by their interned hash
    ks.max_p = c.max_parallelism;
    ks.maxp_div = make_udiv32((uint32_t)c.max_parallelism);
    ks.kg_start = (c.subtask_index * c.max_parallelism + c.parallelism - 1) / c.parallelism;
    const int kg_end = ((c.subtask_index + 1) * c.max_parallelism - 1) / c.parallelism;
    ks.n_kg = kg_end - ks.kg_start + 1;
    // SQL HOP with few slices per window and plain accumulators keeps block state (k_merge_hopb):
    // one entry per (key, HB_R consecutive slices) instead of one per (key, slice)
    const char* hb_env = getenv("FW_HOPB");
    if (const char* nv = getenv("FW_HB_NARROW")) h->hb_narrow = std::min(std::max(atoi(nv), 0), 2);
    w.hopb = c.api == FW_API_SQL && c.window_kind == FW_WIN_HOP && c.agg_phase != FW_PHASE_LOCAL && !wd.has_q &&
             h->nw_t <= 2 && w.n_slices <= HB_R && !(hb_env && atoi(hb_env) == 0);
    if (w.hopb) {
        w.hb_span = HB_R * w.interval;
        w.hb_span_div = make_udiv((uint64_t)w.hb_span);
    }
    h->pwe = 3 + (w.hopb ? HB_R * h->nw_t : h->nw_t);
    // the hint counts (key, slice) entries; a key's live slices (a window plus the batch's newer
    // ones) fit one or two blocks
    const int64_t cap_target = std::max<int64_t>(
        w.hopb ? c.state_capacity * 3 / (2 * (w.n_slices + 3)) : c.state_capacity, 1024);
    // aim for <= ~75% occupancy of the per-superbucket LDS entry table at the hinted capacity (the
    // index has 2E slots, so its load factor stays <= 38%); fewer, fuller superbuckets amortise the
    // merge kernel's per-workgroup costs (CFG5: 4096 -> 2048 superbuckets, merge -27%)
    h->cap_e = mg_entries(h->nw_t, c.api == FW_API_DATASTREAM ? KIND_DSWIN : w.hopb ? KIND_HOPB : c.window_kind);
    const int64_t fill = h->cap_e * h->fill_pct / 100;
    int64_t per_kg = (cap_target + ks.n_kg - 1) / ks.n_kg;
    int64_t sbk = fd_next_pow2((per_kg + fill - 1) / fill);
    // beyond IG_MAX_SB superbuckets the ingest partitions coarser than the state (KeySpace
    // pass_log2): up to MAX_PASS_LOG2 merge passes share one ingest superbucket's partial rows.  A
    // pass re-routes each row's key, so precomputed-hash keys (no hash in the partial rows) cap
    // the state at IG_MAX_SB superbuckets
    const int max_pl = ks.hash_kind == KH_PRE ? 0 : MAX_PASS_LOG2;
    const int64_t max_sb = (int64_t)IG_MAX_SB << max_pl;
    while ((int64_t)ks.n_kg * sbk > max_sb && sbk > 1) sbk >>= 1;
    if ((int64_t)ks.n_kg * sbk > max_sb) return fail(FW_E_INVALID, "too many key groups per subtask for the ingest histogram");
    ks.sb_per_kg_log2 = 0;
    while ((1ll << ks.sb_per_kg_log2) < sbk) ks.sb_per_kg_log2++;
    ks.n_sb = ks.n_kg << ks.sb_per_kg_log2;
    ks.pass_log2 = 0;
    while ((ks.n_sb >> ks.pass_log2) > IG_MAX_SB) ks.pass_log2++;
    if (ks.pass_log2 > ks.sb_per_kg_log2) return fail(FW_E_INVALID, "superbucket split finer than a key group's passes");
    if (c.max_batch_rows <= 0) return fail(FW_E_INVALID, "max_batch_rows must be > 0");
    if (c.output_capacity <= 0) return fail(FW_E_INVALID, "output_capacity must be > 0");
    h->chunk_rows = (int64_t)ig_block(h->nw_t, ig_nv(h->nv)) * ig_rpt(h->nw_t, ig_nv(h->nv));
    h->cap_rows = ((c.max_batch_rows + h->chunk_rows - 1) / h->chunk_rows) * h->chunk_rows;
    h->max_nch = h->cap_rows / h->chunk_rows;
    if (wd.has_ord && (int64_t)FW_MAX_PENDING * h->cap_rows >= (1ll << 32) - 1)
        return fail(FW_E_INVALID, "max_batch_rows too large for MIN/MAX(DOUBLE) / first-element arrival ordinals");
    h->cell_cols = cell_pad(h->max_nch);
    // compact partial rows: SQL rows on the UTC slice grid (the ingest kernel's common path; it falls
    // back to PF_WIDE per chunk), planned for COUNT(*)-only layouts, whose compact row is the key alone:
    // for the others the merge gather's cost of reading two formats outweighed the bytes saved
    // (DESIGN.md 5).  Key-row handles keep PF_WIDE: their collector reads the partial buffer's keys at
    // a fixed stride; split superbuckets (pass_log2) too.  FW_NARROW=0 switches them off (development).
    {
        const char* ne = getenv("FW_NARROW");
        const char* ne1 = getenv("FW_NARROW1");
        const bool count_only = wd.nw == 1 && wd.op[0] == W_CNT && wd.gate[0] < 0;
        // one accumulator word of a class with a compiled merge variant (MergeLayouts<1>): (key, acc)
        // rows, 17 B instead of 24 B per partial with the rank byte
        const bool one_word = wd.nw == 1 && !wd.has_q && !wd.has_ord && wd.gate[0] < 0 && ops_layout(wd) != OPS_ANY;
        const bool ok = c.api == FW_API_SQL && !h->keyrow && c.agg_phase != FW_PHASE_GLOBAL && h->tz_utc.empty() &&
                        w.fast32 && ks.pass_log2 == 0 && !(ne && atoi(ne) == 0) && (h->chunk_rows & (h->chunk_rows - 1)) == 0;
        // (one-word MAX / MIN / SUM layouts read compact rows slower in the merge than they save in the
        // ingest: measured 163 vs 148 us per CFG2 flush, ingest -1.6 us; FW_NARROW1=1 plans them)
        h->narrow = !ok ? 0 : count_only ? 2 : (one_word && ne1 && atoi(ne1) == 1) ? 1 : 0;
    }
    // runs: every chunk claims its stretch of each superbucket's sub-runs, so the merge streams a
    // superbucket's rows (fw_internal.h RUN_X).  Sub-runs hold 5/4 of a uniform share of a full push
    // (+16 rows); skew beyond that stays in the chunks' regions (overflow flags).  Off for key-row
    // handles (their collector reads the chunk regions) and split superbuckets (pass_log2: several
    // readers per ingest superbucket); FW_RUNS=1 / 0 forces them on / off (development A/B).
    {
        const char* re = getenv("FW_RUNS");
        const int n_isb = ks.n_sb >> ks.pass_log2;
        const int blk = ig_block(h->nw_t, ig_nv(h->nv)), rpt = ig_rpt(h->nw_t, ig_nv(h->nv));
        // measured per step: CFG4 (TUMBLE, two words) +2-4%, CFG2 (TUMBLE, one word) +1.5%
        // with its one-block runs gather (round 5: ingest +11 us, merge -14 us), CFG3 (HOP) -5%, CFG5
        // (CUMULATE) -3% -- the ingest's scattered stretch stores cost more than the merge saves there;
        // planned for SQL TUMBLE, FW_RUNS=1 plans them everywhere
        const bool want = re ? atoi(re) != 0 : (c.window_kind == FW_WIN_TUMBLE && c.api == FW_API_SQL);
        if (!h->keyrow && ks.pass_log2 == 0 && ig_runs_fit(n_isb, blk, rpt, h->nw_t) && want) {
            const int64_t subs = (int64_t)n_isb * RUN_X;
            const int64_t sc = ((h->cap_rows * 5 / 4 + subs - 1) / subs + 16 + 15) / 16 * 16;
            if (sc * subs < (1ll << 31)) {
                h->sub_cap = (int32_t)sc;
                h->run_rows = sc * subs;
            }
        }
    }
    // PF_PACK run rows: one 8-B word per partial (key and accumulator offsets, slice rank) for the
    // one-word integer layouts on the compact rows' conditions (COUNT / SUM / MIN / MAX of BIGINT or
    // INT, no NULLs); 24 -> 8 B per partial on the ingest's stores and the merge's reads.  FW_PACK=0
    // switches them off (A/B).
    {
        const char* pe = getenv("FW_PACK");
        const int32_t op = wd.op[0];
        const bool int_word = wd.nw == 1 && !wd.has_q && !wd.has_ord && wd.gate[0] < 0 &&
                              (op == W_CNT || op == W_SUM_I || op == W_MIN_I || op == W_MAX_I) && ops_layout(wd) != OPS_ANY;
        const bool ok = c.api == FW_API_SQL && !h->keyrow && c.agg_phase != FW_PHASE_GLOBAL && h->tz_utc.empty() &&
                        w.fast32 && ks.pass_log2 == 0 && (h->chunk_rows & (h->chunk_rows - 1)) == 0;
        h->pack = ok && int_word && h->run_rows > 0 && !(pe && atoi(pe) == 0);
        // k_ingest_pack takes the PF_PACK pushes of SQL TUMBLE handles with one value column, NOT NULL
        // columns and a key hash computed on the device, whose superbuckets fit its LDS plan (igp_serves).
        // COUNT(*) alone stays with k_ingest: its pushes that cannot pack are PF_UNIT / PF_NARROW.
        h->ig_pack_ok = h->pack && !h->narrow && c.window_kind == FW_WIN_TUMBLE && c.agg_phase != FW_PHASE_LOCAL &&
                        c.nullable_cols == 0 && ks.hash_kind != FW_KEYHASH_PRECOMPUTED && h->nv == 1 && op != W_CNT &&
                        ad.by_prev < 0 && ks.n_sb <= IGP_MAX_SB && h->chunk_rows == IGP_BLOCK * IGP_RPT;
        // the merge's tag path serves the flushes of PF_PACK pushes of SQL TUMBLE handles that keep state
        // (LOCAL emits partials instead); FW_MG_TAG=0 plans the plain variant (A/B)
        const char* te = getenv("FW_MG_TAG");
        h->mg_tag = h->pack && c.window_kind == FW_WIN_TUMBLE && c.agg_phase != FW_PHASE_LOCAL && !(te && atoi(te) == 0);
    }
    h->treq_cap = std::max<int64_t>(c.max_batch_rows * 2, 1 << 16);
    if (c.api == FW_API_DATASTREAM) {
        if (c.allowed_lateness_ms > 0 && (int64_t)FW_MAX_PENDING * h->cap_rows >= (1ll << 32) - 1)
            return fail(FW_E_INVALID, "max_batch_rows too large for late-element arrival ordinals");
        h->lfire_cap = c.allowed_lateness_ms > 0 ? h->treq_cap : 0;
        h->side_cap = c.late_side_output ? h->treq_cap : 0;
        // retains per flush <= new windows of its rows; releases <= live windows
        h->ordev_cap = ad.first_word >= 0
                           ? ((int64_t)FW_MAX_PENDING * h->cap_rows + std::max<int64_t>(c.state_capacity, 0)) * w.n_win + (1 << 16)
                           : 0;
    }
    h->out_cap = c.output_capacity;
    h->slab_cap = std::max<int64_t>(64, (2 * c.output_capacity + ks.n_sb - 1) / ks.n_sb);
    h->stage_cap = c.max_batch_rows;
    if (h->keyrow) {
        h->kr.cap_ids = std::max<int64_t>(1024, std::max<int64_t>(c.state_capacity, 0) + (int64_t)FW_MAX_PENDING * c.max_batch_rows);
        if (h->kr.cap_ids >= (1ll << 31) - 2) return fail(FW_E_INVALID, "key-row table over 2^31 ids");
        h->kr.n_slots = fd_next_pow2(2 * h->kr.cap_ids);
        h->krb_cap = c.max_batch_rows * (int64_t)h->kr.max_len;
    }
    return FW_OK;
}

// the hash kinds whose 256 x 16 instance keeps its rows in registers (the other two spill 4 VGPRs to
// scratch: tools/regs.sh), which the automatic geometry choice may take
static bool igp_auto_kind(int hash_kind) { return hash_kind == KH_BINROW_BIGINT || hash_kind == KH_BINROW_INT; }

int allocate(fw_handle* h) {
    const fw_config& c = h->cfg;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    int rc;
    const int PW = 2 + h->nw_t, PWE = h->pwe;
    if ((rc = fd_dalloc(&h->ctrl, 1))) return rc;
    if (h->cw.on) {  // a count handle holds its control block and the count path's own buffers
        if ((rc = cw_allocate(&h->cw, h->stream, h->ctrl))) return rc;
        HIP_TRY(launch_init_ctrl(h->ctrl, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return FW_OK;
    }
    if (h->sw.on) {  // likewise a session handle
        if ((rc = sw_allocate(&h->sw, h->stream, h->ctrl))) return rc;
        HIP_TRY(launch_init_ctrl(h->ctrl, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return FW_OK;
    }
    if ((rc = fd_dalloc(&h->parts, (size_t)FW_MAX_PENDING * h->cap_rows * PW))) return rc;
    if ((rc = fd_dalloc(&h->cells, (size_t)FW_MAX_PENDING * (h->ks.n_sb >> h->ks.pass_log2) * h->cell_cols))) return rc;
    if ((rc = fd_dalloc(&h->slot_nch, FW_MAX_PENDING))) return rc;
    if ((rc = fd_dalloc(&h->slot_base, FW_MAX_PENDING))) return rc;
    if (h->narrow && (rc = fd_dalloc(&h->ranks, (size_t)FW_MAX_PENDING * h->cap_rows))) return rc;
    if (h->run_rows) {
        // the runs layout is a plan, not a requirement: FW_MAX_PENDING * run_rows partial rows (about
        // 1.25x the partial buffer) on top of it.  When the device cannot hold them the handle keeps
        // the cell layout instead of failing fw_create.
        void* r = nullptr;
        void* rr = nullptr;
        if (hipMalloc(&r, (size_t)FW_MAX_PENDING * h->run_rows * PW * sizeof(uint64_t)) != hipSuccess ||
            (h->narrow && hipMalloc(&rr, (size_t)FW_MAX_PENDING * h->run_rows) != hipSuccess)) {
            (void)hipGetLastError();
            if (r) hipFree(r);
            h->run_rows = 0;
            h->sub_cap = 0;
            h->pack = 0;
            h->mg_tag = false;
            h->ig_pack_ok = false;
        } else {
            h->runs = (uint64_t*)r;
            h->run_ranks = (uint8_t*)rr;
        }
    }
    if (h->ig_pack_ok && h->igp_geom < 0) {  // the resident sets the automatic geometry choice compares a push with
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
        for (int g = 0; g < 2; g++) {
            const int occ = ingest_pack_occupancy(g);
            if (occ < 0) return fail(FW_E_DEVICE, "k_ingest_pack occupancy query: %s", hipGetErrorString((hipError_t)-occ));
            h->igp_res[g] = (int64_t)occ * cus;
        }
    }
    if (h->run_rows) {
        const size_t n_isb = (size_t)(h->ks.n_sb >> h->ks.pass_log2);
        if ((rc = fd_dalloc(&h->run_fill, (size_t)FW_MAX_PENDING * RUN_X * n_isb))) return rc;
        if ((rc = fd_dalloc(&h->run_ovf, (size_t)FW_MAX_PENDING * n_isb))) return rc;
        if ((rc = fd_dalloc(&h->slot_fmt, FW_MAX_PENDING))) return rc;
        HIP_TRY(hipMemsetAsync(h->run_fill, 0, sizeof(uint32_t) * FW_MAX_PENDING * RUN_X * n_isb, h->stream));
        HIP_TRY(hipMemsetAsync(h->run_ovf, 0, sizeof(uint32_t) * FW_MAX_PENDING * n_isb, h->stream));
        HIP_TRY(hipMemsetAsync(h->slot_fmt, 0, sizeof(int32_t) * FW_MAX_PENDING, h->stream));
    }
    if ((rc = fd_dalloc(&h->treq, (size_t)h->treq_cap * 3))) return rc;
    if (h->lfire_cap && (rc = fd_dalloc(&h->lfire, (size_t)h->lfire_cap * LFW))) return rc;
    if (h->side_cap && (rc = fd_dalloc(&h->side, (size_t)h->side_cap * SOW))) return rc;
    if (h->ordev_cap && (rc = fd_dalloc(&h->ordev, (size_t)h->ordev_cap))) return rc;
    if (h->keyrow) {
        KeyRowTable& t = h->kr;
        if ((rc = fd_dalloc(&t.slots, (size_t)t.n_slots))) return rc;
        if ((rc = fd_dalloc(&t.arena, (size_t)t.cap_ids * t.stride_words))) return rc;
        if ((rc = fd_dalloc(&t.mark, (size_t)t.cap_ids))) return rc;
        if ((rc = fd_dalloc(&t.free_list, (size_t)t.cap_ids))) return rc;
        HIP_TRY(hipMemsetAsync(t.slots, 0, sizeof(uint32_t) * t.n_slots, h->stream));
        HIP_TRY(hipMemsetAsync(t.mark, 0, sizeof(uint32_t) * t.cap_ids, h->stream));
        if ((rc = fd_dalloc(&h->res_kr_len, (size_t)h->out_cap))) return rc;
        if ((rc = fd_dalloc(&h->res_kr_img, (size_t)h->out_cap * (t.stride_words - 1)))) return rc;
    }
    if (!h->tz_utc.empty()) {  // shift-zone table on the device; the kernels' WinDesc points at it
        const size_t n = h->tz_utc.size();
        if ((rc = fd_dalloc(&h->d_tz, 3 * n))) return rc;
        HIP_TRY(hipMemcpy(h->d_tz, h->tz_utc.data(), 8 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_tz + n, h->tz_off.data(), 8 * n, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_tz + 2 * n, h->tz_bound.data(), 8 * n, hipMemcpyHostToDevice));
    }
    if ((rc = fd_dalloc(&h->state, (size_t)h->ks.n_sb * h->cap_e * PWE))) return rc;
    if ((rc = fd_dalloc(&h->state_count, h->ks.n_sb))) return rc;
    if ((rc = fd_dalloc(&h->sb_min_timer, h->ks.n_sb))) return rc;
    if ((rc = fd_dalloc(&h->sb_nar, h->ks.n_sb))) return rc;
    const size_t orows = (size_t)h->ks.n_sb * h->slab_cap + h->out_cap;
    if ((rc = cols_alloc_device(&h->out, orows, h->n_out, false))) return rc;  // (window_start is derived at the compaction)
    if ((rc = cols_alloc_device(&h->res, (size_t)h->out_cap, h->n_out, true))) return rc;
    if ((rc = fd_dalloc(&h->sb_out, h->ks.n_sb + 1))) return rc;  // + the overflow region's rows
    if ((rc = fd_dalloc(&h->sb_fired, h->ks.n_sb))) return rc;
    if ((rc = fd_dalloc(&h->coff, h->ks.n_sb + 2))) return rc;
    if ((rc = fd_dalloc(&h->chunk_stats, CS_WORDS * (h->max_nch + 1)))) return rc;
    if ((rc = fd_dalloc(&h->stamps, N_STAMPS))) return rc;
    if ((rc = fd_dalloc(&h->kt_dev, FW_KT_N * KT_WORDS))) return rc;
    if ((rc = fd_dalloc(&h->tickets, 1))) return rc;
    HIP_TRY(hipHostMalloc((void**)&h->mirror, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
    *h->mirror = ~0ull;
    HIP_TRY(hipHostGetDevicePointer((void**)&h->d_mirror, (void*)h->mirror, 0));
    HIP_TRY(hipHostMalloc((void**)&h->ig_mirror, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
    *h->ig_mirror = ~0ull;
    HIP_TRY(hipHostGetDevicePointer((void**)&h->d_ig_mirror, (void*)h->ig_mirror, 0));
    HIP_TRY(hipMemsetAsync(h->tickets, 0, sizeof(Tickets), h->stream));
    if (h->ig_pack_ok)  // only handles that may choose k_ingest_pack have their ingest launches report
        HIP_TRY(hipMemcpyAsync(&h->tickets->ig_mirror, &h->d_ig_mirror, sizeof(h->d_ig_mirror), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->stamps, 0, sizeof(unsigned long long) * N_STAMPS, h->stream));
    HIP_TRY(hipMemsetAsync(h->kt_dev, 0, sizeof(unsigned long long) * FW_KT_N * KT_WORDS, h->stream));
    HIP_TRY(hipMemsetAsync(h->sb_out, 0, sizeof(int32_t) * (h->ks.n_sb + 1), h->stream));
    HIP_TRY(hipMemsetAsync(h->sb_fired, 0, sizeof(uint32_t) * h->ks.n_sb, h->stream));
    HIP_TRY(hipMemsetAsync(h->state_count, 0, sizeof(int32_t) * h->ks.n_sb, h->stream));
    HIP_TRY(hipMemsetAsync(h->sb_nar, 0, h->ks.n_sb, h->stream));
    std::vector<int64_t> inf(h->ks.n_sb, INT64_MAX);
    HIP_TRY(hipMemcpyAsync(h->sb_min_timer, inf.data(), sizeof(int64_t) * h->ks.n_sb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_init_ctrl(h->ctrl, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FW_OK;
}

int alloc_staging(fw_handle* h) {
    if (h->d_ts[0]) return FW_OK;
    const fw_config& c = h->cfg;
    const size_t n = (size_t)h->stage_cap;
    HIP_TRY(hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
    int rc;
    for (int b = 0; b < FW_STAGE_BUFS; b++) {
        HIP_TRY(hipHostMalloc((void**)&h->h_key[b], n * 8, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&h->h_ts[b], n * 8, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void**)&h->h_kh[b], n * 4, hipHostMallocDefault));
        for (int v = 0; v < c.n_value_cols; v++) {
            HIP_TRY(hipHostMalloc((void**)&h->h_val[b][v], n * 8, hipHostMallocDefault));
            if ((c.nullable_cols >> v) & 1u) HIP_TRY(hipHostMalloc((void**)&h->h_nul[b][v], n, hipHostMallocDefault));
        }
        HIP_TRY(hipEventCreateWithFlags(&h->stage_ev[b], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->stage_ev[b], h->cstream));
        HIP_TRY(hipEventCreateWithFlags(&h->dstage_free[b], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->dstage_free[b], h->stream));
        if (h->keyrow) {
            HIP_TRY(hipHostMalloc((void**)&h->h_kro[b], (n + 1) * 8, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc((void**)&h->h_krb[b], (size_t)std::max<int64_t>(h->krb_cap, 8), hipHostMallocDefault));
            if ((rc = fd_dalloc(&h->d_kro[b], n + 1))) return rc;
            if ((rc = fd_dalloc(&h->d_krb[b], (size_t)std::max<int64_t>(h->krb_cap, 8)))) return rc;
        } else {
            if ((rc = fd_dalloc(&h->d_key[b], n))) return rc;
        }
        if ((rc = fd_dalloc(&h->d_ts[b], n))) return rc;
        if (c.key_hash == FW_KEYHASH_PRECOMPUTED && (rc = fd_dalloc(&h->d_kh[b], n))) return rc;
        for (int v = 0; v < c.n_value_cols; v++) {
            if ((rc = fd_dalloc(&h->d_val[b][v], n))) return rc;
            if (((c.nullable_cols >> v) & 1u) && (rc = fd_dalloc(&h->d_nul[b][v], n))) return rc;
        }
    }
    return FW_OK;
}

MergeArgs merge_args(fw_handle* h, int64_t wm, int force) {
    MergeArgs a{};
    a.ks = h->ks;
    a.ctrl = h->ctrl;
    a.tickets = h->tickets;
    a.parts = h->parts;
    a.cells = h->cells;
    a.slot_nch = h->slot_nch;
    a.max_nch = h->cell_cols;
    a.cap_rows = h->cap_rows;
    a.treq = h->treq;
    a.treq_cap = h->treq_cap;
    a.state = h->state;
    a.state_count = h->state_count;
    a.sb_min_timer = h->sb_min_timer;
    a.sb_nar = h->sb_nar;
    a.hb_narrow = h->win.hopb ? h->hb_narrow : 0;
    a.n_sb = h->ks.n_sb;
    a.cap_e = h->cap_e;
    a.win = device_win(h);
    a.lfire = h->lfire;
    a.lfire_cap = h->lfire_cap;
    a.wd = h->wd;
    a.ad = h->ad;
    a.always_flush = h->always_flush;
    a.local = h->cfg.agg_phase == FW_PHASE_LOCAL;
    a.chunk_rows = (int32_t)h->chunk_rows;
    a.out_key = h->out.key;
    a.out_we = h->out.we;
    for (int g = 0; g < FW_MAX_AGGS; g++) a.out_val[g] = h->out.val[g] ? h->out.val[g] : h->out.val[0];
    a.out_null = h->out.null;
    a.out_cap = h->out_cap;
    a.slab_cap = h->slab_cap;
    a.sb_out = h->sb_out;
    a.sb_fired = h->sb_fired;
    a.wm = wm;
    a.force_flush = force;
    a.reset_out = h->reset_pending;
    a.ablate = h->ablate;
    a.stamps = h->stamps;
    a.kt = h->kt_device ? h->kt_dev + FW_KT_MERGE * KT_WORDS : nullptr;
    a.host_mirror = h->d_mirror;  // the launch's last workgroup reports merge_seq << 8 | pending pushes
    a.merge_seq = h->merge_seq;
    a.ordev = h->ordev;
    a.ordev_cap = h->ordev_cap;
    a.slot_base = h->slot_base;
    a.ranks = h->ranks;
    a.compact = h->narrow != 0 || h->pack != 0;
    a.runs = h->runs;
    a.run_ranks = h->run_ranks;
    a.run_fill = h->run_fill;
    a.run_ovf = h->run_ovf;
    a.slot_fmt = h->slot_fmt;
    a.run_rows = h->run_rows;
    a.sub_cap = h->sub_cap;
    a.tag = h->mg_tag && h->pack && h->runs;
    a.ch_log2 = 0;
    while ((1ll << a.ch_log2) < h->chunk_rows) a.ch_log2++;
    return a;
}

// One merge launch and its bookkeeping.  wm_dev: the watermark is read on the device (fw_advance_device, wm
// is INT64_MIN); the host mirrors of currentProgress then stay behind the device -- they only ever skip
// launches, so a stale, lower value skips fewer.
int launch_merge(fw_handle* h, int64_t wm, int force, const int64_t* wm_dev = nullptr) {
    MergeArgs a = merge_args(h, wm, force);
    a.wm_dev = wm_dev;
    HIP_TRY(launch_merge_fire(a, h->stream, h->timer));
    h->pushes_at_merge[h->merge_seq % 64] = h->pushes_total;
    h->merge_seq++;
    h->ig_merges++;
    h->reset_pending = false;  // the launch started every output slab (and the overflow) afresh
    if (!wm_dev && !force && wm > h->dev_cur) {  // merge_finalize's advanceProgress bookkeeping, mirrored
        h->dev_cur = wm;
        if (wm >= h->dev_ntp) h->dev_ntp = tz_next_trigger_watermark(h->win.tz, wm, h->win.slice_div);
    }
    return FW_OK;
}

int push(fw_handle* h, int64_t n, const int64_t* key, const int64_t* ts, const int32_t* kh, const void* const* vals,
         const uint8_t* const* nulls, const int64_t* seg_counts = nullptr, int64_t seg_len = 1, int64_t stride = 1) {
    if (h->ad.first_word >= 0 && (n >= (1ll << 32) || h->push_seq >= (1 << 30)))
        return fail(FW_E_INVALID, "arrival ordinals need < 2^32 rows per call and < 2^30 calls");
    for (int64_t o = 0; o < n; o += h->cap_rows) {
        const int64_t m = std::min(h->cap_rows, n - o);
        if (h->pushes_ub >= FW_MAX_PENDING) {
            // what the last completed merge launch left pending, plus the pushes issued after it.
            // While merge launches issued since are still running, wait for them to report
            // instead of draining the stream: the queue stays busy while the host waits.
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                const unsigned long long v = *h->mirror;
                const uint64_t seq = v >> 8;
                const bool valid = v != ~0ull && seq < h->merge_seq && h->merge_seq - seq <= 64;
                if (valid)
                    h->pushes_ub = std::min<int64_t>(h->pushes_ub,
                                                     (int64_t)(v & 0xff) + (int64_t)(h->pushes_total - h->pushes_at_merge[seq % 64]));
                if (h->pushes_ub < FW_MAX_PENDING || !valid || seq + 1 >= h->merge_seq) break;
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;  // read_ctrl below
                std::this_thread::yield();
            }
        }
        if (h->pushes_ub >= FW_MAX_PENDING) {
            Ctrl c;
            int rc = read_ctrl(h, &c);
            if (rc) return rc;
            h->pushes_ub = c.pending_pushes;
            if (h->pushes_ub >= FW_MAX_PENDING) {
                // buffer full: flush into state (RecordsWindowBuffer.addElement EOFException path)
                if ((rc = force_flush(h))) return rc;
            }
        }
        IngestArgs a{};
        a.stride = stride;
        a.key = key + o * stride;
        a.ts = ts + o * stride;
        a.khash = kh ? kh + o : nullptr;
        for (int s = 0; s < MAX_KCOLS; s++) {
            const bool live = s < h->nv;
            a.vals[s] = live ? (const uint64_t*)vals[h->slot_col[s]] + o * stride : nullptr;
            a.nulls[s] = live && ((h->cfg.nullable_cols >> h->slot_col[s]) & 1u) ? nulls[h->slot_col[s]] + o : nullptr;
        }
        a.n = m;
        a.win = device_win(h);
        a.lfire = h->lfire;
        a.lfire_cap = h->lfire_cap;
        a.side = h->side;
        a.side_cap = h->side_cap;
        a.side_output = h->cfg.late_side_output ? 1 : 0;
        a.push_seq = h->push_seq;
        a.row0 = o;
        a.seg_counts = seg_counts;
        a.fold_always = h->fold_always;
        a.no_fold = h->ad.by_prev >= 0;
        a.seg_div = make_udiv((uint64_t)std::max<int64_t>(seg_len, 1));
        a.ks = h->ks;
        a.wd = h->wd;
        a.nv = h->nv;
        a.ctrl = h->ctrl;
        a.tickets = h->tickets;
        a.parts = h->parts;
        a.cap_rows = h->cap_rows;
        a.cells = h->cells;
        a.slot_nch = h->slot_nch;
        a.max_nch = h->cell_cols;
        a.chunk_stats = h->chunk_stats;
        a.n_chunks = (m + h->chunk_rows - 1) / h->chunk_rows;
        a.treq = h->treq;
        a.treq_cap = h->treq_cap;
        a.lds_bytes = ig_lds(ig_block(h->nw_t, ig_nv(h->nv)));
        a.local = h->cfg.agg_phase == FW_PHASE_LOCAL;
        a.global = h->cfg.agg_phase == FW_PHASE_GLOBAL;
        a.ablate = h->ablate;
        a.kt = h->kt_device ? h->kt_dev + FW_KT_REDUCE * KT_WORDS : nullptr;
        a.narrow = h->narrow;
        a.rank_lim = std::min<int64_t>(PF_MAX_RANK + 1, ((1ll << 31) - 1) / std::max<int64_t>(h->win.interval, 1)) *
                     h->win.interval;
        a.slot_base = h->slot_base;
        a.ranks = h->ranks;
        a.runs = h->runs;
        a.run_ranks = h->run_ranks;
        a.run_fill = h->run_fill;
        a.run_ovf = h->run_ovf;
        a.slot_fmt = h->slot_fmt;
        a.run_rows = h->run_rows;
        a.sub_cap = h->sub_cap;
        a.pack = h->pack;
        // k_ingest_pack or k_ingest (fw_host_ig_pack_choice).  The mirror may lag the device by the
        // launches in flight: the packing kernel checks again on the device and falls back per launch
        // or per chunk, so a stale word costs time only.
        const unsigned long long igv = h->ig_mirror ? *h->ig_mirror : ~0ull;
        const int32_t choice = fw_host_ig_pack_choice(
            h->ig_pack_mode, igv, h->ig_since_fold, h->ig_merges,
            (h->ig_pack_ok ? 0u : FW_IGX_PLAN) | (kh ? FW_IGX_KEY_HASH : 0u) | (seg_counts ? FW_IGX_SEGMENTS : 0u) |
                (stride != 1 ? FW_IGX_STRIDE : 0u) | (h->fold_always ? FW_IGX_FOLD_ALWAYS : 0u));
        const bool packing = choice == FW_IG_PACK;
        if (choice == FW_IG_FOLD) a.fold_always = 1;  // the push on which k_ingest folds and measures again
        if (packing) h->igp_last = h->igp_geom >= 0 ? h->igp_geom : (a.n_chunks > h->igp_res[0] && a.n_chunks <= h->igp_res[1] && igp_auto_kind(h->ks.hash_kind));
        HIP_TRY(packing ? launch_ingest_pack(a, h->igp_last, h->stream, h->timer) : launch_ingest(a, h->stream, h->timer));
        // k_ingest does not write the mirror itself: a one-thread launch behind it does (in the steady
        // state of a uniform stream that is one push in 64)
        if (!packing && h->ig_pack_ok && h->ig_pack_mode == 1) HIP_TRY(launch_ig_report(h->tickets, h->ctrl, h->stream));
        // a k_ingest launch folds when told to, when fold_skip is clear, and on every 8th push by
        // Ctrl::push_count, which ig_pushes follows
        if (!packing && (a.fold_always || (h->ig_pushes & 7u) == 0 || (igv != ~0ull && !(igv & IGM_FOLD_SKIP)))) h->ig_since_fold = 0;
        h->ig_since_fold++;
        h->ig_pushes++;
        if (packing) {
            h->ig_pack_launches++;
            g_ig_pack_launches.fetch_add(1, std::memory_order_relaxed);
        }
        h->pushes_ub++;
        h->pushes_total++;
    }
    h->push_seq++;
    return FW_OK;
}

// key rows no state / partial / timer request / unread result holds any more are collected behind a merge
int kr_collect(fw_handle* h) {
    HIP_TRY(launch_kr_collect(h->kr, h->ctrl, h->state, h->state_count, h->sb_nar, h->nw_t, h->ks.n_sb, h->cap_e, h->pwe,
                              2 + h->nw_t, h->parts, h->cap_rows, h->treq, h->out.key, h->sb_out, h->slab_cap,
                              h->treq_cap, h->out_cap, h->stream));
    return FW_OK;
}

int push_key_rows(fw_handle* h, int64_t n, const int64_t* d_off, const uint8_t* d_bytes, const int64_t* ts,
                  const void* const* vals, const uint8_t* const* nulls) {
    int rc = kr_intern(h, n, d_off, d_bytes);
    if (rc) return rc;
    return push(h, n, h->d_kid, ts, h->d_khash, vals, nulls);
}

}  // namespace

// ---- the helpers the checkpoint code shares with this file (fw_handle.h)
int fw::read_ctrl(fw_handle* h, Ctrl* out) {
    HIP_TRY(hipMemcpyAsync(out, h->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (out->error) {
        return fail(FW_E_CAPACITY, "device error (bits 0x%x:%s%s%s%s%s%s%s%s%s)", out->error,
                    out->error & ERR_CHUNKS ? " partial-buffer" : "", out->error & ERR_STATE ? " state-table" : "",
                    out->error & ERR_OUTPUT ? " result-buffer" : "", out->error & ERR_TREQ ? " timer-requests" : "",
                    out->error & ERR_KEYGROUP ? " key-group-not-owned" : "",
                    out->error & ERR_LATE ? " late-rows (call fw_late_records more often)" : "",
                    out->error & ERR_ORDEV ? " first-element-events (call fw_first_element_events after each advance)" : "",
                    out->error & ERR_KEYROW ? " key-rows (table full, or a row over key_row_max_bytes)" : "",
                    out->error & ERR_GAP ? " session-gap (a row's gap outside (0, size_ms])" : "");
    }
    return FW_OK;
}

WinDesc fw::device_win(const fw_handle* h) {
    WinDesc w = h->win;
    if (h->d_tz) {
        const size_t n = h->tz_utc.size();
        w.tz.utc = h->d_tz;
        w.tz.off = h->d_tz + n;
        w.tz.bound = h->d_tz + 2 * n;
    }
    return w;
}

int fw::check_row_words(const fw_handle* h, int32_t row_words, const char* name) {
    const int32_t F = h->cfg.n_value_cols;
    if (row_words == 2 + F) return FW_OK;
    if (!name) return fail(FW_E_INVALID, "row_words %d != 2 + value columns", row_words);
    return fail(FW_E_INVALID, "%s: row_words %d != 2 + value columns (%d record fields)", name, row_words, F);
}

int fw::force_flush(fw_handle* h) {
    int rc = launch_merge(h, INT64_MIN, 1);
    if (rc) return rc;
    h->pushes_ub = 0;
    return FW_OK;
}

int fw::kr_intern(fw_handle* h, int64_t n, const int64_t* d_off, const uint8_t* d_bytes) {
    if (n > h->kr_scratch_n) {
        hipFree(h->d_kid);
        hipFree(h->d_khash);
        h->d_kid = nullptr;
        h->d_khash = nullptr;
        h->kr_scratch_n = 0;
        int rc;
        if ((rc = fd_dalloc(&h->d_kid, (size_t)n))) return rc;
        if ((rc = fd_dalloc(&h->d_khash, (size_t)n))) return rc;
        h->kr_scratch_n = n;
    }
    HIP_TRY(launch_kr_intern(h->kr, h->ctrl, n, d_off, d_bytes, h->d_kid, h->d_khash, h->stream));
    return FW_OK;
}

// ======================================================================================
extern "C" {

const char* fw_last_error(void) { return g_err.c_str(); }
int fw_abi_version(void) { return FW_ABI_VERSION; }

int fw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fw_create(const fw_config* cfg, fw_handle** out) {
    if (!cfg || !out) return fail(FW_E_INVALID, "null argument");
    *out = nullptr;
    fw_handle* h = new fw_handle();
    h->cfg = *cfg;
    if (const char* ab = getenv("FW_ABLATE")) h->ablate = atoi(ab);
    if (const char* fo = getenv("FW_FOLD")) h->fold_always = atoi(fo);
    if (const char* ip = getenv("FW_IG_PACK")) h->ig_pack_mode = std::min(std::max(atoi(ip), 0), 2);
    if (const char* ge = getenv("FW_IGP_GEOM")) h->igp_geom = atoi(ge) != 0;
    if (const char* ak = getenv("FW_AR_KERNEL")) h->ar_kernel = atoi(ak);
    if (const char* fp = getenv("FW_FILL_PCT")) h->fill_pct = std::min(95, std::max(10, atoi(fp)));
    if (const char* si = getenv("FW_SKIP_IDLE")) h->skip_idle = atoi(si) != 0;
    int rc = validate_and_plan(h);
    h->cfg.tz_utc = nullptr;  // the shift-zone table was copied (h->tz_*); never read the caller's
    h->cfg.tz_offset_ms = nullptr;
    if (!rc) rc = allocate(h);
    if (rc) {
        std::string keep = g_err;
        fw_destroy(h);
        g_err = keep;
        return rc;
    }
    *out = h;
    return FW_OK;
}

// the handle's superbuckets by merge path (Tickets::mg_path), after the launches queued so far
static int read_mg_path(fw_handle* h, unsigned long long (&n)[2]) {
    n[0] = n[1] = 0;
    if (!h->tickets || !h->stream) return FW_OK;
    HIP_TRY(hipMemcpyAsync(n, h->tickets->mg_path, sizeof n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return FW_OK;
}

int fw_destroy(fw_handle* h) {
    if (!h) return FW_OK;
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->mg_tag) {
        unsigned long long n[2];
        if (read_mg_path(h, n) == FW_OK) {
            g_mg_path[0].fetch_add((int64_t)n[0], std::memory_order_relaxed);
            g_mg_path[1].fetch_add((int64_t)n[1], std::memory_order_relaxed);
        } else {
            (void)hipGetLastError();
        }
    }
    cw_free(&h->cw);
    sw_free(&h->sw);
    hipFree(h->ctrl);
    hipFree(h->parts);
    hipFree(h->runs);
    hipFree(h->run_ranks);
    hipFree(h->run_fill);
    hipFree(h->run_ovf);
    hipFree(h->slot_fmt);
    hipFree(h->cells);
    hipFree(h->slot_nch);
    hipFree(h->slot_base);
    hipFree(h->ranks);
    hipFree(h->treq);
    if (h->mirror) hipHostFree((void*)h->mirror);
    if (h->ig_mirror) hipHostFree((void*)h->ig_mirror);
    hipFree(h->lfire);
    hipFree(h->side);
    hipFree(h->ordev);
    hipFree(h->kr.slots);
    hipFree(h->kr.arena);
    hipFree(h->kr.mark);
    hipFree(h->kr.free_list);
    hipFree(h->d_kid);
    hipFree(h->d_khash);
    hipFree(h->res_kr_len);
    hipFree(h->res_kr_img);
    for (int b = 0; b < FW_STAGE_BUFS; b++) {
        hipHostFree(h->h_kro[b]);
        hipHostFree(h->h_krb[b]);
    }
    hipFree(h->d_tz);
    hipFree(h->state);
    hipFree(h->state_count);
    hipFree(h->sb_min_timer);
    hipFree(h->sb_nar);
    cols_free(&h->out, false);
    cols_free(&h->res, false);
    hipFree(h->sb_out);
    hipFree(h->sb_fired);
    hipFree(h->coff);
    hipFree(h->chunk_stats);
    hipFree(h->tickets);
    hipFree(h->stamps);
    hipFree(h->kt_dev);
    for (int b = 0; b < FW_STAGE_BUFS; b++) {
        hipHostFree(h->h_key[b]);
        hipHostFree(h->h_ts[b]);
        hipHostFree(h->h_kh[b]);
        for (int v = 0; v < FW_MAX_COLS; v++) {
            hipHostFree(h->h_val[b][v]);
            hipHostFree(h->h_nul[b][v]);
        }
        if (h->stage_ev[b]) hipEventDestroy(h->stage_ev[b]);
        if (h->dstage_free[b]) hipEventDestroy(h->dstage_free[b]);
        hipFree(h->d_kro[b]);
        hipFree(h->d_krb[b]);
        hipFree(h->d_key[b]);
        hipFree(h->d_ts[b]);
        hipFree(h->d_pack[b]);
        hipFree(h->d_kh[b]);
        for (int v = 0; v < FW_MAX_COLS; v++) {
            hipFree(h->d_val[b][v]);
            hipFree(h->d_nul[b][v]);
        }
    }
    if (h->d2h_stream) hipStreamSynchronize(h->d2h_stream);  // an early DMA (ar_kick) may still be reading the buffers
    for (int b = 0; b < FW_AR_BUFS; b++) {
        cols_free(&h->ar[b], true);
        hipHostFree(h->ar_n[b]);
        if (h->ar_ev[b]) hipEventDestroy(h->ar_ev[b]);
        if (h->ar_dma_ev[b]) hipEventDestroy(h->ar_dma_ev[b]);
        cols_free(&h->ard[b], false);
    }
    if (h->d2h_stream) hipStreamDestroy(h->d2h_stream);
    if (h->cstream) hipStreamDestroy(h->cstream);
    delete h->timer;
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return FW_OK;
}

void* fw_get_stream(fw_handle* h) { return h ? (void*)h->stream : nullptr; }

int fw_sync(fw_handle* h) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    Ctrl c;
    return read_ctrl(h, &c);
}

int fw_initialize_watermark(fw_handle* h, int64_t watermark) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    HIP_TRY(hipMemcpyAsync(&h->ctrl->cur, &watermark, sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->host_cur = watermark;
    h->dev_cur = watermark;
    return FW_OK;
}

int fw_reserve(fw_handle* h, int64_t n, fw_host_cols* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    if (n < 0 || n > h->stage_cap) return fail(FW_E_INVALID, "reserve %lld rows > max_batch_rows %lld", (long long)n, (long long)h->stage_cap);
    int rc = alloc_staging(h);
    if (rc) return rc;
    const int b = h->stage_cur;
    HIP_TRY(hipEventSynchronize(h->stage_ev[b]));  // previous H2D from this buffer has finished
    memset(out, 0, sizeof *out);
    out->key = h->h_key[b];
    out->ts = h->h_ts[b];
    out->key_hash = h->h_kh[b];
    for (int v = 0; v < h->cfg.n_value_cols; v++) {
        out->values[v] = h->h_val[b][v];
        out->nulls[v] = h->h_nul[b][v];
    }
    if (h->keyrow) {
        out->key_row_offsets = h->h_kro[b];
        out->key_row_bytes = h->h_krb[b];
        out->key_row_bytes_cap = h->krb_cap;
        h->h_kro[b][0] = 0;
    }
    h->reserved = n;
    return FW_OK;
}

static int commit_impl(fw_handle* h, int64_t n, uint32_t packed, const int64_t* bases);

int fw_commit(fw_handle* h, int64_t n) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    return commit_impl(h, n, 0u, nullptr);
}

// the loop vectorises; the wider x86 units where the host has them (chosen at load time)
__attribute__((target_clones("avx512f", "avx2", "default")))
int fw_delta32_encode(const int64_t* src, int64_t n, int64_t base, uint32_t* dst) {
    if (n <= 0) return 0;
    uint64_t out = 0;  // any high bits: a value outside the column's 2^32 window
    for (int64_t i = 0; i < n; i++) {
        const uint64_t d = (uint64_t)src[i] - (uint64_t)base;
        out |= d >> 32;
        dst[i] = (uint32_t)d;
    }
    return out ? 1 : 0;
}

int fw_commit_delta32(fw_handle* h, int64_t n, uint32_t delta_cols, const int64_t* bases) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    const uint32_t valid = FW_DELTA_KEY | FW_DELTA_TS | (((1u << h->cfg.n_value_cols) - 1u) << 2);
    if (delta_cols & ~valid) return fail(FW_E_INVALID, "delta_cols 0x%x names a column the operator does not have", delta_cols);
    if ((delta_cols & FW_DELTA_KEY) && h->keyrow) return fail(FW_E_INVALID, "key-row operators have no key column to pack");
    if (delta_cols && !bases) return fail(FW_E_INVALID, "packed columns need their bases");
    return commit_impl(h, n, delta_cols, bases);
}

static int commit_impl(fw_handle* h, int64_t n, uint32_t packed, const int64_t* bases) {
    ar_kick(h);
    if (h->reserved < 0 || n > h->reserved || n < 0) return fail(FW_E_STATE, "commit without matching reserve");
    h->reserved = -1;
    const int b = h->stage_cur;
    h->stage_cur = (b + 1) % FW_STAGE_BUFS;
    if (n == 0) return FW_OK;
    int64_t krb_n = 0;
    if (h->keyrow) {
        krb_n = h->h_kro[b][n];
        if (h->h_kro[b][0] != 0 || krb_n < 0 || krb_n > h->krb_cap)
            return fail(FW_E_INVALID, "key row offsets must start at 0 and end within key_row_bytes_cap");
    }
    // H2D on the copy stream into device buffer b, once the ingest that last read it has run; the
    // operator stream waits for the copies.  The previous batch's ingest and merge overlap them.
    hipStream_t cs = h->cstream;
    HIP_TRY(hipStreamWaitEvent(cs, h->dstage_free[b], 0));
    // (a second copy stream for the upper half of every column was measured slower: CFG2 end to end
    // 1.76 -> 1.26 G ev/s, its enqueue blocking the host 0.9 ms per batch)
    auto h2d = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs);
    };
    if (packed && !h->d_pack[b]) {  // first packed commit into this set (allocation outside any timed loop of the caller's)
        h->pack_stride = (h->stage_cap + 3) & ~3ll;
        HIP_TRY(hipMalloc((void**)&h->d_pack[b], (size_t)FW_PACK_COLS * h->pack_stride * 4));
    }
    // an 8-byte word column: a packed one crosses PCIe as n 32-bit deltas (the first 4n bytes of its
    // staging column) and is widened on the copy stream, behind its copy
    WidenArgs wa{};
    wa.n = n;
    int nw = 0;
    auto col = [&](int slot, void* dst, const void* src) -> hipError_t {
        if (!((packed >> slot) & 1u)) return h2d(dst, src, (size_t)n * 8);
        uint32_t* p = h->d_pack[b] + (size_t)slot * h->pack_stride;
        wa.src[nw] = p;
        wa.dst[nw] = (uint64_t*)dst;
        wa.base[nw] = (uint64_t)bases[slot];
        nw++;
        return h2d(p, src, (size_t)n * 4);
    };
    if (h->keyrow) {
        HIP_TRY(h2d(h->d_kro[b], h->h_kro[b], (n + 1) * 8));
        HIP_TRY(h2d(h->d_krb[b], h->h_krb[b], (size_t)krb_n));
    } else {
        HIP_TRY(col(0, h->d_key[b], h->h_key[b]));
    }
    HIP_TRY(col(1, h->d_ts[b], h->h_ts[b]));
    if (h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED) HIP_TRY(h2d(h->d_kh[b], h->h_kh[b], n * 4));
    for (int s = 0; s < h->nv; s++) {
        const int v = h->slot_col[s];
        HIP_TRY(col(2 + v, h->d_val[b][v], h->h_val[b][v]));
        if (h->d_nul[b][v]) HIP_TRY(h2d(h->d_nul[b][v], h->h_nul[b][v], n));
    }
    HIP_TRY(launch_widen(wa, nw, cs));
    HIP_TRY(hipEventRecord(h->stage_ev[b], cs));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->stage_ev[b], 0));
    const void* vals[FW_MAX_COLS];
    const uint8_t* nuls[FW_MAX_COLS];
    for (int v = 0; v < FW_MAX_COLS; v++) {
        vals[v] = h->d_val[b][v];
        nuls[v] = h->d_nul[b][v];
    }
    const int rc = h->cw.on  ? cw_push(&h->cw, n, h->d_key[b], h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED ? h->d_kh[b] : nullptr,
                                       (const uint64_t*)vals[h->slot_col[0]])
                   : h->sw.on ? sw_push(&h->sw, h->host_cur, n, h->d_key[b], h->d_ts[b],
                                        h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED ? h->d_kh[b] : nullptr, vals, nuls)
                   : h->keyrow ? push_key_rows(h, n, h->d_kro[b], h->d_krb[b], h->d_ts[b], vals, nuls)
                             : push(h, n, h->d_key[b], h->d_ts[b],
                                    h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED ? h->d_kh[b] : nullptr, vals, nuls);
    HIP_TRY(hipEventRecord(h->dstage_free[b], h->stream));
    return rc;
}

// ---- the push entry points' argument checks: each returns FW_OK or the refusal
static int check_segments(int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts) {
    if (n_segs < 0 || seg_len < 1 || (n_segs > 0 && !d_seg_counts)) return fail(FW_E_INVALID, "bad segments");
    return FW_OK;
}
static int check_key_hash(const fw_handle* h, const int32_t* d_key_hash) {
    if (h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED && !d_key_hash) return fail(FW_E_INVALID, "key_hash column required");
    return FW_OK;
}
static int fail_value_null(int v) { return fail(FW_E_INVALID, "value column %d is NULL", v); }
// every value column the plan loads, and the null-flag column of each NULL-able one
static int check_value_cols(const fw_handle* h, const void* const* d_values, const uint8_t* const* d_nulls) {
    if (h->nv > 0 && !d_values) return fail(FW_E_INVALID, "value columns required");
    for (int s = 0; s < h->nv; s++) {
        const int v = h->slot_col[s];
        if (!d_values[v]) return fail_value_null(v);
        if (((h->cfg.nullable_cols >> v) & 1u) && (!d_nulls || !d_nulls[v]))
            return fail(FW_E_INVALID, "nullable value column %d needs its null-flag column", v);
    }
    return FW_OK;
}
// a count handle numbers the rows of a segment push by buffer position
static int check_ordinals(int32_t n_segs, int64_t seg_len) {
    if (seg_len >= (1ll << 32) || (int64_t)n_segs * seg_len >= (1ll << 32))
        return fail(FW_E_INVALID, "arrival ordinals need n_segs * seg_len < 2^32 rows per call");
    return FW_OK;
}
#define CHECK(call) \
    if (int rc_ = (call)) return rc_

int fw_push_device_key_rows(fw_handle* h, int64_t n, const int64_t* d_key_row_offsets, const uint8_t* d_key_row_bytes,
                            const int64_t* d_ts, const void* const* d_values, const uint8_t* const* d_nulls) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_REFUSE(h, "fw_push_device_key_rows");
    if (!h->keyrow) return fail(FW_E_INVALID, "fw_push_device_key_rows needs a FW_KEYHASH_KEYROW operator");
    if (n < 0) return fail(FW_E_INVALID, "negative n");
    if (n == 0) return FW_OK;
    if (!d_key_row_offsets || !d_key_row_bytes || !d_ts) return fail(FW_E_INVALID, "null key row / ts column");
    CHECK(check_value_cols(h, d_values, d_nulls));
    return push_key_rows(h, n, d_key_row_offsets, d_key_row_bytes, d_ts, d_values, d_nulls);
}

int fw_push_device(fw_handle* h, int64_t n, const int64_t* d_key, const int64_t* d_ts, const int32_t* d_key_hash,
                   const void* const* d_values, const uint8_t* const* d_nulls) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    if (n < 0) return fail(FW_E_INVALID, "negative n");
    ar_kick(h);
    if (n == 0) return FW_OK;
    if (h->cw.on) {  // count windows ignore the ts column (d_ts may be NULL)
        if (!d_key) return fail(FW_E_INVALID, "null key column");
        CHECK(check_key_hash(h, d_key_hash));
        if (h->nv > 0 && (!d_values || !d_values[h->slot_col[0]])) return fail_value_null(h->slot_col[0]);
        return cw_push(&h->cw, n, d_key, d_key_hash, h->nv > 0 ? (const uint64_t*)d_values[h->slot_col[0]] : nullptr);
    }
    if (!d_key || !d_ts) return fail(FW_E_INVALID, "null key/ts column");
    if (h->sw.on) {  // session windows: folded into the state now, under the current watermark
        CHECK(check_key_hash(h, d_key_hash));
        CHECK(check_value_cols(h, d_values, d_nulls));
        return sw_push(&h->sw, h->host_cur, n, d_key, d_ts, d_key_hash, d_values, d_nulls);
    }
    if (h->keyrow) return fail(FW_E_INVALID, "a FW_KEYHASH_KEYROW operator takes key rows (fw_push_device_key_rows)");
    CHECK(check_key_hash(h, d_key_hash));
    CHECK(check_value_cols(h, d_values, d_nulls));
    return push(h, n, d_key, d_ts, d_key_hash, d_values, d_nulls);
}

int fw_push_device_segments(fw_handle* h, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts,
                            const int64_t* d_key, const int64_t* d_ts, const int32_t* d_key_hash,
                            const void* const* d_values, const uint8_t* const* d_nulls) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_REFUSE_EXCHANGE(h, "fw_push_device_segments");
    CHECK(check_segments(n_segs, seg_len, d_seg_counts));
    if (h->keyrow) return fail(FW_E_INVALID, "a FW_KEYHASH_KEYROW operator takes key rows (fw_push_device_key_rows)");
    const int64_t n = (int64_t)n_segs * seg_len;
    if (n == 0) return FW_OK;
    if (!d_key || !d_ts) return fail(FW_E_INVALID, "null key/ts column");
    CHECK(check_key_hash(h, d_key_hash));
    CHECK(check_value_cols(h, d_values, d_nulls));
    if (h->sw.on) {  // folded now, under Ctrl::cur at this point of the stream
        ar_kick(h);
        return sw_push_segments(&h->sw, n_segs, seg_len, d_seg_counts, d_key, d_ts, 1, d_key_hash, d_values, d_nulls);
    }
    return push(h, n, d_key, d_ts, d_key_hash, d_values, d_nulls, d_seg_counts, seg_len);
}

int fw_push_device_packed_segments(fw_handle* h, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts,
                                   const int64_t* d_rows, int32_t row_words) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_REFUSE_EXCHANGE(h, "fw_push_device_packed_segments");
    CHECK(check_segments(n_segs, seg_len, d_seg_counts));
    CHECK(check_row_words(h, row_words, nullptr));
    if (h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED || h->keyrow || h->cfg.nullable_cols)
        return fail(FW_E_INVALID, "packed rows carry no key-hash, key-row or null-flag columns");
    const int64_t n = (int64_t)n_segs * seg_len;
    if (n == 0) return FW_OK;
    if (!d_rows) return fail(FW_E_INVALID, "null rows");
    const void* vals[FW_MAX_COLS] = {nullptr};
    for (int c = 0; c < h->cfg.n_value_cols; c++) vals[c] = d_rows + 2 + c;
    if (h->sw.on) {
        ar_kick(h);
        return sw_push_segments(&h->sw, n_segs, seg_len, d_seg_counts, d_rows, d_rows + 1, row_words, nullptr, vals, nullptr);
    }
    return push(h, n, d_rows, d_rows + 1, nullptr, vals, nullptr, d_seg_counts, seg_len, row_words);
}

// The count handle's own segment pushes: count rows have no timestamp, so the two entries above keep
// refusing them.  Only a count handle of parallelism > 1 has an exchange in front of it.
#define CW_ONLY_EXCHANGE(h, name)                                                                                  \
    if ((h)->sw.on) return fail(FW_E_INVALID, name ": not for session windows (count windows only)");              \
    CW_REFUSE_RECORD(h, name);                                                                                     \
    if (!(h)->cw.on) return fail(FW_E_INVALID, name ": not for time windows (count windows only)");                \
    if ((h)->cfg.parallelism <= 1)                                                                                 \
        return fail(FW_E_INVALID, name ": a count handle of parallelism 1 has no keyBy exchange in front of it")

int fw_push_device_count_segments(fw_handle* h, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts,
                                  const int64_t* d_key, const int32_t* d_key_hash, const void* d_value) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_ONLY_EXCHANGE(h, "fw_push_device_count_segments");
    CHECK(check_segments(n_segs, seg_len, d_seg_counts));
    CHECK(check_ordinals(n_segs, seg_len));
    if (n_segs == 0) return FW_OK;
    if (!d_key) return fail(FW_E_INVALID, "null key column");
    CHECK(check_key_hash(h, d_key_hash));
    if (h->nv > 0 && !d_value) return fail_value_null(h->slot_col[0]);
    return cw_push_segments(&h->cw, n_segs, seg_len, d_seg_counts, d_key,
                            h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED ? d_key_hash : nullptr,
                            h->nv > 0 ? (const uint64_t*)d_value : nullptr, 1);
}

int fw_push_device_count_packed_segments(fw_handle* h, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts,
                                         const int64_t* d_rows, int32_t row_words) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_ONLY_EXCHANGE(h, "fw_push_device_count_packed_segments");
    CHECK(check_segments(n_segs, seg_len, d_seg_counts));
    CHECK(check_row_words(h, row_words, nullptr));
    if (h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED) return fail(FW_E_INVALID, "packed rows carry no key-hash column");
    CHECK(check_ordinals(n_segs, seg_len));
    if (n_segs == 0) return FW_OK;
    if (!d_rows) return fail(FW_E_INVALID, "null rows");
    // (key, ts, value): word 1 is not read; a count aggregate reads no value word either
    return cw_push_segments(&h->cw, n_segs, seg_len, d_seg_counts, d_rows, nullptr, (const uint64_t*)d_rows + 2, row_words);
}

int fw_push_device_count_record_packed_segments(fw_handle* h, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts,
                                                const int64_t* d_rows, int32_t row_words) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_ONLY_RECORD_EXCHANGE(h, "fw_push_device_count_record_packed_segments");
    CHECK(check_segments(n_segs, seg_len, d_seg_counts));
    CHECK(check_row_words(h, row_words, "fw_push_device_count_record_packed_segments"));
    if (h->cfg.key_hash == FW_KEYHASH_PRECOMPUTED)
        return fail(FW_E_INVALID, "fw_push_device_count_record_packed_segments: packed rows carry no key-hash column");
    if (seg_len > h->cfg.max_batch_rows)  // (keeps n_segs * seg_len in range below)
        return fail(FW_E_INVALID, "fw_push_device_count_record_packed_segments: seg_len = %lld exceeds max_batch_rows (%lld)",
                    (long long)seg_len, (long long)h->cfg.max_batch_rows);
    if (n_segs == 0) return FW_OK;
    if (!d_rows) return fail(FW_E_INVALID, "null rows");
    // (key, unread word, the record's fields): the aggregated field is word 2 + input_col
    return cw_push_record_segments(&h->cw, n_segs, seg_len, d_seg_counts, d_rows, row_words);
}

int fw_advance(fw_handle* h, int64_t watermark) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    if (h->cw.on) {  // CountTrigger.onEventTime: CONTINUE -- the watermark is recorded, nothing fires
        if (watermark > h->host_cur) h->host_cur = watermark;
        h->cw.watermark = h->host_cur;
        return FW_OK;
    }
    if (h->sw.on) {  // EventTimeTrigger: every session with end - 1 <= watermark fires; W' <= W changes nothing
        // once advanced from the device the host's mirror is only a lower bound of Ctrl::cur: the
        // device takes the maximum
        if (h->sw.wm_dev) return sw_advance_device(&h->sw, nullptr, watermark);
        if (watermark <= h->host_cur) return FW_OK;
        const int64_t prev = h->host_cur;  // (lateness: the sessions with a timer at or below it have fired)
        h->host_cur = watermark;
        HIP_TRY(hipMemcpyAsync(&h->ctrl->cur, &h->host_cur, sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        return sw_advance(&h->sw, watermark, prev);
    }
    ar_kick(h);
    // A SQL watermark below the next trigger watermark crosses no slice end: no window fires, no
    // buffer flush is due (AbstractSliceSyncStateWindowAggProcessor.advanceProgress :139-153 only
    // flushes at a trigger) and lateness is unchanged (no window end lies between the old and the
    // new watermark), so the merge launch would only move currentProgress.  It is skipped; the next
    // launch moves currentProgress past it and registers any pending late-record timers before it
    // fires.  DataStream cleanup timers are off the slice grid (cleanupTime), so DataStream and
    // key-row operators (whose collector runs with the merge) always launch.
    // The trigger grid is the slice-end grid only in UTC with an offset on the grid: otherwise a
    // timer or a lateness bound can lie between two trigger watermarks, and only a repeated
    // watermark is skipped.
    const bool on_grid = h->win.tz.n == 0 && h->win.offset % h->win.interval == 0;
    if (h->skip_idle && !h->always_flush && !h->keyrow &&
        (watermark <= h->dev_cur || (on_grid && watermark < h->dev_ntp))) {
        if (watermark > h->host_cur) h->host_cur = watermark;
        return FW_OK;
    }
    int rc = launch_merge(h, watermark, 0);
    if (rc) return rc;
    if (h->keyrow && (rc = kr_collect(h))) return rc;
    if (watermark > h->host_cur) h->host_cur = watermark;
    return FW_OK;
}

int fw_advance_device(fw_handle* h, const int64_t* d_watermark) {
    if (!h || !d_watermark) return fail(FW_E_INVALID, "null argument");
    if (h->sw.on) {
        // parallelism 1: no exchange, no device valve; the fold takes its watermark from the host
        if (h->cfg.parallelism <= 1)
            return fail(FW_E_INVALID, "fw_advance_device: not for session windows (the late test needs the watermark on the host)");
        // parallelism > 1: Ctrl::cur becomes the watermark of record (W' = max(cur, *d_watermark));
        // two stream-ordered launches, no host wait
        return sw_advance_device(&h->sw, d_watermark, INT64_MIN);
    }
    if (h->cw.on) {  // recorded on the device (fw_stats.current_watermark), nothing fires
        HIP_TRY(hipMemcpyAsync(&h->ctrl->cur, d_watermark, sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream));
        return FW_OK;
    }
    int rc = launch_merge(h, INT64_MIN, 0, d_watermark);
    if (rc) return rc;
    return h->keyrow ? kr_collect(h) : FW_OK;
}

int fw_flush(fw_handle* h) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    if (h->cw.on || h->sw.on) return FW_OK;  // every push is folded into the state when it is pushed
    return force_flush(h);
}

int fw_get_stats(fw_handle* h, fw_stats* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    if (h->cw.on) {
        Ctrl cc;
        HIP_TRY(hipMemcpyAsync(&cc, h->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        memset(out, 0, sizeof *out);
        out->current_watermark = std::max<int64_t>(cc.cur, h->host_cur);
        out->next_trigger_progress = INT64_MAX;  // no watermark triggers a count window
        out->live_state_entries = cc.live_entries;  // keys in the table
        out->results_available = std::min<int64_t>((int64_t)cc.out_count[0], h->cw.out_cap);
        out->num_fired_windows = (int64_t)cc.fired;
        out->error_flags = (int32_t)cc.error;
        out->num_superbuckets = h->ks.n_sb;
        out->superbucket_capacity = h->cw.cap_e;
        return FW_OK;
    }
    if (h->sw.on) {
        Ctrl cc;
        HIP_TRY(hipMemcpyAsync(&cc, h->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        memset(out, 0, sizeof *out);
        if (h->sw.wm_dev) h->host_cur = cc.cur;  // the watermark of record, behind the synchronisation above
        out->current_watermark = h->host_cur;
        out->next_trigger_progress = INT64_MAX;
        out->num_late_records_dropped = (int64_t)cc.late_dropped;
        out->live_state_entries = cc.live_entries;  // live sessions
        out->results_available = std::min<int64_t>((int64_t)cc.out_count[0], h->sw.out_cap);
        out->num_fired_windows = (int64_t)cc.fired;
        out->error_flags = (int32_t)cc.error;
        out->num_superbuckets = h->ks.n_sb;
        out->superbucket_capacity = h->sw.cap_s;
        return FW_OK;
    }
    Ctrl c;
    const int nsb = h->ks.n_sb;
    std::vector<int32_t> cnt(nsb), sbo(nsb);
    std::vector<uint32_t> fired(nsb);
    HIP_TRY(hipMemcpyAsync(&c, h->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(cnt.data(), h->state_count, 4ll * nsb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(sbo.data(), h->sb_out, 4ll * nsb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(fired.data(), h->sb_fired, 4ll * nsb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int64_t live = 0, avail = std::min<int64_t>((int64_t)c.out_count[c.ovf_sel & 1], h->out_cap), nf = (int64_t)c.fired;
    for (int s = 0; s < nsb; s++) {
        live += cnt[s];
        avail += sbo[s];
        nf += fired[s];
    }
    if (h->reset_pending) avail = 0;
    memset(out, 0, sizeof *out);
    out->current_watermark = std::max<int64_t>(c.cur, h->host_cur);  // skipped idle advances included
    out->next_trigger_progress = c.ntp;
    out->num_late_records_dropped = (int64_t)c.late_dropped;
    out->live_state_entries = live;
    out->pending_rows = (int64_t)c.pending_rows;
    out->results_available = avail;
    out->num_fired_windows = nf;
    out->partials_emitted = (int64_t)c.partials;
    out->error_flags = (int32_t)c.error;
    out->num_superbuckets = h->ks.n_sb;
    out->flush_launches = (int64_t)c.flush_launches;
    out->partials_merged = (int64_t)c.parts_merged;
    out->state_entries_moved = (int64_t)c.state_moved;
    out->partial_bytes_written = (int64_t)c.part_bytes;
    out->partial_bytes_merged = (int64_t)c.part_bytes_merged;
    out->compact_chunks = (int64_t)c.compact_chunks;
    out->peak_superbucket_entries = (int64_t)c.peak_entries;
    out->superbucket_capacity = h->cap_e;
    out->key_rows = h->keyrow ? std::min(c.kr_next_id, h->kr.cap_ids) - std::max<int64_t>(0, c.kr_free_count - std::min(c.kr_free_cursor, c.kr_free_count)) : 0;
    out->key_row_collections = c.kr_collections;
    return FW_OK;
}

int fw_set_profiling(fw_handle* h, int enable) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_REFUSE(h, "fw_set_profiling");
    HIP_TRY(hipStreamSynchronize(h->stream));
    delete h->timer;
    h->timer = nullptr;
    h->kt_device = enable == FW_PROF_DEVICE;
    HIP_TRY(hipMemsetAsync(h->kt_dev, 0, sizeof(unsigned long long) * FW_KT_N * KT_WORDS, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (enable == FW_PROF_EVENTS || enable == FW_PROF_EVENTS_ALL) {
        EvTimer* t = new EvTimer();
        t->all = enable == FW_PROF_EVENTS_ALL;
        h->timer = t;
    } else if (enable && enable != FW_PROF_DEVICE) {
        return fail(FW_E_INVALID, "bad profiling mode %d", enable);
    }
    return FW_OK;
}

int64_t fw_ingest_pack_launches(fw_handle* h) {
    return h ? h->ig_pack_launches : g_ig_pack_launches.load(std::memory_order_relaxed);
}

int fw_ingest_pack_geometry(fw_handle* h, int32_t* geom, int32_t* threads, int32_t* rows_per_thread, int32_t* workgroups_per_cu) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int g = h->igp_geom >= 0 ? h->igp_geom : h->igp_last;
    if (geom) *geom = g;
    if (threads) *threads = g ? IGP_BLOCK1 : IGP_BLOCK;
    if (rows_per_thread) *rows_per_thread = g ? IGP_RPT1 : IGP_RPT;
    if (workgroups_per_cu) {
        const int n = ingest_pack_occupancy(g);
        if (n < 0) return fail(FW_E_DEVICE, "k_ingest_pack occupancy query: %s", hipGetErrorString((hipError_t)-n));
        *workgroups_per_cu = n;
    }
    return FW_OK;
}

int64_t fw_merge_path_superbuckets(fw_handle* h, int tag_path) {
    const int i = tag_path ? 1 : 0;
    if (!h) return g_mg_path[i].load(std::memory_order_relaxed);
    unsigned long long n[2];
    if (read_mg_path(h, n) != FW_OK) return -1;
    return (int64_t)n[i];
}

int fw_get_kernel_times(fw_handle* h, fw_kernel_times* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_get_kernel_times");
    memset(out, 0, sizeof *out);
    unsigned long long st[N_STAMPS];
    HIP_TRY(hipMemcpyAsync(st, h->stamps, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < N_STAMPS && k < FW_KT_N; k++) out->merge_phase_cycles[k] = (int64_t)st[k];
    if (h->ablate & AB_GSTAMPS)  // diagnostic builds only: thread 0's gather parts
        fprintf(stderr, "gather_parts cells=%llu scan=%llu loads=%llu probe=%llu fold+insert=%llu seq_miss=%llu\n", st[13],
                st[14], st[2], st[4], st[7], st[15]);
    if (h->ablate & AB_GSTAMPS)  // wave 0's rows: live / home empty / undecided / slow path, slow-path rounds
        fprintf(stderr, "gather_rows live=%llu fresh=%llu undecided=%llu slow=%llu slow_rounds=%llu\n", st[8], st[9], st[10],
                st[11], st[12]);
    if (h->ablate & AB_FSTAMPS)  // diagnostic builds only: per-lane cycles of fire_one's parts
        fprintf(stderr, "fire_parts probe+merge=%llu emit=%llu expire+next=%llu claim=%llu windows=%llu\n", st[8], st[9],
                st[10], st[11], st[12]);
    if (h->kt_device) {
        unsigned long long kt[FW_KT_N * KT_WORDS];
        HIP_TRY(hipMemcpyAsync(kt, h->kt_dev, sizeof kt, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        int khz = 0;  // rate of the constant device clock wall_clock64() counts
        HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device));
        for (int k = 0; k < FW_KT_N; k++) {
            out->ms[k] = khz > 0 ? (double)kt[k * KT_WORDS + 1] / (double)khz : 0.0;
            out->launches[k] = (int64_t)kt[k * KT_WORDS + 2];
        }
        return FW_OK;
    }
    if (!h->timer) return FW_OK;
    EvTimer* t = static_cast<EvTimer*>(h->timer);
    HIP_TRY(t->resolve());
    for (int k = 0; k < FW_KT_N; k++) {
        out->ms[k] = t->ms[k];
        out->launches[k] = t->n[k];
    }
    return FW_OK;
}

// ---- host-side restatements (the exact code the kernels run), for host partitioners/tests
int32_t fw_host_key_group(int32_t key_hash_kind, int64_t key, int32_t precomputed_hash, int32_t max_parallelism) {
    return key_group_for_hash(java_key_hash(key_hash_kind, key, precomputed_hash), max_parallelism);
}
int fw_host_assign_key_groups(const int64_t* key, const int32_t* key_hash, int64_t n, int32_t key_hash_kind,
                              int32_t max_parallelism, int32_t parallelism, int32_t* kg, int32_t* dest) {
    if (n < 0 || (n > 0 && !key) || max_parallelism <= 0 || parallelism <= 0 || parallelism > max_parallelism)
        return fail(FW_E_INVALID, "fw_host_assign_key_groups: bad arguments");
    for (int64_t i = 0; i < n; i++) {
        const int32_t g = key_group_for_hash(java_key_hash(key_hash_kind, key[i], key_hash ? key_hash[i] : 0), max_parallelism);
        if (kg) kg[i] = g;
        if (dest) dest[i] = operator_for_key_group(max_parallelism, parallelism, g);
    }
    return FW_OK;
}
int64_t fw_host_window_start(int64_t ts, int64_t offset, int64_t size) {
    return window_start(ts, offset, make_udiv((uint64_t)size));
}
int64_t fw_host_next_trigger_watermark(int64_t wm, int64_t interval) {
    return next_trigger_watermark(wm, make_udiv((uint64_t)interval));
}

// Which ingest kernel takes a push (pure; push() above is its only caller beside the tests).
// k_ingest_pack never folds, so k_ingest keeps every push on which something has to be folded or
// measured: while fold_skip is clear or no PF_PACK fields are valid, while no flush has opened an
// epoch that could carry such fields (the packing kernel would send every chunk the slow way), and
// once in FW_IG_REFRESH pushes -- once in FW_IG_REFRESH_SKEW while the packing kernel's own sampled
// estimate (IGM_SKEW) says the stream folds -- on which it is told to fold whatever
// Ctrl::push_count is, so that fold_skip is measured again.
int32_t fw_host_ig_pack_choice(int32_t mode, uint64_t mirror, uint64_t pushes_since_fold, uint64_t merge_launches,
                               uint32_t ineligible) {
    if (mode <= 0 || (ineligible & ~(uint32_t)FW_IGX_FOLD_ALWAYS)) return FW_IG_INGEST;
    if (mode >= 2) return FW_IG_PACK;
    if (ineligible & FW_IGX_FOLD_ALWAYS) return FW_IG_INGEST;  // (folds on every push as it is)
    if (mirror == ~0ull || !(mirror & IGM_FOLD_SKIP) || !(mirror & IGM_PK_OK)) return FW_IG_INGEST;
    if (merge_launches == 0) return FW_IG_INGEST;
    if (pushes_since_fold >= (uint64_t)((mirror & IGM_SKEW) ? FW_IG_REFRESH_SKEW : FW_IG_REFRESH)) return FW_IG_FOLD;
    return FW_IG_PACK;
}

int fw_host_time_op(const fw_config* cfg, int32_t what, int64_t x, int64_t* out) {
    if (!cfg || !out) return fail(FW_E_INVALID, "null argument");
    fw_handle h;
    h.cfg = *cfg;
    const int rc = validate_and_plan(&h);  // host-only planning; w.tz points at h's host copy
    if (rc) return rc;
    CW_REFUSE(&h, "fw_host_time_op");
    const WinDesc& w = h.win;
    switch (what) {
        case 0: *out = tz_to_utc_ts(w.tz, x); break;
        case 1: *out = tz_epoch_for_timer(w.tz, x); break;
        case 2: *out = tz_next_trigger_watermark(w.tz, x, w.slice_div); break;
        case 3: *out = slice_end_of(w, tz_to_utc_ts(w.tz, x)); break;
        case 4: *out = window_start_of(w, x); break;
        default: return fail(FW_E_INVALID, "bad time op %d", what);
    }
    return FW_OK;
}


int fw_host_count_step(const fw_config* cfg, int64_t index, int64_t* slice, int32_t* ring_slot, int32_t* fires,
                       int64_t* window_start, int32_t* n_slices) {
    if (!cfg || !slice || !ring_slot || !fires || !window_start || !n_slices) return fail(FW_E_INVALID, "null argument");
    if (cfg->window_kind != FW_WIN_COUNT && cfg->window_kind != FW_WIN_COUNT_RECORD)
        return fail(FW_E_INVALID, "fw_host_count_step needs a FW_WIN_COUNT configuration (or FW_WIN_COUNT_RECORD)");
    if (index < 0) return fail(FW_E_INVALID, "negative element index");
    fw_handle h;
    h.cfg = *cfg;
    const int rc = validate_and_plan(&h);
    if (rc) return rc;
    count_step(h.cw.d, index, slice, ring_slot, fires, window_start, n_slices);
    return FW_OK;
}

int fw_host_count_record_fold(const fw_config* cfg, int64_t a_val, int64_t a_ord, int64_t b_val, int64_t b_ord, int64_t* out_val,
                              int64_t* out_ord) {
    if (!cfg || !out_val || !out_ord) return fail(FW_E_INVALID, "null argument");
    if (cfg->window_kind != FW_WIN_COUNT_RECORD) return fail(FW_E_INVALID, "fw_host_count_record_fold needs a FW_WIN_COUNT_RECORD configuration");
    fw_handle h;
    h.cfg = *cfg;
    const int rc = validate_and_plan(&h);
    if (rc) return rc;
    const CountOp& w = h.cw;
    uint64_t v, o;
    count_record_fold(w.d.op, w.mode, w.vtype == FW_T_F64, (uint64_t)a_val, (uint64_t)a_ord, (uint64_t)b_val, (uint64_t)b_ord, &v, &o);
    if (w.vtype == FW_T_I32 && w.d.op == CW_ADD_I) v = (uint64_t)(int64_t)(int32_t)(uint32_t)v;  // as a result row carries it
    *out_val = (int64_t)v;
    *out_ord = (int64_t)o;
    return FW_OK;
}

// One session list, one element: the body of the four fw_host_session_add* entry points.  `kind` is the
// window kind the entry point accepts (kind_name in the messages) and `name` its own name; `gap` is the
// caller's gap (the dynamic kinds) or null for the configuration's; `fired_index` is given by the
// lateness kinds, which run session_add<1, true>.  (Only FW_WIN_SESSION plans a SQL configuration.)
static int host_session_add(int32_t kind, const char* kind_name, const char* name, const fw_config* cfg, int64_t watermark, int64_t ts,
                            const int64_t* gap, int64_t value, int64_t* starts, int64_t* ends, int64_t* accs, int32_t* n,
                            int32_t capacity, int32_t* outcome, int32_t* fired_index) {
    if (!cfg || !n || !outcome || (capacity > 0 && (!starts || !ends || !accs))) return fail(FW_E_INVALID, "null argument");
    if (cfg->window_kind != kind) return fail(FW_E_INVALID, "%s needs a %s configuration", name, kind_name);
    fw_handle h;
    h.cfg = *cfg;
    const int rc = validate_and_plan(&h);
    if (rc) return rc;
    const SessionDesc& d = h.sw.d;
    if (d.sql) return fail(FW_E_INVALID, "%s needs a DataStream session configuration (SQL: fw_host_sql_session_add)", name);
    if (gap && (*gap < 1 || *gap > d.gap))
        return fail(FW_E_INVALID, "session gap %lld is outside (0, size_ms = %lld]", (long long)*gap, (long long)d.gap);
    if (*n < 0 || *n > capacity) return fail(FW_E_INVALID, "bad session count %d (capacity %d)", *n, capacity);
    for (int32_t i = 0; i < *n; i++) accs[i] = (int64_t)session_word_of_result(d, (uint64_t)accs[i]);
    const uint64_t word = session_word(d, (uint64_t)value);
    const int64_t g = gap ? *gap : d.gap;
    int32_t at = -1;
    const int r = fired_index ? session_add<1, true>(g, d.ops, watermark, ts, &word, 1, starts, ends, (uint64_t*)accs, 1, 1, n, capacity,
                                                     h.sw.lateness, &at)
                              : session_add<1>(g, d.ops, watermark, ts, &word, 1, starts, ends, (uint64_t*)accs, 1, 1, n, capacity);
    for (int32_t i = 0; i < *n; i++) accs[i] = (int64_t)session_result(d, (uint64_t)accs[i]);
    if (r < 0) return fail(FW_E_CAPACITY, "the session list is full (%d sessions)", capacity);
    *outcome = r;
    // EventTimeTrigger.onElement: the session the element produced fires at once if its timer has passed
    // (with a dynamic gap: recalled, parity unpinned)
    if (fired_index) *fired_index = r == 1 && session_due(ends[at], watermark) ? at : -1;
    return FW_OK;
}

int fw_host_session_add(const fw_config* cfg, int64_t watermark, int64_t ts, int64_t value, int64_t* starts, int64_t* ends,
                        int64_t* accs, int32_t* n, int32_t capacity, int32_t* outcome) {
    return host_session_add(FW_WIN_SESSION, "FW_WIN_SESSION", "fw_host_session_add", cfg, watermark, ts, nullptr, value, starts, ends,
                            accs, n, capacity, outcome, nullptr);
}

int fw_host_session_add_late(const fw_config* cfg, int64_t watermark, int64_t ts, int64_t value, int64_t* starts, int64_t* ends,
                             int64_t* accs, int32_t* n, int32_t capacity, int32_t* outcome, int32_t* fired_index) {
    if (!fired_index) return fail(FW_E_INVALID, "null argument");
    return host_session_add(FW_WIN_SESSION_LATENESS, "FW_WIN_SESSION_LATENESS", "fw_host_session_add_late", cfg, watermark, ts, nullptr,
                            value, starts, ends, accs, n, capacity, outcome, fired_index);
}

int fw_host_session_add_gap(const fw_config* cfg, int64_t watermark, int64_t ts, int64_t gap, int64_t value, int64_t* starts,
                            int64_t* ends, int64_t* accs, int32_t* n, int32_t capacity, int32_t* outcome) {
    return host_session_add(FW_WIN_SESSION_DYNAMIC, "FW_WIN_SESSION_DYNAMIC", "fw_host_session_add_gap", cfg, watermark, ts, &gap, value,
                            starts, ends, accs, n, capacity, outcome, nullptr);
}

int fw_host_session_add_gap_late(const fw_config* cfg, int64_t watermark, int64_t ts, int64_t gap, int64_t value, int64_t* starts,
                                 int64_t* ends, int64_t* accs, int32_t* n, int32_t capacity, int32_t* outcome,
                                 int32_t* fired_index) {
    if (!fired_index) return fail(FW_E_INVALID, "null argument");
    return host_session_add(FW_WIN_SESSION_DYNAMIC_LATENESS, "FW_WIN_SESSION_DYNAMIC_LATENESS", "fw_host_session_add_gap_late", cfg,
                            watermark, ts, &gap, value, starts, ends, accs, n, capacity, outcome, fired_index);
}

// the plan of a SQL session configuration, as fw_create makes it
static int sql_session_plan(const fw_config* cfg, const char* name, fw_handle* h) {
    if (cfg->window_kind != FW_WIN_SESSION || cfg->api != FW_API_SQL)
        return fail(FW_E_INVALID, "%s needs a FW_WIN_SESSION configuration with api FW_API_SQL", name);
    h->cfg = *cfg;
    return validate_and_plan(h);
}

int fw_host_sql_session_words(const fw_config* cfg, int32_t* nw) {
    if (!cfg || !nw) return fail(FW_E_INVALID, "null argument");
    fw_handle h;
    const int rc = sql_session_plan(cfg, "fw_host_sql_session_words", &h);
    if (rc) return rc;
    *nw = h.sw.d.nw;
    return FW_OK;
}

int fw_host_sql_session_add(const fw_config* cfg, int64_t watermark, int64_t ts, const int64_t* values, const uint8_t* nulls,
                            int64_t* starts, int64_t* ends, int64_t* acc_words, int32_t* n, int32_t capacity, int32_t* outcome) {
    if (!cfg || !n || !outcome || (capacity > 0 && (!starts || !ends || !acc_words))) return fail(FW_E_INVALID, "null argument");
    fw_handle h;
    const int rc = sql_session_plan(cfg, "fw_host_sql_session_add", &h);
    if (rc) return rc;
    if (cfg->n_value_cols > 0 && !values) return fail(FW_E_INVALID, "null argument");
    if (cfg->nullable_cols && !nulls) return fail(FW_E_INVALID, "null flags required (nullable_cols != 0)");
    if (*n < 0 || *n > capacity) return fail(FW_E_INVALID, "bad session count %d (capacity %d)", *n, capacity);
    const SessionDesc& d = h.sw.d;
    uint64_t words[SW_MAX_NW];
    for (int w = 0; w < d.nw; w++) {  // a row's words, as sw_row_words computes them on the device
        const int32_t col = d.col[w], gate = d.gate[w];
        if (gate >= 0 && nulls[gate]) words[w] = session_identity(d.ops[w]);
        else words[w] = col == SW_COL_ONE ? 1ull : (uint64_t)values[col];
    }
    uint64_t* acc = (uint64_t*)acc_words;
    int r;
    switch (d.nw) {
        case 1: r = session_add<1>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 1, n, capacity); break;
        case 2: r = session_add<2>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 2, n, capacity); break;
        case 3: r = session_add<3>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 3, n, capacity); break;
        case 4: r = session_add<4>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 4, n, capacity); break;
        case 5: r = session_add<5>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 5, n, capacity); break;
        case 6: r = session_add<6>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 6, n, capacity); break;
        case 7: r = session_add<7>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 7, n, capacity); break;
        default: r = session_add<8>(d.gap, d.ops, watermark, ts, words, 1, starts, ends, acc, 1, 8, n, capacity); break;
    }
    if (r < 0) return fail(FW_E_CAPACITY, "the session list is full (%d sessions)", capacity);
    *outcome = r;
    return FW_OK;
}

int fw_host_sql_session_result(const fw_config* cfg, const int64_t* acc_words, int64_t* values, uint32_t* null_mask) {
    if (!cfg || !acc_words || !values || !null_mask) return fail(FW_E_INVALID, "null argument");
    fw_handle h;
    const int rc = sql_session_plan(cfg, "fw_host_sql_session_result", &h);
    if (rc) return rc;
    uint32_t nm = 0;
    for (int g = 0; g < h.sw.ad.n; g++) {
        bool isnull;
        values[g] = (int64_t)sql_agg_result(h.sw.ad, g, (const uint64_t*)acc_words, &isnull);
        if (isnull) nm |= 1u << g;
    }
    *null_mask = nm;
    return FW_OK;
}

}  // extern "C"
