// fw_count.h -- DataStream count windows (KeyedStream.countWindow) as count slices.
//
// countWindow(size, slide) is GlobalWindows + CountTrigger.of(slide) + CountEvictor.of(size), run by
// EvictingWindowOperator; countWindow(size) is GlobalWindows + PurgingTrigger(CountTrigger.of(size)).
// A key fires when its element count c reaches a multiple of slide, and the fired window holds the
// key's last min(c, size) elements.  With g = gcd(size, slide) both c and c - size are multiples of
// g, so every fired window is exactly the last R = size / g complete count slices of g elements:
// the state per key is a count and a ring of R slice accumulators (DESIGN.md "Count windows").
//
// This header holds the slice arithmetic the kernel and fw_host_count_step share (FW_HD), the
// per-handle state of a count operator (CountOp) and the entry points fw_api.hip dispatches to.
#pragma once
#include "fw_folded.h"

namespace fw {

// accumulator classes of a count window's one word
enum CountWordOp : int32_t { CW_ADD_I = 0, CW_ADD_F = 1, CW_MIN = 2, CW_MAX = 3 };

struct CountDesc {
    int64_t size;       // CountEvictor.of(size)
    int64_t slide;      // CountTrigger.of(slide)
    int64_t g;          // gcd(size, slide): elements per count slice
    int32_t R;          // size / g: ring slots per key (<= FW_COUNT_MAX_SLICES)
    int32_t op;         // CountWordOp
    UDiv g_div;         // divisor g
    UDiv slide_div;     // divisor slide
    UDiv r_div;         // divisor R
};

// One element of a key, 0-based per-key index `index`: the count slice it falls in, that slice's
// ring slot, whether the element triggers a fire (CountTrigger: the count reached a multiple of
// slide) and, if so, the window's first element index max(0, c - size) and the ring slots the window
// reads (the slices [slice - n_slices + 1, slice], oldest first).
FW_HD void count_step(const CountDesc& d, int64_t index, int64_t* slice, int32_t* ring_slot, int32_t* fires,
                      int64_t* window_start, int32_t* n_slices) {
    const uint64_t s = udiv((uint64_t)index, d.g_div);
    *slice = (int64_t)s;
    *ring_slot = (int32_t)(s - udiv(s, d.r_div) * (uint64_t)d.R);
    const uint64_t c = (uint64_t)index + 1;
    const bool f = c - udiv(c, d.slide_div) * (uint64_t)d.slide == 0;
    *fires = f ? 1 : 0;
    const int64_t held = (int64_t)c < d.size ? (int64_t)c : d.size;  // min(c, size), a multiple of g at a fire
    *window_start = f ? (int64_t)c - held : 0;
    *n_slices = f ? (int32_t)udiv((uint64_t)held, d.g_div) : 0;
}

// op(older, newer): the reduce of two partial aggregates, the older one on the left (DOUBLE sums are
// added in that order; min / max compare the sortable keys of fw_device.h dkey)
FW_HD uint64_t count_fold(int32_t op, uint64_t a, uint64_t b) {
    switch (op) {
        case CW_ADD_I: return a + b;
        case CW_ADD_F: {
            double x, y;
            __builtin_memcpy(&x, &a, 8);
            __builtin_memcpy(&y, &b, 8);
            x += y;
            uint64_t r;
            __builtin_memcpy(&r, &x, 8);
            return r;
        }
        case CW_MIN: return (int64_t)b < (int64_t)a ? b : a;
        default: return (int64_t)b > (int64_t)a ? b : a;
    }
}

// ---- record-shaped count windows (FW_WIN_COUNT_RECORD): every partial aggregate travels with the
// arrival ordinal of one element.  Value words stay raw here (a DOUBLE is compared through dkey, never
// stored as one), so a NaN keeps its payload and the fold is the reducer's own:
//   CR_FIRST     sum / min / max (SumAggregator, ComparableAggregator byAggregate = false): value1 with
//                the field set -- the ordinal is the older side's; min / max keep the older field only
//                when it is strictly extremal (isExtremal), else take the newer one's
//   CR_BY_FIRST  minBy / maxBy(field, first = true): the pair with the extremal field, ties to the older
//   CR_BY_LAST   minBy / maxBy(field, first = false): ties to the newer
enum CountRecMode : int32_t { CR_FIRST = 0, CR_BY_FIRST = 1, CR_BY_LAST = 2 };

FW_HD void count_record_fold(int32_t op, int32_t mode, bool dbl, uint64_t av, uint64_t ao, uint64_t bv, uint64_t bo,
                             uint64_t* ov, uint64_t* oo) {
    if (op == CW_ADD_I || op == CW_ADD_F) {
        *ov = count_fold(op, av, bv);
        *oo = ao;
        return;
    }
    const int64_t ka = dbl ? dkey(av) : (int64_t)av, kb = dbl ? dkey(bv) : (int64_t)bv;
    const bool a_strict = op == CW_MIN ? ka < kb : ka > kb;
    const bool keep_a = a_strict || (mode == CR_BY_FIRST && ka == kb);
    *ov = keep_a ? av : bv;
    *oo = (mode == CR_FIRST || keep_a) ? ao : bo;
}

// the table's own slot hash of a key inside its superbucket (not a Flink-visible hash)
FW_HD uint32_t count_slot_hash(int64_t key, uint32_t mask) { return (uint32_t)mix64((uint64_t)key) & mask; }

constexpr int CW_TILE = FD_TILE;                    // rows per tile = threads per workgroup
constexpr int64_t CW_CLAIMED = INT64_MIN;           // count word of an entry claimed in the running tile

// Per-handle state of a count operator.  The key table is open addressed, partitioned by
// superbucket: entry e of superbucket sb is table[(sb * cap_e + e) * pwe ..]: key, count, ring[R]; a
// record handle (rec) adds ord[R], the ordinal beside each ring slot's aggregate.
// count == 0 marks an empty slot (a key enters the table with its first element).
struct CountOp {
    bool on = false;
    CountDesc d{};
    KeySpace ks{};
    int32_t vtype = 0;      // fw_value_type of the aggregated field
    int32_t is_count = 0;   // COUNT_STAR: every element counts 1, no value column is read
    int32_t val_col = 0;    // value column the aggregate reads
    int32_t cap_e = 0;      // table slots per superbucket (power of two)
    int32_t pwe = 0;        // words per entry: 2 + R (rec: 2 + 2R)
    int32_t rec = 0;        // FW_WIN_COUNT_RECORD
    int32_t mode = 0;       // rec: CountRecMode
    int32_t agg_sig = 0;    // rec: aggregate kind << 8 | flags (the snapshot fingerprint's part)
    int64_t out_cap = 0;
    hipStream_t stream = nullptr;  // the handle's
    Ctrl* ctrl = nullptr;          // the handle's control block: out_count[0], fired, live_entries, error
    uint64_t* table = nullptr;
    FoldedPart part{};             // the superbucket partition's buffers
    // result rows
    int64_t* out_key = nullptr;
    int64_t* out_ws = nullptr;
    int64_t* out_we = nullptr;
    uint64_t* out_val = nullptr;
    int64_t* out_ord = nullptr;
    uint32_t* out_null = nullptr;  // zeros
    uint64_t* out_rord = nullptr;  // rec: the ordinal of the record each result row is built from
    int64_t* ordev = nullptr;      // rec: retain / release events (ORDEV_RELEASE | ordinal) since the last read
    int64_t ordev_cap = 0;         // 2 * max_batch_rows: a row appends at most a release and a retain
    uint64_t* g_ev = nullptr;      // rec, behind the exchange: the gathered record words, [ordev_cap][F] beside ordev and
    uint64_t* g_res = nullptr;     // [out_cap][F] beside the result rows (allocated by the first cw_record_rows)
    int64_t push_seq = 0;
    int64_t watermark = INT64_MIN;
};

// validation + plan of a FW_WIN_COUNT / FW_WIN_COUNT_RECORD configuration; no device call
int cw_plan(const fw_config& c, CountOp* op);
int cw_allocate(CountOp* op, hipStream_t stream, Ctrl* ctrl);
void cw_free(CountOp* op);
// folds n rows into the state and appends the fired rows (stream-ordered, asynchronous)
int cw_push(CountOp* op, int64_t n, const int64_t* d_key, const int32_t* d_khash, const uint64_t* d_val);
// The same over a padded exchange receive buffer (the device form, behind the N > 1 keyBy exchange):
// n_segs segments of seg_len rows, segment s holding min(d_seg_counts[s], seg_len) live rows in front
// of its padding; row i has its key at d_key[i * stride], its value at d_val[i * stride] (1: columns,
// row_words: packed rows) and its hash at d_khash[i].  Arrival order is buffer position order; a
// fired row's ordinal is push_seq << 32 | the triggering element's position in the buffer.
int cw_push_segments(CountOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_key,
                     const int32_t* d_khash, const uint64_t* d_val, int32_t stride);
// A record handle's push behind the exchange: packed rows (key, unread word, the record's F fields), the
// aggregated one at word 2 + val_col; one launch (k_cw_fold<true, true>), at most max_batch_rows rows.
int cw_push_record_segments(CountOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_rows,
                            int32_t row_words);
// launches k_cw_gather_rec over the last push's buffer: g_ev / g_res take the F payload words of the rows
// its retain events and the unread result rows name (stream-ordered; the caller reads Ctrl behind it)
int cw_record_rows(CountOp* op, const int64_t* d_rows, int32_t row_words, int64_t n_rows, int32_t F);
int cw_snapshot(CountOp* op, int32_t key_group, void* buf, int64_t capacity, int64_t* size);
int cw_restore(CountOp* op, bool key_group, const void* buf, int64_t size);

}  // namespace fw
