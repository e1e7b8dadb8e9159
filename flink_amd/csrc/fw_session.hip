// fw_session.hip -- the session-window path (fw_session.h): kernels and the per-handle host code.
//
// One push is folded into the state when it is pushed: the folded paths' stable superbucket
// partition (fd_partition, fw_folded.hip: four stream-ordered launches), then
//   k_sw_fold     one workgroup per superbucket walks its rows in arrival order, a tile at a time:
//                 LDS sort by (key, ts, position), tile sessions by a segmented scan, merge with the
//                 sorted state into a scratch list, coalesce by a segmented running max of `end`
// and one launch per watermark:
//   k_sw_advance  one workgroup per superbucket: emit the due sessions, compact the rest
// k_sw_fold and k_sw_advance are templates on the accumulator words a session carries (NW = 1, 2, 4
// or 8; 3 + NW words per session): the DataStream handle is the NW = 1 instance, a SQL session handle
// takes the instance of its plan's word count and a merge class per word.  k_sw_fold<1, true> is the
// dynamic-gap form (FW_WIN_SESSION_DYNAMIC): a gap per row, read from value column 1.
// Behind the N > 1 keyBy exchange (a handle of parallelism > 1) both kernels have a device form, one
// more template argument: k_sw_fold<NW, DYN, true> reads strided rows of a padded receive buffer, whose
// live rows fd_partition_segments selected, and the watermark from Ctrl::cur; k_sw_advance<NW, true>
// reads Ctrl::cur behind the one-thread k_sw_raise.  The instances above are unchanged and are what a
// direct push of a host-watermark handle launches.
// An allowed lateness (FW_WIN_SESSION_LATENESS) is a last template argument of both kernels, NW = 1
// only: k_sw_fold<1, false, DEV, true> re-fires a retained session from the arrival-order
// walk of a late-candidate run, k_sw_advance<1, DEV, true> fires the sessions whose timer lies between
// the previous watermark and the new one and removes the ones past their cleanup time (in the device
// form behind k_sw_raise_late, which keeps the previous watermark).  Every lateness line sits behind
// that argument; the instances above compile to what they compiled to without it.
// Both together (FW_WIN_SESSION_DYNAMIC_LATENESS) are k_sw_fold<1, true, DEV, true>: the late-candidate
// tests take the row's own gap, and the advance is the lateness one, which reads no gap.
// No workgroup waits on another: the only cross-workgroup traffic is counters (atomic adds).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "fw_session.h"

namespace fw {
namespace {

// (padding, key, ts, position) order; positions are unique, so the order is total
__device__ __forceinline__ bool sw_less(uint64_t ka, int64_t ta, uint32_t pa, uint64_t kb, int64_t tb, uint32_t pb) {
    const uint32_t ia = pa >> 31, ib = pb >> 31;
    if (ia != ib) return ia < ib;
    if (ka != kb) return ka < kb;
    if (ta != tb) return ta < tb;
    return pa < pb;
}

// bitonic sort of the first n2 (a power of two <= SW_TILE) triples; every thread of the workgroup
// calls it, after a barrier behind the stores that filled the arrays; it ends with a barrier
__device__ void sw_sort(uint64_t* k, int64_t* ts, uint32_t* p, int n2) {
    const int t = threadIdx.x;
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int x = t ^ j;
            if (t < n2 && x > t) {
                const bool asc = (t & kk) == 0;
                const uint64_t ka = k[t], kb = k[x];
                const int64_t ta = ts[t], tb = ts[x];
                const uint32_t pa = p[t], pb = p[x];
                if (sw_less(kb, tb, pb, ka, ta, pa) == asc) {
                    k[t] = kb;
                    k[x] = ka;
                    ts[t] = tb;
                    ts[x] = ta;
                    p[t] = pb;
                    p[x] = pa;
                }
            }
            __syncthreads();
        }
}

// bitonic sort of n2 distinct 32-bit words
__device__ void sw_sort32(uint32_t* a, int n2) {
    const int t = threadIdx.x;
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int x = t ^ j;
            if (t < n2 && x > t) {
                const bool asc = (t & kk) == 0;
                const uint32_t va = a[t], vb = a[x];
                if ((vb < va) == asc) {
                    a[t] = vb;
                    a[x] = va;
                }
            }
            __syncthreads();
        }
}

// ---- the fold ------------------------------------------------------------------------------------
struct SwFoldArgs {
    const int64_t* key;
    const int64_t* ts;
    const uint64_t* vals[FW_MAX_COLS];   // value columns by column index (the ones SessionDesc::col names)
    const uint8_t* nulls[FW_MAX_COLS];   // null-flag columns (the ones SessionDesc::gate names)
    const uint32_t* perm;
    const int32_t* seg;
    SessionDesc d;
    uint32_t opsp;  // d.ops, two bits per word
    int64_t watermark;
    int32_t cap_s;
    int32_t late_side;
    uint64_t* state;
    uint64_t* scratch;
    int32_t* n_s;
    int64_t* min_end;
    Ctrl* ctrl;
    int64_t* side;
    int64_t side_cap;
    int64_t ord_base;  // push_seq << 32 | row offset of this launch within its call
    int32_t stride;    // the device form (DEV): key, ts and value words of row r at col[r * stride]
    // the lateness form (LATE) alone reads what follows: rows that fire at once go to the result buffer
    int64_t lateness;
    int64_t* min_fire;
    int64_t* out_key;
    int64_t* out_ws;
    int64_t* out_we;
    uint64_t* out_val;
    int64_t out_cap;
};

// first index in [lo, hi) of the sorted session list whose (key, start) is not below (k, s)
template <int SWS>
__device__ __forceinline__ int sw_lower(const uint64_t* st, int lo, int hi, uint64_t k, int64_t s) {
    while (lo < hi) {  // <= 32 steps
        const int mid = (lo + hi) >> 1;
        const uint64_t mk = st[(size_t)mid * SWS];
        const int64_t ms = (int64_t)st[(size_t)mid * SWS + 1];
        if (mk < k || (mk == k && ms < s)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a row's NW accumulator words: the identity where the word's gate column is NULL, 1 for a count
// word, 0 for a padding word, else the value of the word's column
// (DEV: value columns are strided, null-flag columns never)
template <int NW, bool DEV>
__device__ __forceinline__ void sw_row_words(const SwFoldArgs& a, uint32_t row, uint64_t* out) {
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const int32_t col = a.d.col[w], gate = a.d.gate[w];
        uint64_t v;
        if (gate >= 0 && a.nulls[gate][row]) v = session_identity((int32_t)((a.opsp >> (2 * w)) & 3u));
        else if (col == SW_COL_ONE) v = 1ull;
        else if (col == SW_COL_PAD) v = 0ull;
        else {
            v = a.vals[col][DEV ? (size_t)row * (size_t)a.stride : (size_t)row];
            if (NW == 1 && a.d.dbl_cmp) v = (uint64_t)dkey(v);
        }
        out[w] = v;
    }
}

// DYN (NW = 1 only): the dynamic-gap form.  A row's gap is the word of value column 1 and a.d.gap the
// largest a row may carry; everything that reads `ts + gap` in the static form reads the row's own end.
// DEV: the device form, behind the N > 1 keyBy exchange (sw_push_segments) and for every push of a
// handle whose watermark of record is Ctrl::cur (sw_push with no host watermark).  The rows are read
// as col[row * a.stride] -- stride 1 over separate column pointers is a SoA buffer, stride row_words
// over rows + 0, 1, 2 + c a packed one -- and the watermark from a.ctrl->cur, a word no workgroup of
// a fold launch writes.  Everything else is the one body.  The instances without DEV are the ones a
// direct push of a host-watermark handle launches; they read neither a.stride nor Ctrl::cur.
// LATE (NW = 1): the form with an allowed lateness (FW_WIN_SESSION_LATENESS).  The state
// then also holds sessions that have fired (end - 1 <= W) until their cleanup time.  A late candidate
// is the same row as ever, ts + gap - 1 <= W, and its key run takes the same arrival-order walk, where
// the drop test is the cleanup time and a row whose resulting session has end - 1 <= W emits that
// session at once (EventTimeTrigger.onElement: FIRE, no purge).  A run without a candidate holds only
// rows with ts + gap - 1 > W: whatever they merge with, fired sessions included, ends behind the
// watermark, nothing fires and nothing is dropped, so the result is the union of intervals as before.
// DYN && LATE (FW_WIN_SESSION_DYNAMIC_LATENESS): every late-candidate test takes the row's own gap g.
// A run without a candidate then holds only rows with ts + g - 1 > W, so the same holds: whatever they
// merge with, retained fired sessions included, ends behind the watermark, nothing fires at once and
// nothing is dropped, and the run keeps the parallel path with the dynamic form's running-maximum cut
// unchanged.  Ends are not ordered like starts here, so the bounds are kept per row, not per run:
//   min_fire[sb] is a lower bound of the smallest end among the sessions that have not fired,
//   min_end[sb]  a lower bound of the smallest end of any held session.
// A bound that is too high lets k_sw_advance return early past a due timer; too low is only slower.
// A session that has not fired (end - 1 > W) took its end from a held session that had not fired
// (>= the old min_fire) or from a row with ts + g - 1 > W, which is no candidate by its own gap and
// feeds tile_min_fire with its own end ts + g -- a short row inside a long run included, although the
// run's largest gap would put its timer much later.  Every row feeds tile_min_end with ts + g.
template <int NW, bool DYN = false, bool DEV = false, bool LATE = false>
__global__ __launch_bounds__(SW_TILE) void k_sw_fold(SwFoldArgs a) {
    static_assert(!DYN || NW == 1, "the dynamic-gap fold is a DataStream instance");
    static_assert(!LATE || NW == 1, "the lateness fold is a DataStream instance");
    constexpr int SWS = sw_stride(NW);   // words per session
    __shared__ uint64_t sk[SW_TILE];     // sorted keys; then the coalesce chunk's keys
    __shared__ int64_t sts[SW_TILE];     // their timestamps; then the chunk's ends
    __shared__ uint64_t sa[NW][SW_TILE]; // scan: accumulators, word by word
    __shared__ int64_t se[SW_TILE];      // scan: ends
    __shared__ uint32_t sp[SW_TILE];     // positions in the tile (arrival order)
    __shared__ uint32_t sf[SW_TILE];     // scan: segment flags
    __shared__ int32_t hx[SW_TILE];      // sorted index of the row's key run head
    __shared__ uint32_t ord[SW_TILE];    // key runs with a late candidate re-sorted by position: sorted index
    __shared__ int32_t hlo[SW_TILE];     // by head: the key's sessions are state[hlo, hhi)
    __shared__ int32_t hhi[SW_TILE];
    __shared__ int32_t hlen[SW_TILE];    // by head: run length | late-candidate flag << 30
    __shared__ int64_t c_max, c_end;     // coalesce carries: running max end of the last key, open group's end
    __shared__ uint64_t c_key, c_acc[NW];
    __shared__ int32_t c_groups, c_valid;
    __shared__ uint32_t n_drop;

    const int t = threadIdx.x;
    const int64_t gap = a.d.gap, W = DEV ? a.ctrl->cur : a.watermark;
#define SW_AT(row) (DEV ? (size_t)(row) * (size_t)a.stride : (size_t)(row))
    // the words' merge classes, two bits each, and their identities, derived where they are used:
    // one scalar register instead of three per word across the scan loops
    const uint32_t opsp = a.opsp;
#define SW_OP(w) ((int32_t)((opsp >> (2 * (w))) & 3u))
#define SW_IDN(w) session_identity(SW_OP(w))
    const int64_t seg0 = a.seg[blockIdx.x], seg1 = a.seg[blockIdx.x + 1];
    if (seg0 >= seg1) return;
    uint64_t* st = a.state + (size_t)blockIdx.x * a.cap_s * SWS;
    uint64_t* M = a.scratch + (size_t)blockIdx.x * ((size_t)a.cap_s + SW_TILE) * SWS;
    int ns = a.n_s[blockIdx.x];
    const int ns_at_entry = ns;
    int64_t tile_min_end = INT64_MAX;
    int64_t tile_min_fire = INT64_MAX;  // (LATE) over the rows that are no late candidates

    for (int64_t base = seg0; base < seg1; base += SW_TILE) {
        const int nrows = (int)(seg1 - base < SW_TILE ? seg1 - base : SW_TILE);
        const int n2 = fd_pow2(nrows);
        if (t == 0) n_drop = 0;
        bool badgap = false;  // (dynamic) a row with a gap out of range is padding: it adds nothing
        if (DYN && t < nrows) {
            const int64_t g = (int64_t)a.vals[1][SW_AT(a.perm[base + t])];
            badgap = g < 1 || g > gap;
        }
        if (t < nrows && !badgap) {
            const uint32_t row = a.perm[base + t];
            sk[t] = (uint64_t)a.key[SW_AT(row)];
            sts[t] = a.ts[SW_AT(row)];
            sp[t] = (uint32_t)t;
        } else {
            sk[t] = ~0ull;
            sts[t] = 0;
            sp[t] = FD_PAD | (uint32_t)t;
        }
        hlen[t] = 0;
        int nbad = 0;
        if (DYN) {
            nbad = __syncthreads_count(badgap);
            if (nbad && t == 0) atomicOr(&a.ctrl->error, ERR_GAP);
            if (nbad == nrows) continue;  // (uniform)
        }
        const int nt = nrows - nbad;  // the rows the tile folds
        __syncthreads();
        sw_sort(sk, sts, sp, n2);
        const bool valid = t < nt;  // the padding sorted behind the rows
        const uint64_t mykey = sk[t];
        const int64_t myts = sts[t];
        // the end of the row's own window (dynamic: its gap through perm, as its words below)
        const int64_t mygap = DYN && valid ? (int64_t)a.vals[1][SW_AT(a.perm[base + sp[t]])] : 0;
#define SW_END (DYN ? myts + mygap : myts + gap)
        const bool head = valid && (t == 0 || sk[t - 1] != mykey);
        hx[t] = head ? t : 0;
        __syncthreads();
        fd_max_scan(hx, n2);
        const int hi_ = valid ? hx[t] : 0;
        const int rank = t - hi_;
        // a key run that holds a late candidate is folded in arrival order (rule: an element that is
        // late when it arrives stays only if a session intersects it then)
        if (valid && session_late(myts, DYN ? mygap : gap, W)) atomicOr((uint32_t*)&hlen[hi_], 1u << 30);
        const bool runtail = valid && (t == nt - 1 || sk[t + 1] != mykey);
        if (runtail) atomicOr((uint32_t*)&hlen[hi_], (uint32_t)(rank + 1));
        if (head) {
            hlo[t] = sw_lower<SWS>(st, 0, ns, mykey, INT64_MIN);
            hhi[t] = mykey == ~0ull ? ns : sw_lower<SWS>(st, 0, ns, mykey + 1, INT64_MIN);
        }
        __syncthreads();
        const bool slow = valid && (hlen[hi_] >> 30) != 0;
        const int len = valid ? (hlen[hi_] & 0xFFFF) : 0;
        const int lo = valid ? hlo[hi_] : 0, hi = valid ? hhi[hi_] : 0;
        // dynamic gaps: a row's window may lie wholly inside an earlier, longer one of its key, so the
        // difference to the previous row says nothing.  The cut is where ts exceeds the run's running
        // maximum of end over the rows before it (touching windows merge: strictly greater) -- a
        // forward key-segmented max scan, in `se`, which is free until the reverse reduce below
        int64_t pmax = INT64_MIN, imax = INT64_MIN;  // the run's max end before the row / with it
        if (DYN) {
            se[t] = valid ? SW_END : INT64_MIN;
            __syncthreads();
            for (int dd = 1; dd < n2; dd <<= 1) {
                const bool take = valid && t - dd >= hi_;
                const int64_t ov = take ? se[t - dd] : INT64_MIN;
                __syncthreads();
                if (take && ov > se[t]) se[t] = ov;
                __syncthreads();
            }
            imax = se[t];
            if (valid && rank > 0) pmax = se[t - 1];
            // (se is written again behind the barrier of __syncthreads_count below)
        }
        // tile sessions of the other runs: a new one where the gap to the previous row is exceeded
        const bool shead = valid && !slow && (rank == 0 || (DYN ? myts > pmax : myts - sts[t - 1] > gap));
        const bool stail = valid && !slow && (runtail || (DYN ? sts[t + 1] > imax : sts[t + 1] - myts > gap));
        tile_min_end = valid && SW_END < tile_min_end ? SW_END : tile_min_end;
        if (LATE && valid && !session_late(myts, DYN ? mygap : gap, W) && SW_END < tile_min_fire) tile_min_fire = SW_END;
        // the sessions the tile can add at most; if they might not fit, the coalesce pass below runs
        // once more in front, only counting (uniform)
        const int may_add = __syncthreads_count(shead || slow);
        const bool tight = ns + may_add > a.cap_s;
        // the run's rows in arrival order, for the late-candidate runs
        ord[t] = valid ? ((uint32_t)hi_ << 20 | (slow ? sp[t] : (uint32_t)rank) << 10 | (uint32_t)rank) : (0x7FF00000u | (uint32_t)t);
        // reverse segmented scan: a tile session's first row gets the reduce of its rows and its end
        {
            uint64_t myword[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) myword[w] = SW_IDN(w);
            if (valid) sw_row_words<NW, DEV>(a, a.perm[base + sp[t]], myword);
            if (t < n2) {
#pragma unroll
                for (int w = 0; w < NW; w++) sa[w][t] = myword[w];
                se[t] = SW_END;
                sf[t] = (!valid || slow || stail) ? 1u : 0u;
            }
        }
        __syncthreads();
        for (int dd = 1; dd < n2; dd <<= 1) {  // all NW words per step
            const bool take = t + dd < n2 && !sf[t];
            uint64_t ov[NW];
            int64_t oe = 0;
            uint32_t of = 0;
            if (take) {
#pragma unroll
                for (int w = 0; w < NW; w++) ov[w] = sa[w][t + dd];
                oe = se[t + dd];
                of = sf[t + dd];
            }
            __syncthreads();
            if (take) {
#pragma unroll
                for (int w = 0; w < NW; w++) sa[w][t] = session_fold(SW_OP(w), sa[w][t], ov[w]);
                if (oe > se[t]) se[t] = oe;
                sf[t] = of;
            }
            __syncthreads();
        }
        sw_sort32(ord, n2);

        // ---- the merged list M: every state session and every tile row by merge path.  A row that
        // starts no tile session is a dead slot.  A late-candidate key's sessions and rows share the
        // region M[lo + head, hi + head + len), which the run's head lane fills below.
        for (int i = t; i < ns; i += SW_TILE) {
            const uint64_t k = st[(size_t)i * SWS];
            const int64_t s = (int64_t)st[(size_t)i * SWS + 1];
            int l = 0, h = nt;  // rows with key < k
            while (l < h) {
                const int mid = (l + h) >> 1;
                if (sk[mid] < k) l = mid + 1;
                else h = mid;
            }
            int before = l;
            if (l < nt && sk[l] == k && !(hlen[l] >> 30)) {  // rows of the key with ts < s
                h = l + (hlen[l] & 0xFFFF);
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    if (sts[mid] < s) l = mid + 1;
                    else h = mid;
                }
                before = l;
            }
            uint64_t* dst = M + (size_t)(i + before) * SWS;
            dst[0] = k;
            dst[1] = (uint64_t)s;
            dst[2] = st[(size_t)i * SWS + 2];
#pragma unroll
            for (int w = 0; w < NW; w++) dst[3 + w] = st[(size_t)i * SWS + 3 + w];
        }
        if (valid && !slow) {
            // state sessions of the key with start <= ts sort before the row
            const int c = sw_lower<SWS>(st, lo, hi, mykey, myts + 1);
            uint64_t* dst = M + (size_t)(t + c) * SWS;
            dst[0] = mykey;
            dst[1] = (uint64_t)myts;
            dst[2] = shead ? (uint64_t)se[t] : (uint64_t)SW_DEAD;
#pragma unroll
            for (int w = 0; w < NW; w++) dst[3 + w] = shead ? sa[w][t] : SW_IDN(w);
        }
        __threadfence_block();
        __syncthreads();
        if (head && slow) {
            uint64_t* reg = M + (size_t)(lo + t) * SWS;
            int32_t n = hi - lo;
            const int32_t room = n + len;
            for (int r = 0; r < len; r++) {  // arrival order
                const int u = hi_ + (int)(ord[t + r] & 0x3FFu);
                const int64_t ts = sts[u];
                const uint32_t row = a.perm[base + sp[u]];
                int32_t ops[NW];
#pragma unroll
                for (int w = 0; w < NW; w++) ops[w] = SW_OP(w);
                // the row's words: a late-candidate run's rows are segments of their own in the scan
                // above, so sa[.][u] still holds the words of the row at sorted index u (and se[u] its
                // own end: a dynamic gap travels like the word)
                int32_t at = 0;
                const int rc = session_add<NW, LATE>(DYN ? se[u] - ts : gap, ops, W, ts, &sa[0][u], SW_TILE, (int64_t*)reg + 1,
                                                     (int64_t*)reg + 2, reg + 3, SWS, SWS, &n, room, LATE ? a.lateness : 0, &at);
                if (LATE && rc == 1 && session_due((int64_t)reg[(size_t)at * SWS + 2], W)) {
                    // the session the row produced has fired before: it fires again, with the row
                    const unsigned long long o = atomicAdd((unsigned long long*)&a.ctrl->out_count[0], 1ull);
                    atomicAdd((unsigned long long*)&a.ctrl->fired, 1ull);
                    if (o < (unsigned long long)a.out_cap) {
                        a.out_key[o] = (int64_t)mykey;
                        a.out_ws[o] = (int64_t)reg[(size_t)at * SWS + 1];
                        a.out_we[o] = (int64_t)reg[(size_t)at * SWS + 2];
                        a.out_val[o] = session_result(a.d, reg[(size_t)at * SWS + 3]);
                    } else {
                        atomicOr(&a.ctrl->error, ERR_OUTPUT);
                    }
                }
                if (rc == 0) {  // dropped: counted (SQL has no side output: late_side is 0)
                    atomicAdd(&n_drop, 1u);
                    if (NW == 1 && a.late_side) {
                        const uint64_t raw = a.d.is_count ? 1ull : a.vals[a.d.col[0]][SW_AT(row)];
                        const unsigned long long o = atomicAdd((unsigned long long*)&a.ctrl->n_side, 1ull);
                        if (o < (unsigned long long)a.side_cap) {
                            int64_t* sd = a.side + (size_t)o * SW_SIDE_WORDS;
                            sd[0] = (int64_t)mykey;
                            sd[1] = ts;
                            sd[2] = a.ord_base + (int64_t)row;
                            sd[3] = (int64_t)raw;
                        } else {
                            atomicOr(&a.ctrl->error, ERR_LATE);
                        }
                    }
                }
            }
            for (int32_t q = 0; q < room; q++) {
                reg[(size_t)q * SWS] = mykey;
                if (q >= n) {
                    reg[(size_t)q * SWS + 1] = (uint64_t)INT64_MAX;
                    reg[(size_t)q * SWS + 2] = (uint64_t)SW_DEAD;
#pragma unroll
                    for (int w = 0; w < NW; w++) reg[(size_t)q * SWS + 3 + w] = SW_IDN(w);
                }
            }
        }
        __threadfence_block();
        __syncthreads();
        if (t == 0 && n_drop) atomicAdd((unsigned long long*)&a.ctrl->late_dropped, (unsigned long long)n_drop);

        // ---- coalesce M[0, L) into the state: a new session starts where the key changes or
        // start > the key's running max end
        const int L = ns + nt;
        bool fits = true;
        for (int pass = tight ? 0 : 1; pass < 2 && fits; pass++) {
            if (t == 0) {
                c_valid = 0;
                c_groups = 0;
                c_max = INT64_MIN;
                c_end = INT64_MIN;
                c_key = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) c_acc[w] = SW_IDN(w);
            }
            __syncthreads();
            for (int c0 = 0; c0 < L; c0 += SW_TILE) {
                const int j = c0 + t;
                const bool in = j < L;
                uint64_t k = ~0ull;
                int64_t s = INT64_MAX, e = SW_DEAD;
#pragma unroll
                for (int w = 0; w < NW; w++) sa[w][t] = SW_IDN(w);  // (free since the previous chunk's last barrier)
                if (in) {
                    const uint64_t* src = M + (size_t)j * SWS;
                    k = src[0];
                    s = (int64_t)src[1];
                    e = (int64_t)src[2];
#pragma unroll
                    for (int w = 0; w < NW; w++) sa[w][t] = src[3 + w];
                }
                const bool live = e != SW_DEAD;
                const uint64_t pk = c_key;
                const int64_t pmax = c_max, pend = c_end;
                const int32_t pgroups = c_groups, pvalid = c_valid;
                sk[t] = k;
                sts[t] = e;
                sf[t] = 0;
                __syncthreads();
                // inclusive running max of end inside the key
                for (int dd = 1; dd < SW_TILE; dd <<= 1) {
                    const bool take = t >= dd && sk[t - dd] == k;
                    const int64_t ov = take ? sts[t - dd] : INT64_MIN;
                    __syncthreads();
                    if (take && ov > sts[t]) sts[t] = ov;
                    __syncthreads();
                }
                const bool from_carry = pvalid && pk == sk[0];
                int64_t mx = INT64_MIN;  // exclusive
                if (t > 0 && sk[t - 1] == k) mx = sts[t - 1];
                if (from_carry && k == pk && pmax > mx) mx = pmax;
                const int64_t incl_last = sts[SW_TILE - 1];
                const uint64_t last_key = sk[SW_TILE - 1];
                const bool is_head = live && s > mx;
                __syncthreads();
                // group index and the reduce of each group
                int32_t total_heads;
                const int32_t hcount = fd_block_scan<SW_TILE>(is_head ? 1 : 0, hx, &total_heads);
                se[t] = e;
                sf[t] = is_head ? 1u : 0u;
                __syncthreads();
                for (int dd = 1; dd < SW_TILE; dd <<= 1) {  // all NW words per step
                    const bool take = t >= dd && !sf[t];
                    uint64_t ov[NW];
                    int64_t oe = 0;
                    uint32_t of = 0;
                    if (take) {
#pragma unroll
                        for (int w = 0; w < NW; w++) ov[w] = sa[w][t - dd];
                        oe = se[t - dd];
                        of = sf[t - dd];
                    }
                    __syncthreads();
                    if (take) {
#pragma unroll
                        for (int w = 0; w < NW; w++) sa[w][t] = session_fold(SW_OP(w), ov[w], sa[w][t]);
                        if (oe > se[t]) se[t] = oe;
                        sf[t] = of;
                    }
                    __syncthreads();
                }
                uint64_t gacc[NW];
#pragma unroll
                for (int w = 0; w < NW; w++) gacc[w] = sa[w][t];
                int64_t gend = se[t];
                if (hcount == 0) {  // still the group the previous chunk left open (c_acc: rewritten behind the next barrier)
#pragma unroll
                    for (int w = 0; w < NW; w++) gacc[w] = session_fold(SW_OP(w), c_acc[w], gacc[w]);
                    if (pend > gend) gend = pend;
                }
                const int32_t g = pgroups + hcount - 1;
                const bool glast = t == SW_TILE - 1 || j + 1 >= L || hx[t + 1] != hcount;
                if (pass == 1 && in && g >= 0 && g < a.cap_s) {
                    uint64_t* dst = st + (size_t)g * SWS;
                    if (is_head) {
                        dst[0] = k;
                        dst[1] = (uint64_t)s;
                    }
                    if (glast) {
                        dst[2] = (uint64_t)gend;
#pragma unroll
                        for (int w = 0; w < NW; w++) dst[3 + w] = gacc[w];
                    }
                }
                __syncthreads();
                if (t == SW_TILE - 1) {
                    c_valid = 1;
                    c_key = last_key;
                    c_max = (from_carry && last_key == pk && pmax > incl_last) ? pmax : incl_last;
                    c_groups = pgroups + total_heads;
#pragma unroll
                    for (int w = 0; w < NW; w++) c_acc[w] = gacc[w];
                    c_end = gend;
                }
                __threadfence_block();
                __syncthreads();
            }
            if (pass == 0 && c_groups > a.cap_s) fits = false;
            __syncthreads();
        }
        if (!fits) {  // the fold's result does not fit: the tile's rows are dropped, the state stays
            if (t == 0) atomicOr(&a.ctrl->error, ERR_STATE);
            continue;
        }
        ns = c_groups < a.cap_s ? c_groups : a.cap_s;
        __syncthreads();
    }
    if (t == 0) {
        a.n_s[blockIdx.x] = ns;
        if (ns != ns_at_entry)
            atomicAdd((unsigned long long*)&a.ctrl->live_entries, (unsigned long long)(long long)(ns - ns_at_entry));
    }
    // every session's end is at least the smaller of the old bound and the tile rows' ts + gap
    sts[t] = tile_min_end;
    __syncthreads();
    for (int dd = SW_TILE >> 1; dd > 0; dd >>= 1) {
        if (t < dd && sts[t + dd] < sts[t]) sts[t] = sts[t + dd];
        __syncthreads();
    }
    if (t == 0 && sts[0] < a.min_end[blockIdx.x]) a.min_end[blockIdx.x] = sts[0];
    if (LATE) {
        // a session that has not fired ends where a held one did or where a row that is no late
        // candidate (by its own gap) does: a candidate's own window ends at or before W + 1
        __syncthreads();
        sts[t] = tile_min_fire;
        __syncthreads();
        for (int dd = SW_TILE >> 1; dd > 0; dd >>= 1) {
            if (t < dd && sts[t + dd] < sts[t]) sts[t] = sts[t + dd];
            __syncthreads();
        }
        if (t == 0 && sts[0] < a.min_fire[blockIdx.x]) a.min_fire[blockIdx.x] = sts[0];
    }
#undef SW_OP
#undef SW_IDN
#undef SW_END
#undef SW_AT
}

// ---- the watermark -----------------------------------------------------------------------------
struct SwAdvArgs {
    SessionDesc d;
    AggDesc ad;   // SQL: the aggregates over the session's words
    int64_t watermark;
    int32_t cap_s;
    uint64_t* state;
    int32_t* n_s;
    int64_t* min_end;
    Ctrl* ctrl;
    int64_t* out_key;
    int64_t* out_ws;
    int64_t* out_we;
    uint64_t* out_val[FW_MAX_AGGS];
    uint32_t* out_null;
    int64_t out_cap;
    // the lateness form (LATE) alone reads what follows
    int64_t lateness;
    int64_t prev_watermark;     // host form: the watermark in front of this advance
    const int64_t* prev_wm;     // device form: the same, as k_sw_raise_late left it
    int64_t* min_fire;
};

// DEV: the watermark is Ctrl::cur, which k_sw_raise set in a launch of its own in front (no
// workgroup of this launch writes it)
// LATE: an advance from W0 to W emits the sessions whose timer lies in (W0, W] -- the ones at or below
// W0 have fired -- and removes the ones whose cleanup time end - 1 + L has passed, emitted or not.
// min_fire and min_end are exact behind it, so an advance that neither fires nor cleans returns
// without reading the list.
template <int NW, bool DEV = false, bool LATE = false>
__global__ __launch_bounds__(SW_TILE) void k_sw_advance(SwAdvArgs a) {
    static_assert(!LATE || NW == 1, "the lateness advance is the DataStream instance");
    constexpr int SWS = sw_stride(NW);
    const int64_t W = DEV ? a.ctrl->cur : a.watermark;
    const int64_t W0 = !LATE ? 0 : DEV ? *a.prev_wm : a.prev_watermark;
    const int64_t Lt = LATE ? a.lateness : 0;
    __shared__ int32_t buf[SW_TILE];
    __shared__ int64_t mn[SW_TILE];
    __shared__ unsigned long long out_base;
    const int t = threadIdx.x;
    const int ns = a.n_s[blockIdx.x];
    if (!LATE && (ns == 0 || !session_due(a.min_end[blockIdx.x], W))) return;  // nothing is due (uniform)
    if (LATE && (ns == 0 || W <= W0 || (!session_due(a.min_fire[blockIdx.x], W) && !session_cleaned(a.min_end[blockIdx.x], Lt, W))))
        return;  // no timer of either kind is due (uniform)
    uint64_t* st = a.state + (size_t)blockIdx.x * a.cap_s * SWS;
    // the due sessions, counted first: one device atomic per workgroup claims their output rows
    int32_t mine = 0;
#define SW_DUE(e) (LATE ? session_fires((e), W0, W) : session_due((e), W))
#define SW_GONE(e) (LATE ? session_cleaned((e), Lt, W) : session_due((e), W))
    for (int i = t; i < ns; i += SW_TILE) mine += SW_DUE((int64_t)st[(size_t)i * SWS + 2]) ? 1 : 0;
    int32_t n_due;
    fd_block_scan<SW_TILE>(mine, buf, &n_due);
    if (t == 0) {
        out_base = 0;
        if (n_due) {
            out_base = atomicAdd((unsigned long long*)&a.ctrl->out_count[0], (unsigned long long)n_due);
            atomicAdd((unsigned long long*)&a.ctrl->fired, (unsigned long long)n_due);
            if (!LATE) atomicAdd((unsigned long long*)&a.ctrl->live_entries, (unsigned long long)(long long)(-n_due));
            if (out_base + (unsigned long long)n_due > (unsigned long long)a.out_cap) atomicOr(&a.ctrl->error, ERR_OUTPUT);
        }
    }
    __syncthreads();
    const bool sql = a.d.sql != 0;  // (uniform)
    int32_t fired = 0, kept = 0;
    int64_t min_end = INT64_MAX, min_fire = INT64_MAX;
    for (int c0 = 0; c0 < ns; c0 += SW_TILE) {
        const int i = c0 + t;
        const bool in = i < ns;
        uint64_t k = 0, acc[NW];
        int64_t s = 0, e = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) acc[w] = 0;
        if (in) {
            k = st[(size_t)i * SWS];
            s = (int64_t)st[(size_t)i * SWS + 1];
            e = (int64_t)st[(size_t)i * SWS + 2];
#pragma unroll
            for (int w = 0; w < NW; w++) acc[w] = st[(size_t)i * SWS + 3 + w];
        }
        const bool due = in && SW_DUE(e);
        int32_t n_f;
        int32_t fi = fd_block_scan<SW_TILE>(due ? 1 : 0, buf, &n_f);  // (barriers: the chunk is in registers)
        const int32_t n_in = ns - c0 < SW_TILE ? ns - c0 : SW_TILE;
        if (due) {
            const unsigned long long o = out_base + (unsigned long long)(fired + fi - 1);
            if (o < (unsigned long long)a.out_cap) {
                a.out_key[o] = (int64_t)k;
                a.out_ws[o] = s;
                a.out_we[o] = e;
                if (!sql) {
                    a.out_val[0][o] = session_result(a.d, acc[0]);
                } else {
                    // the aggregates index the words at run time: read from the session's own slot,
                    // which no kept session of this chunk is moved into before the barrier below
                    uint32_t nm = 0;
                    for (int g = 0; g < a.ad.n; g++) {
                        bool isnull;
                        const uint64_t v = sql_agg_result(a.ad, g, st + (size_t)i * SWS + 3, &isnull);
                        a.out_val[g][o] = v;
                        if (isnull) nm |= 1u << g;
                    }
                    a.out_null[o] = nm;
                }
            }
        }
        if (sql) __syncthreads();
        bool gone = due;
        if (LATE) {  // what leaves the list is what is cleaned, a set of its own: counted again
            gone = in && SW_GONE(e);
            fired += n_f;  // (the output rows claimed so far)
            fi = fd_block_scan<SW_TILE>(gone ? 1 : 0, buf, &n_f);
        }
        if (in && !gone) {  // stable compaction: the slot is at or before the session's own
            uint64_t* dst = st + (size_t)(kept + (t + 1 - fi) - 1) * SWS;
            dst[0] = k;
            dst[1] = (uint64_t)s;
            dst[2] = (uint64_t)e;
#pragma unroll
            for (int w = 0; w < NW; w++) dst[3 + w] = acc[w];
            if (e < min_end) min_end = e;
            if (LATE && !session_due(e, W) && e < min_fire) min_fire = e;
        }
        if (!LATE) fired += n_f;
        kept += n_in - n_f;
        __threadfence_block();
        __syncthreads();
    }
    mn[t] = min_end;
    __syncthreads();
    for (int dd = SW_TILE >> 1; dd > 0; dd >>= 1) {
        if (t < dd && mn[t + dd] < mn[t]) mn[t] = mn[t + dd];
        __syncthreads();
    }
    if (t == 0) {
        a.n_s[blockIdx.x] = kept;
        a.min_end[blockIdx.x] = mn[0];
        if (LATE && kept != ns)
            atomicAdd((unsigned long long*)&a.ctrl->live_entries, (unsigned long long)(long long)(kept - ns));
    }
    if (LATE) {
        __syncthreads();
        mn[t] = min_fire;
        __syncthreads();
        for (int dd = SW_TILE >> 1; dd > 0; dd >>= 1) {
            if (t < dd && mn[t + dd] < mn[t]) mn[t] = mn[t + dd];
            __syncthreads();
        }
        if (t == 0) a.min_fire[blockIdx.x] = mn[0];
    }
#undef SW_DUE
#undef SW_GONE
}

// k_sw_raise for a lateness handle: the watermark in front of the raise goes to *prev, a word of the
// session operator that only k_sw_advance<1, true, true> reads, in the launch behind this one
__global__ void k_sw_raise_late(Ctrl* ctrl, const int64_t* d_w, int64_t w, int64_t* prev) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t v = d_w ? *d_w : w;
        const int64_t c = ctrl->cur;
        *prev = c;
        if (v > c) ctrl->cur = v;
    }
}

// Ctrl::cur = max(Ctrl::cur, the proposed watermark): *d_w if given, else w.  One thread, a launch of
// its own in front of k_sw_advance<NW, true>, so no launch both reads and writes the word.
__global__ void k_sw_raise(Ctrl* ctrl, const int64_t* d_w, int64_t w) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t v = d_w ? *d_w : w;
        if (v > ctrl->cur) ctrl->cur = v;
    }
}

__global__ void k_sw_fill(int64_t* p, int64_t v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

// the SQL form: SESSION(TABLE t PARTITION BY k, DESCRIPTOR(rowtime), gap) aggregated per session
static int sw_plan_sql(const fw_config& c, SessionOp* op) {
    if (c.key_hash == FW_KEYHASH_LONG || c.key_hash == FW_KEYHASH_INT)
        return set_error(FW_E_INVALID, "FW_KEYHASH_LONG / FW_KEYHASH_INT are DataStream key hashes; a SQL session takes BINROW_BIGINT / "
                                       "BINROW_INT / PRECOMPUTED keys");
    if (c.key_hash == FW_KEYHASH_KEYROW)
        return set_error(FW_E_INVALID, "SQL session windows: key rows (FW_KEYHASH_KEYROW) run on the reference operator");
    if (c.size_ms < 1) return set_error(FW_E_INVALID, "session gap (size_ms) must be > 0");
    if (c.size_ms > SW_MAX_GAP) return set_error(FW_E_INVALID, "session gap (size_ms) must be <= 2^40");
    if (c.slide_ms != 0) return set_error(FW_E_INVALID, "session windows have no slide (slide_ms must be 0)");
    if (c.offset_ms != 0) return set_error(FW_E_INVALID, "session windows have no offset (offset_ms must be 0)");
    if (c.allowed_lateness_ms != 0)
        return set_error(FW_E_INVALID, "SQL session windows have no allowed lateness (allowed_lateness_ms must be 0)");
    if (c.late_side_output != 0)
        return set_error(FW_E_INVALID, "SQL session windows have no late side output (late_side_output must be 0)");
    if (c.ds_first_ordinals) return set_error(FW_E_INVALID, "ds_first_ordinals is a DataStream option (ds_first_ordinals must be 0)");
    if (c.tz_n != 0)
        return set_error(FW_E_INVALID, "SQL session windows over TIMESTAMP_LTZ (shift time zones) run on the reference operator (tz_n must be 0)");
    if (c.agg_phase != FW_PHASE_ONE)
        return set_error(FW_E_INVALID, "SQL session windows are one-phase (agg_phase must be FW_PHASE_ONE)");
    if (c.max_batch_rows <= 0 || c.max_batch_rows >= (1ll << 31)) return set_error(FW_E_INVALID, "max_batch_rows must be in (0, 2^31)");
    if (c.output_capacity <= 0) return set_error(FW_E_INVALID, "output_capacity must be > 0");
    for (int g = 0; g < c.n_aggs; g++) {
        const fw_agg_desc& a = c.aggs[g];
        if (a.kind < FW_AGG_COUNT_STAR || a.kind > FW_AGG_AVG)
            return set_error(FW_E_INVALID, "SQL session windows: agg %d: kind %d is not COUNT(*) / COUNT / SUM / MIN / MAX / AVG", g, a.kind);
        if (a.type != FW_T_I64 && a.type != FW_T_I32 && a.type != FW_T_F64)
            return set_error(FW_E_INVALID, "SQL session windows: agg %d: bad type %d", g, a.type);
        if ((a.kind == FW_AGG_MIN || a.kind == FW_AGG_MAX) && a.type == FW_T_F64)
            return set_error(FW_E_INVALID, "SQL session windows: agg %d: MIN / MAX over DOUBLE run on the reference operator (strict "
                                           "comparison in arrival order)", g);
    }
    WordDesc wd{};
    int rc = plan_aggs(c, &wd, &op->ad, op->slot_col, &op->n_slots);
    if (rc) return rc;
    SessionDesc& d = op->d;
    d = SessionDesc{};
    d.gap = c.size_ms;
    d.sql = 1;
    d.nw = wd.nw;
    for (int w = 0; w < SW_MAX_NW; w++) {
        d.ops[w] = CW_ADD_I;
        d.col[w] = SW_COL_PAD;
        d.gate[w] = -1;
        if (w >= wd.nw) continue;
        d.ops[w] = session_op_of_word(wd.op[w]);
        if (d.ops[w] < 0)  // W_Q*, W_DN*, W_BY*, W_FIRST, W_CNTV: the sorted fold has no arrival ordinals
            return set_error(FW_E_INVALID, "SQL session windows: accumulator word op %d is outside the four merge classes", wd.op[w]);
        d.col[w] = wd.op[w] == W_CNT ? SW_COL_ONE : op->slot_col[wd.col[w]];
        d.gate[w] = wd.gate[w] >= 0 ? op->slot_col[wd.gate[w]] : -1;
    }
    d.op = d.ops[0];
    op->nw_t = sw_round_nw(d.nw);
    op->n_out = c.n_aggs;
    op->val_col = 0;
    op->late_side = 0;
    return FW_OK;
}

// the DataStream forms: EventTimeSessionWindows.withGap with one built-in aggregation; dyn:
// withDynamicGap (FW_WIN_SESSION_DYNAMIC); late: with allowedLateness >= 0 (FW_WIN_SESSION_LATENESS); both:
// FW_WIN_SESSION_DYNAMIC_LATENESS.  The kinds share every message.  They differ in where the lateness is
// checked -- the static and dynamic kinds refuse any, the lateness kind checks its range behind the API,
// the dynamic lateness kind last -- and the lateness kind alone names itself when the API is wrong.
static int sw_plan_ds(const fw_config& c, SessionOp* op, bool dyn, bool late) {
    const bool bad_lateness = c.allowed_lateness_ms < 0 || c.allowed_lateness_ms > SW_MAX_GAP;
    const char* const lateness_range = "session windows: allowed_lateness_ms must be in [0, 2^40]";
    if (c.api != FW_API_DATASTREAM)
        return late && !dyn ? set_error(FW_E_INVALID, "FW_WIN_SESSION_LATENESS (EventTimeSessionWindows with allowedLateness) is a "
                                                      "DataStream window: api must be FW_API_DATASTREAM")
                            : set_error(FW_E_INVALID, "FW_WIN_SESSION (EventTimeSessionWindows) is a DataStream window: api must be "
                                                      "FW_API_DATASTREAM");
    if (late && !dyn && bad_lateness) return set_error(FW_E_INVALID, "%s", lateness_range);
    if (c.n_aggs != 1) return set_error(FW_E_INVALID, "session windows take one aggregation (n_aggs == 1), got %d", c.n_aggs);
    const fw_agg_desc& g = c.aggs[0];
    if (g.kind == FW_AGG_MINBY || g.kind == FW_AGG_MAXBY)
        return set_error(FW_E_INVALID, "session windows: minBy / maxBy run on the reference operator");
    if (g.kind != FW_AGG_SUM && g.kind != FW_AGG_MIN && g.kind != FW_AGG_MAX && g.kind != FW_AGG_COUNT_STAR)
        return set_error(FW_E_INVALID, "session windows: aggregate kind %d is not sum / min / max / count", g.kind);
    if (g.type != FW_T_I64 && g.type != FW_T_I32 && g.type != FW_T_F64)
        return set_error(FW_E_INVALID, "session windows: bad aggregate type %d", g.type);
    if (g.flags) return set_error(FW_E_INVALID, "session windows: bad aggregate flags %d", g.flags);
    const bool is_count = g.kind == FW_AGG_COUNT_STAR;
    if (!is_count) {
        if (g.input_col < 0 || g.input_col >= c.n_value_cols) return set_error(FW_E_INVALID, "session windows: bad input_col");
        if (c.value_col_types[g.input_col] != g.type)
            return set_error(FW_E_INVALID, "session windows: type does not match value column type");
    }
    if (c.size_ms < 1) return set_error(FW_E_INVALID, "session gap (size_ms) must be > 0");
    if (c.size_ms > SW_MAX_GAP) return set_error(FW_E_INVALID, "session gap (size_ms) must be <= 2^40");
    if (c.slide_ms != 0) return set_error(FW_E_INVALID, "session windows have no slide (slide_ms must be 0)");
    if (c.offset_ms != 0) return set_error(FW_E_INVALID, "session windows have no offset (offset_ms must be 0)");
    if (!late && c.allowed_lateness_ms != 0)
        return set_error(FW_E_INVALID, "session windows with allowed lateness run on the reference operator (allowed_lateness_ms must be 0)");
    if (c.late_side_output != 0 && c.late_side_output != 1) return set_error(FW_E_INVALID, "late_side_output must be 0 or 1");
    if (c.ds_first_ordinals) return set_error(FW_E_INVALID, "session windows are (key, aggregate) shaped (ds_first_ordinals must be 0)");
    if (c.nullable_cols) return set_error(FW_E_INVALID, "session windows take no NULL inputs (nullable_cols must be 0)");
    if (c.tz_n != 0) return set_error(FW_E_INVALID, "session windows have no time zone (tz_n must be 0)");
    if (c.agg_phase != FW_PHASE_ONE) return set_error(FW_E_INVALID, "session windows are one-phase (agg_phase must be FW_PHASE_ONE)");
    if (c.key_hash != FW_KEYHASH_LONG && c.key_hash != FW_KEYHASH_INT && c.key_hash != FW_KEYHASH_PRECOMPUTED)
        return set_error(FW_E_INVALID, "session windows take LONG, INT or PRECOMPUTED keys (key_hash %d: KEYROW / BINROW keys are not supported)",
                         c.key_hash);
    if (c.max_batch_rows <= 0 || c.max_batch_rows >= (1ll << 31)) return set_error(FW_E_INVALID, "max_batch_rows must be in (0, 2^31)");
    if (c.output_capacity <= 0) return set_error(FW_E_INVALID, "output_capacity must be > 0");

    SessionDesc& d = op->d;
    d = SessionDesc{};
    d.gap = c.size_ms;
    const bool f = g.type == FW_T_F64;
    d.op = is_count ? CW_ADD_I : g.kind == FW_AGG_SUM ? (f ? CW_ADD_F : CW_ADD_I) : g.kind == FW_AGG_MIN ? CW_MIN : CW_MAX;
    d.vtype = g.type;
    d.is_count = is_count;
    d.dbl_cmp = f && !is_count && (d.op == CW_MIN || d.op == CW_MAX);
    d.nw = 1;
    for (int w = 0; w < SW_MAX_NW; w++) {
        d.ops[w] = CW_ADD_I;
        d.col[w] = SW_COL_PAD;
        d.gate[w] = -1;
    }
    d.ops[0] = d.op;
    d.col[0] = is_count ? SW_COL_ONE : g.input_col;
    op->nw_t = 1;
    op->n_out = 1;
    op->val_col = is_count ? 0 : g.input_col;
    op->late_side = c.late_side_output;
    if (dyn) {  // value column 1 carries the element's gap and size_ms (d.gap) the largest one
        if (c.n_value_cols != 2)
            return set_error(FW_E_INVALID, "dynamic-gap session windows take two value columns, the aggregated field and the gap "
                                           "(n_value_cols == 2), got %d", c.n_value_cols);
        if (c.value_col_types[1] != FW_T_I64)
            return set_error(FW_E_INVALID, "dynamic-gap session windows: the gap column (value column 1) must be FW_T_I64");
        if (!is_count && g.input_col != 0)
            return set_error(FW_E_INVALID, "dynamic-gap session windows: the aggregate reads value column 0 (input_col %d: column 1 is the gap)",
                             g.input_col);
        if (late && bad_lateness) return set_error(FW_E_INVALID, "%s", lateness_range);
    }
    op->dyn = dyn;
    op->late = late;
    op->lateness = late ? c.allowed_lateness_ms : 0;
    return FW_OK;
}

int sw_plan(const fw_config& c, SessionOp* op) {
    const bool dyn = c.window_kind == FW_WIN_SESSION_DYNAMIC || c.window_kind == FW_WIN_SESSION_DYNAMIC_LATENESS;
    const bool late = c.window_kind == FW_WIN_SESSION_LATENESS || c.window_kind == FW_WIN_SESSION_DYNAMIC_LATENESS;
    const int prc = !dyn && !late && c.api == FW_API_SQL ? sw_plan_sql(c, op) : sw_plan_ds(c, op, dyn, late);
    if (prc) return prc;
    const SessionDesc& d = op->d;

    KeySpace& ks = op->ks;
    const int rc = fd_plan_keyspace(c, "session windows", &ks, &op->part);
    if (rc) return rc;
    // twice the hinted share of a superbucket
    const int64_t hint = std::max<int64_t>(c.state_capacity, 1024);
    const int64_t cs = fd_next_pow2(std::max<int64_t>(64, 2 * ((hint + ks.n_sb - 1) / ks.n_sb)));
    if (cs > (1ll << 22)) return set_error(FW_E_INVALID, "session windows: state_capacity too large per superbucket");
    op->cap_s = (int32_t)cs;
    op->out_cap = c.output_capacity;
    op->side_cap = c.late_side_output ? 2 * c.max_batch_rows : 0;
    // the semantics fingerprint of the blobs (FNV-1a, as the time windows'), one value list per kind
    std::vector<int64_t> fp{(int64_t)c.api, (int64_t)c.window_kind, d.gap};
    if (!d.sql) {  // (the DataStream blobs' fingerprint since their first build; the other three kinds name themselves, and
        // a lateness kind its lateness: the fired sessions of a blob are read off its watermark)
        if (op->late) fp.push_back(op->lateness);
        fp.insert(fp.end(), {(int64_t)d.op, (int64_t)d.vtype, (int64_t)d.is_count, (int64_t)ks.hash_kind, (int64_t)ks.max_p});
    } else {  // every aggregate, the NULL-able columns, key hash, max parallelism
        fp.insert(fp.end(), {(int64_t)c.n_aggs, (int64_t)c.nullable_cols, (int64_t)ks.hash_kind, (int64_t)ks.max_p});
        for (int g = 0; g < c.n_aggs; g++)
            fp.insert(fp.end(), {(int64_t)c.aggs[g].kind, (int64_t)c.aggs[g].type, (int64_t)c.aggs[g].input_col});
    }
    uint64_t x = 0xcbf29ce484222325ull;
    for (int64_t v : fp)
        for (int b = 0; b < 8; b++) {
            x ^= (uint64_t)((v >> (8 * b)) & 0xff);
            x *= 0x100000001b3ull;
        }
    op->fingerprint = x;
    op->on = true;
    return FW_OK;
}

int sw_allocate(SessionOp* op, hipStream_t stream, Ctrl* ctrl) {
    op->stream = stream;
    op->ctrl = ctrl;
    int rc;
    const int n_sb = op->ks.n_sb;
    const size_t sws = (size_t)sw_stride(op->nw_t);
    if ((rc = fd_dalloc(&op->state, (size_t)n_sb * op->cap_s * sws))) return rc;
    if ((rc = fd_dalloc(&op->scratch, (size_t)n_sb * ((size_t)op->cap_s + SW_TILE) * sws))) return rc;
    if ((rc = fd_dalloc(&op->n_s, (size_t)n_sb))) return rc;
    FD_TRY(hipMemsetAsync(op->n_s, 0, (size_t)n_sb * 4, stream));
    if ((rc = fd_dalloc(&op->min_end, (size_t)n_sb))) return rc;
    hipLaunchKernelGGL(k_sw_fill, dim3((n_sb + 255) / 256), dim3(256), 0, stream, op->min_end, INT64_MAX, n_sb);
    if (op->late) {
        if ((rc = fd_dalloc(&op->min_fire, (size_t)n_sb))) return rc;
        hipLaunchKernelGGL(k_sw_fill, dim3((n_sb + 255) / 256), dim3(256), 0, stream, op->min_fire, INT64_MAX, n_sb);
        if ((rc = fd_dalloc(&op->prev_wm, 1))) return rc;
        hipLaunchKernelGGL(k_sw_fill, dim3(1), dim3(256), 0, stream, op->prev_wm, INT64_MIN, 1);
    }
    if ((rc = fd_allocate(&op->part, op->ks))) return rc;
    const size_t oc = (size_t)op->out_cap;
    if ((rc = fd_dalloc(&op->out_key, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_ws, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_we, oc))) return rc;
    for (int g = 0; g < op->n_out; g++)
        if ((rc = fd_dalloc(&op->out_val[g], oc))) return rc;
    if ((rc = fd_dalloc(&op->out_null, oc))) return rc;
    FD_TRY(hipMemsetAsync(op->out_null, 0, oc * 4, stream));
    if (op->side_cap && (rc = fd_dalloc(&op->side, (size_t)op->side_cap * SW_SIDE_WORDS))) return rc;
    FD_TRY(hipGetLastError());
    return FW_OK;
}

void sw_free(SessionOp* op) {
    hipFree(op->state);
    hipFree(op->scratch);
    hipFree(op->n_s);
    hipFree(op->min_end);
    hipFree(op->min_fire);
    hipFree(op->prev_wm);
    fd_free(&op->part);
    hipFree(op->out_key);
    hipFree(op->out_ws);
    hipFree(op->out_we);
    for (int g = 0; g < FW_MAX_AGGS; g++) hipFree(op->out_val[g]);
    hipFree(op->out_null);
    hipFree(op->side);
}

// The kernels' instance of a handle, chosen in one place: calls launch(SwInstance<NW, DYN, DEV, LATE>{})
// with NW = nw_t (sw_round_nw of the plan's words).  DYN and LATE exist with NW == 1 only (the DataStream
// kinds), so a fold has 14 instances; an advance ignores DYN and has 10.
template <int NW, bool DYN, bool DEV, bool LATE>
struct SwInstance {
    static constexpr int nw = NW;
    static constexpr bool dyn = DYN, dev = DEV, late = LATE;
};
template <int NW, class F>
static void sw_dispatch_sql(bool dev, F& launch) {
    if (dev) launch(SwInstance<NW, false, true, false>{});
    else launch(SwInstance<NW, false, false, false>{});
}
template <class F>
static void sw_dispatch(int32_t nw_t, bool dyn, bool dev, bool late, F launch) {
    switch (nw_t) {
        case 1:
            switch ((dyn ? 4 : 0) | (dev ? 2 : 0) | (late ? 1 : 0)) {
                case 0: launch(SwInstance<1, false, false, false>{}); break;
                case 1: launch(SwInstance<1, false, false, true>{}); break;
                case 2: launch(SwInstance<1, false, true, false>{}); break;
                case 3: launch(SwInstance<1, false, true, true>{}); break;
                case 4: launch(SwInstance<1, true, false, false>{}); break;
                case 5: launch(SwInstance<1, true, false, true>{}); break;
                case 6: launch(SwInstance<1, true, true, false>{}); break;
                default: launch(SwInstance<1, true, true, true>{}); break;
            }
            break;
        case 2: sw_dispatch_sql<2>(dev, launch); break;
        case 4: sw_dispatch_sql<4>(dev, launch); break;
        default: sw_dispatch_sql<8>(dev, launch); break;
    }
}

// the folds of one call: n rows at d_key[i * stride] ..., split into launches of part.cap_rows rows by
// position.  d_seg_counts: the rows are a padded buffer of segments of seg_len rows (the device form);
// dev: the device form of the fold (strided reads, the watermark from Ctrl::cur, `watermark` unread)
static int sw_fold_call(SessionOp* op, bool dev, int64_t watermark, int64_t n, const int64_t* d_key, const int64_t* d_ts,
                        int32_t stride, const int32_t* d_khash, const void* const* d_vals, const uint8_t* const* d_nulls,
                        const int64_t* d_seg_counts, int64_t seg_len) {
    if (n >= (1ll << 32) || op->push_seq >= (1ll << 30))
        return set_error(FW_E_INVALID, "arrival ordinals need < 2^32 rows per call and < 2^30 calls");
    hipStream_t s = op->stream;
    const int n_sb = op->ks.n_sb;
    const int64_t cap_rows = op->part.cap_rows;
    for (int64_t o = 0; o < n; o += cap_rows) {
        const int64_t m = std::min(cap_rows, n - o);
        const int rc = d_seg_counts ? fd_partition_segments(op->part, op->ks, op->ctrl, s, m, d_key + o * stride, stride,
                                                            d_khash ? d_khash + o : nullptr, d_seg_counts, seg_len, o)
                                    : fd_partition(op->part, op->ks, op->ctrl, s, m, d_key + o, d_khash ? d_khash + o : nullptr);
        if (rc) return rc;
        SwFoldArgs fa{};
        fa.key = d_key + o * stride;
        fa.ts = d_ts + o * stride;
        for (int w = 0; w < op->d.nw; w++) {  // the columns the words name
            const int32_t col = op->d.col[w], gate = op->d.gate[w];
            if (col >= 0) fa.vals[col] = (const uint64_t*)d_vals[col] + o * stride;
            if (gate >= 0) fa.nulls[gate] = d_nulls[gate] + o;
        }
        if (op->dyn) fa.vals[1] = (const uint64_t*)d_vals[1] + o * stride;  // the gap column
        fa.perm = op->part.perm;
        fa.seg = op->part.seg;
        fa.d = op->d;
        for (int w = 0; w < SW_MAX_NW; w++) fa.opsp |= (uint32_t)op->d.ops[w] << (2 * w);
        fa.watermark = watermark;
        fa.cap_s = op->cap_s;
        fa.late_side = op->late_side;
        fa.state = op->state;
        fa.scratch = op->scratch;
        fa.n_s = op->n_s;
        fa.min_end = op->min_end;
        fa.ctrl = op->ctrl;
        fa.side = op->side;
        fa.side_cap = op->side_cap;
        fa.ord_base = (op->push_seq << 32) + o;
        fa.stride = stride;
        if (op->late) {
            fa.lateness = op->lateness;
            fa.min_fire = op->min_fire;
            fa.out_key = op->out_key;
            fa.out_ws = op->out_ws;
            fa.out_we = op->out_we;
            fa.out_val = op->out_val[0];
            fa.out_cap = op->out_cap;
        }
        sw_dispatch(op->nw_t, op->dyn, dev, op->late, [&](auto inst) {
            using I = decltype(inst);
            hipLaunchKernelGGL((k_sw_fold<I::nw, I::dyn, I::dev, I::late>), dim3(n_sb), dim3(SW_TILE), 0, s, fa);
        });
        FD_TRY(hipGetLastError());
    }
    op->push_seq++;
    return FW_OK;
}

int sw_push(SessionOp* op, int64_t watermark, int64_t n, const int64_t* d_key, const int64_t* d_ts, const int32_t* d_khash,
            const void* const* d_vals, const uint8_t* const* d_nulls) {
    return sw_fold_call(op, op->wm_dev, watermark, n, d_key, d_ts, 1, d_khash, d_vals, d_nulls, nullptr, 0);
}

int sw_push_segments(SessionOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_key,
                     const int64_t* d_ts, int32_t stride, const int32_t* d_khash, const void* const* d_vals,
                     const uint8_t* const* d_nulls) {
    return sw_fold_call(op, true, 0, (int64_t)n_segs * seg_len, d_key, d_ts, stride, d_khash, d_vals, d_nulls, d_seg_counts, seg_len);
}

static SwAdvArgs sw_adv_args(SessionOp* op, int64_t watermark) {
    SwAdvArgs a{};
    a.d = op->d;
    a.watermark = watermark;
    a.cap_s = op->cap_s;
    a.state = op->state;
    a.n_s = op->n_s;
    a.min_end = op->min_end;
    a.ctrl = op->ctrl;
    a.out_key = op->out_key;
    a.out_ws = op->out_ws;
    a.out_we = op->out_we;
    a.ad = op->ad;
    for (int g = 0; g < op->n_out; g++) a.out_val[g] = op->out_val[g];
    a.out_null = op->out_null;
    a.out_cap = op->out_cap;
    a.lateness = op->lateness;
    a.prev_wm = op->prev_wm;
    a.min_fire = op->min_fire;
    return a;
}

// (a dynamic-gap handle runs the static instance: sessions carry their ends, no gap is read)
static int sw_advance_launch(SessionOp* op, bool dev, const SwAdvArgs& a) {
    sw_dispatch(op->nw_t, false, dev, op->late, [&](auto inst) {
        using I = decltype(inst);
        hipLaunchKernelGGL((k_sw_advance<I::nw, I::dev, I::late>), dim3(op->ks.n_sb), dim3(SW_TILE), 0, op->stream, a);
    });
    FD_TRY(hipGetLastError());
    return FW_OK;
}

int sw_advance(SessionOp* op, int64_t watermark, int64_t prev_watermark) {
    SwAdvArgs a = sw_adv_args(op, watermark);
    a.prev_watermark = prev_watermark;  // (read by the lateness instances alone)
    return sw_advance_launch(op, false, a);
}

int sw_advance_device(SessionOp* op, const int64_t* d_watermark, int64_t watermark) {
    op->wm_dev = true;
    if (op->late) hipLaunchKernelGGL(k_sw_raise_late, dim3(1), dim3(1), 0, op->stream, op->ctrl, d_watermark, watermark, op->prev_wm);
    else hipLaunchKernelGGL(k_sw_raise, dim3(1), dim3(1), 0, op->stream, op->ctrl, d_watermark, watermark);
    return sw_advance_launch(op, true, sw_adv_args(op, 0));
}

int sw_read_watermark(SessionOp* op, int64_t* watermark) {
    FD_TRY(hipMemcpyAsync(watermark, &op->ctrl->cur, sizeof(int64_t), hipMemcpyDeviceToHost, op->stream));
    FD_TRY(hipStreamSynchronize(op->stream));
    return FW_OK;
}

// ---- checkpoint: the library's own blob.  Entries are (key, start, end, acc[nw_t], key group << 32 |
// sub-bucket) in no particular order (nw_t = 1 for a DataStream handle: five words, as ever): a
// restore routes every key again (precomputed-hash keys carry no hash in the state, so they are
// placed by the recorded sub-bucket and may not be split finer than the snapshot's) and sorts each
// superbucket's list.
namespace {
struct SwHeader {
    uint64_t magic;
    int64_t push_seq;   // at byte 8 of both blobs (runtime/handle.py _snapshot_push_seq)
    int64_t watermark;
    uint64_t fingerprint;
    int32_t key_group, sb_log2;
    int64_t n;
};
const uint64_t SW_MAGIC = 0x464c4b5753573031ull;     // "FLKWSW01"
const uint64_t SW_KG_MAGIC = 0x464c4b5753473031ull;  // "FLKWSG01"
constexpr int SW_MAX_BLOB_WORDS = 3 + SW_MAX_NW + 1;
}  // namespace

int sw_snapshot(SessionOp* op, int64_t watermark, int32_t key_group, void* buf, int64_t capacity, int64_t* size) {
    const KeySpace& ks = op->ks;
    const int L = ks.sb_per_kg_log2;
    int sb0 = 0, sb1 = ks.n_sb, rc = 0;
    if (key_group >= 0 && (rc = fd_sb_range(ks, key_group, &sb0, &sb1))) return rc;
    FD_TRY(hipStreamSynchronize(op->stream));
    std::vector<int32_t> cnt(sb1 - sb0);
    FD_TRY(hipMemcpy(cnt.data(), op->n_s + sb0, cnt.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> ent, tmp;
    const int SWS = sw_stride(op->nw_t);
    int64_t n = 0;
    for (int sb = sb0; sb < sb1; sb++) {
        const int c = cnt[sb - sb0];
        if (c <= 0) continue;
        tmp.resize((size_t)c * SWS);
        FD_TRY(hipMemcpy(tmp.data(), op->state + (size_t)sb * op->cap_s * SWS, tmp.size() * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < c; i++) {
            ent.insert(ent.end(), tmp.begin() + (size_t)i * SWS, tmp.begin() + (size_t)(i + 1) * SWS);
            ent.push_back((uint64_t)(ks.kg_start + (sb >> L)) << 32 | (uint32_t)(sb & ((1 << L) - 1)));
            n++;
        }
    }
    const int64_t need = (int64_t)sizeof(SwHeader) + (int64_t)ent.size() * 8;
    *size = need;
    if (!buf) return FW_OK;
    if (capacity < need) return set_error(FW_E_INVALID, "snapshot buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    SwHeader hd{key_group >= 0 ? SW_KG_MAGIC : SW_MAGIC, op->push_seq, watermark, op->fingerprint, key_group, L, n};
    memcpy(buf, &hd, sizeof hd);
    if (!ent.empty()) memcpy((char*)buf + sizeof hd, ent.data(), ent.size() * 8);
    return FW_OK;
}

int sw_restore(SessionOp* op, bool key_group, const void* buf, int64_t size, int64_t* watermark) {
    SwHeader hd;
    if (size < (int64_t)sizeof hd) return set_error(FW_E_INVALID, "session-window snapshot truncated");
    memcpy(&hd, buf, sizeof hd);
    const KeySpace& ks = op->ks;
    const int L = ks.sb_per_kg_log2;
    const int NW = op->nw_t, SWS = sw_stride(NW), SW_BLOB_WORDS = SWS + 1;
    if (hd.magic != (key_group ? SW_KG_MAGIC : SW_MAGIC))
        return set_error(FW_E_INVALID, "not a session-window %ssnapshot", key_group ? "key-group " : "");
    if (hd.fingerprint != op->fingerprint) return set_error(FW_E_INVALID, "session-window snapshot of a different operator configuration");
    // lateness: which of a blob's sessions have fired is read off its watermark, so a key group joins
    // only a handle that stands at that watermark (fw_initialize_watermark sets it for a rescaled restore)
    if (op->late && key_group && hd.watermark != *watermark)
        return set_error(FW_E_STATE, "session windows with lateness: key group %d was snapshotted at watermark %lld, this subtask "
                                     "stands at %lld (fw_initialize_watermark before the first key group)",
                         hd.key_group, (long long)hd.watermark, (long long)*watermark);
    if (hd.n < 0 || size < (int64_t)sizeof hd + hd.n * SW_BLOB_WORDS * 8) return set_error(FW_E_INVALID, "session-window snapshot truncated");
    if (ks.hash_kind == KH_PRE && L > hd.sb_log2)
        return set_error(FW_E_INVALID, "precomputed-hash keys cannot be split finer than the snapshot's sub-buckets");
    int sb0 = 0, sb1 = ks.n_sb, rc = 0;
    if (key_group && (rc = fd_sb_range(ks, hd.key_group, &sb0, &sb1))) return rc;
    FD_TRY(hipStreamSynchronize(op->stream));
    std::vector<int32_t> cnt(sb1 - sb0, 0);
    if (key_group) {
        FD_TRY(hipMemcpy(cnt.data(), op->n_s + sb0, cnt.size() * 4, hipMemcpyDeviceToHost));
        for (int32_t c : cnt)
            if (c != 0) return set_error(FW_E_STATE, "key group %d already holds state in this subtask", hd.key_group);
    }
    struct Ent {
        uint64_t key;
        int64_t start, end;
        uint64_t acc[SW_MAX_NW];
    };
    std::vector<std::vector<Ent>> per(sb1 - sb0);
    const uint64_t* src = (const uint64_t*)((const char*)buf + sizeof hd);
    for (int64_t i = 0; i < hd.n; i++) {
        uint64_t e[SW_MAX_BLOB_WORDS];
        memcpy(e, src + (size_t)i * SW_BLOB_WORDS, (size_t)SW_BLOB_WORDS * 8);
        int sb;
        if ((rc = fd_restore_sb(ks, (int64_t)e[0], e[SWS], sb0, sb1, &sb))) return rc;
        Ent en{e[0], (int64_t)e[1], (int64_t)e[2], {}};
        for (int w = 0; w < NW; w++) en.acc[w] = e[3 + w];
        per[sb - sb0].push_back(en);
    }
    std::vector<uint64_t> tmp;
    std::vector<int64_t> mins(sb1 - sb0, INT64_MAX), minf(sb1 - sb0, INT64_MAX);
    for (int sb = sb0; sb < sb1; sb++) {
        std::vector<Ent>& v = per[sb - sb0];
        if ((int64_t)v.size() > op->cap_s)
            return set_error(FW_E_CAPACITY, "restored state exceeds the session list (%d sessions per superbucket)", op->cap_s);
        std::sort(v.begin(), v.end(), [](const Ent& x, const Ent& y) { return x.key != y.key ? x.key < y.key : x.start < y.start; });
        tmp.clear();
        for (const Ent& x : v) {
            tmp.push_back(x.key);
            tmp.push_back((uint64_t)x.start);
            tmp.push_back((uint64_t)x.end);
            for (int w = 0; w < NW; w++) tmp.push_back(x.acc[w]);
            mins[sb - sb0] = std::min(mins[sb - sb0], x.end);
            if (!session_due(x.end, hd.watermark)) minf[sb - sb0] = std::min(minf[sb - sb0], x.end);
        }
        cnt[sb - sb0] = (int32_t)v.size();
        if (!tmp.empty())
            FD_TRY(hipMemcpy(op->state + (size_t)sb * op->cap_s * SWS, tmp.data(), tmp.size() * 8, hipMemcpyHostToDevice));
    }
    FD_TRY(hipMemcpy(op->n_s + sb0, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
    FD_TRY(hipMemcpy(op->min_end + sb0, mins.data(), mins.size() * 8, hipMemcpyHostToDevice));
    if (op->late) FD_TRY(hipMemcpy(op->min_fire + sb0, minf.data(), minf.size() * 8, hipMemcpyHostToDevice));
    Ctrl c;
    if ((rc = fd_restored_ctrl(op->ctrl, key_group, hd.n, hd.watermark, &c))) return rc;
    op->push_seq = key_group ? std::max(op->push_seq, hd.push_seq) : hd.push_seq;
    if (!key_group) {
        c.n_side = 0;
        *watermark = hd.watermark;
    }
    FD_TRY(hipMemcpy(op->ctrl, &c, sizeof c, hipMemcpyHostToDevice));
    return FW_OK;
}

}  // namespace fw
