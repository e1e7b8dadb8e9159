// fw_count.hip -- the count-window path (fw_count.h): kernels and the per-handle host code.
//
// One push is folded into the key table when it is pushed: the folded paths' stable superbucket
// partition (fd_partition, fw_folded.hip: four stream-ordered launches), then
//   k_cw_fold     one workgroup per superbucket walks its segment in arrival order, a tile at a time
// No workgroup waits on another: the only cross-workgroup traffic is counters (atomic adds).
// Behind the N > 1 keyBy exchange (cw_push_segments) the partition is fd_partition_segments over the
// padded receive buffer and the fold the strided instance k_cw_fold<true, false>; buffer position order is
// the arrival order.
// A record handle (FW_WIN_COUNT_RECORD) launches k_cw_fold<false, true>: the same body with an ordinal
// beside every value word -- in the scan, the fire loop and the write-back -- and the retain / release
// events of the ordinals the ring holds.  Behind the exchange (cw_push_record_segments) it is
// k_cw_fold<true, true>, and k_cw_gather_rec copies the record rows the events and results name out of
// the receive buffer (cw_record_rows), so the buffer itself never crosses to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "fw_count.h"

namespace fw {
namespace {

struct CwFoldArgs {
    const int64_t* key;
    const uint64_t* val;
    const uint32_t* perm;
    const int32_t* seg;
    CountDesc d;
    int32_t cap_e, pwe, is_count, vtype;
    uint64_t* table;
    Ctrl* ctrl;
    int64_t* out_key;
    int64_t* out_ws;
    int64_t* out_we;
    uint64_t* out_val;
    int64_t* out_ord;
    int64_t out_cap;
    int64_t ord_base;  // push_seq << 32 | row offset of this launch within its call
    int32_t stride;    // the device form (DEV): key and value word of row r at key[r * stride], val[r * stride]
};
// the record instance (REC) takes these on top; the other instances keep CwFoldArgs as their whole argument
struct CwRecFoldArgs : CwFoldArgs {
    int32_t mode;  // CountRecMode
    uint64_t* out_rord;
    int64_t* ordev;
    int64_t ordev_cap;
};
template <bool REC>
using CwArgs = std::conditional_t<REC, CwRecFoldArgs, CwFoldArgs>;

// what the record instance keeps in LDS on top of the one body's; the other instances hold nothing
template <bool REC>
struct CwRecLds {};
template <>
struct CwRecLds<true> {
    uint32_t n_ev;  // the tile's retain / release events
    unsigned long long ev_base;
};

// DEV: the device form, behind the N > 1 keyBy exchange (cw_push_segments): perm / seg name the live
// rows fd_partition_segments selected from a padded receive buffer -- a padding row is in no segment,
// so it is never read -- and a row's words are strided (1: columns, row_words: packed rows).  Everything
// else is the one body; the instance without DEV is the one a direct push launches.
// REC: the record instance.  A value word stays raw (count_record_fold compares a DOUBLE through dkey),
// a row's ordinal is ord_base + its row index, a ring slot's ordinal lies R words behind its value.
#define CW_AT(row) (DEV ? (size_t)(row) * (size_t)a.stride : (row))
template <bool DEV, bool REC>
__global__ __launch_bounds__(CW_TILE) void k_cw_fold(CwArgs<REC> a) {
    __shared__ uint64_t sk[CW_TILE];     // sorted keys
    __shared__ uint32_t sp[CW_TILE];     // their positions in the tile (arrival order)
    __shared__ uint64_t pv[CW_TILE];     // by position: value word, row index
    __shared__ uint32_t prow[CW_TILE];
    __shared__ uint64_t sv[CW_TILE];     // segmented scan over (key, slice) runs
    __shared__ uint32_t sf[CW_TILE];
    __shared__ int32_t hx[CW_TILE];      // sorted index of the row's key run head
    __shared__ int32_t hslot[CW_TILE];   // by head: table slot (-1: table full), count before the tile, run length
    __shared__ int64_t hc0[CW_TILE];
    __shared__ int32_t hlen[CW_TILE];
    __shared__ uint32_t n_fire, n_new;
    __shared__ unsigned long long fire_base;
    __shared__ CwRecLds<REC> rl;
    // REC: the ordinal beside sv[].  pv[] is dead once the scan has taken its values, so it holds them.
    [[maybe_unused]] uint64_t(&so)[CW_TILE] = pv;

    const int t = threadIdx.x;
    const CountDesc& d = a.d;
    const int op = d.op, R = d.R, pwe = a.pwe;
    const uint32_t mask = (uint32_t)a.cap_e - 1u;
    const int64_t seg0 = a.seg[blockIdx.x], seg1 = a.seg[blockIdx.x + 1];
    uint64_t* tab = a.table + (size_t)blockIdx.x * a.cap_e * pwe;
    const bool dbl_cmp = !REC && a.vtype == FW_T_F64 && (op == CW_MIN || op == CW_MAX);
    [[maybe_unused]] const bool dbl = a.vtype == FW_T_F64;

    for (int64_t base = seg0; base < seg1; base += CW_TILE) {
        const int nt = (int)(seg1 - base < CW_TILE ? seg1 - base : CW_TILE);
        const int n2 = fd_pow2(nt);
        if (t == 0) {
            n_fire = 0;
            n_new = 0;
            if constexpr (REC) rl.n_ev = 0;
        }
        if (t < nt) {
            const uint32_t row = a.perm[base + t];
            uint64_t v = a.is_count ? 1ull : a.val[CW_AT(row)];
            if (dbl_cmp) v = (uint64_t)dkey(v);
            sk[t] = (uint64_t)a.key[CW_AT(row)];
            sp[t] = (uint32_t)t;
            pv[t] = v;
            prow[t] = row;
        } else {
            sk[t] = ~0ull;
            sp[t] = FD_PAD | (uint32_t)t;
        }
        __syncthreads();
        fd_sort(sk, sp, n2);
        const bool valid = t < nt;  // the padding sorted behind the rows
        const bool head = valid && (t == 0 || sk[t - 1] != sk[t]);
        hx[t] = head ? t : 0;
        __syncthreads();
        fd_max_scan(hx, n2);

        // ---- the key's table slot: look every distinct key up, then insert the new ones
        int32_t slot = -1;
        int64_t cnt0 = 0;
        bool ins = false;
        const int64_t mykey = (int64_t)sk[t];
        if (head) {
            uint32_t e = count_slot_hash(mykey, mask);
            for (int p = 0; p < a.cap_e; p++, e = (e + 1) & mask) {
                const int64_t c = (int64_t)tab[(size_t)e * pwe + 1];
                if (c == 0) {
                    ins = true;
                    break;
                }
                if ((int64_t)tab[(size_t)e * pwe] == mykey) {
                    slot = (int32_t)e;
                    cnt0 = c;
                    break;
                }
            }
        }
        __syncthreads();
        if (head && ins) {  // the heads' keys are distinct: a slot another head claimed is just occupied
            uint32_t e = count_slot_hash(mykey, mask);
            for (int p = 0; p < a.cap_e; p++, e = (e + 1) & mask) {
                const unsigned long long old = atomicCAS((unsigned long long*)&tab[(size_t)e * pwe + 1], 0ull,
                                                         (unsigned long long)CW_CLAIMED);
                if (old == 0ull) {
                    tab[(size_t)e * pwe] = (uint64_t)mykey;
                    slot = (int32_t)e;
                    cnt0 = 0;
                    atomicAdd(&n_new, 1u);
                    break;
                }
            }
        }
        if (head) {
            if (slot < 0) atomicOr(&a.ctrl->error, ERR_STATE);  // table full: the key's rows are dropped
            hslot[t] = slot;
            hc0[t] = cnt0;
        }
        if (valid && (t == nt - 1 || sk[t + 1] != sk[t])) hlen[hx[t]] = t - hx[t] + 1;
        __syncthreads();

        // ---- per row: its per-key index and count slice; segmented scan over (key, slice) runs
        const int hi = valid ? hx[t] : 0;
        slot = valid ? hslot[hi] : -1;
        cnt0 = valid ? hc0[hi] : 0;
        const bool live = valid && slot >= 0;
        const int rank = t - hi;
        const int64_t idx = cnt0 + rank;
        int64_t sl = 0, ws = 0;
        int32_t rs = 0, fires = 0, ns = 0;
        if (valid) count_step(d, idx, &sl, &rs, &fires, &ws, &ns);
        const int64_t s0k = (int64_t)udiv((uint64_t)cnt0, d.g_div);  // the key's first slice in this tile
        const bool partial0 = cnt0 - s0k * d.g != 0;                 // ... began before the tile
        if (t < n2) {
            sv[t] = valid ? pv[sp[t]] : 0;
            sf[t] = (!valid || rank == 0 || idx - sl * d.g == 0) ? 1u : 0u;
        }
        if constexpr (REC) {
            __syncthreads();  // every pv[] read above is done
            if (t < n2) so[t] = valid ? (uint64_t)a.ord_base + prow[sp[t]] : 0;
        }
        __syncthreads();
        for (int dd = 1; dd < n2; dd <<= 1) {
            const bool take = t < n2 && t >= dd && !sf[t];
            uint64_t ov = 0;
            [[maybe_unused]] uint64_t oo = 0;
            uint32_t of = 0;
            if (take) {
                ov = sv[t - dd];
                of = sf[t - dd];
                if constexpr (REC) oo = so[t - dd];
            }
            __syncthreads();
            if (take) {
                if constexpr (REC) {
                    uint64_t rv, ro;
                    count_record_fold(op, a.mode, dbl, ov, oo, sv[t], so[t], &rv, &ro);
                    sv[t] = rv;
                    so[t] = ro;
                } else {
                    sv[t] = count_fold(op, ov, sv[t]);
                }
                sf[t] = of;
            }
            __syncthreads();
        }

        // ---- fires: the window's slices oldest first; older ones from the ring as it stood before
        // the tile, the tile's own from the scan (the last row of slice j of this key run)
        const bool fire = live && fires;
        uint64_t acc = 0;
        [[maybe_unused]] uint64_t acc_o = 0;  // (acc_o: REC, the ordinal of the record the row is built from)
        uint32_t loc = 0;
        if (fire) {
            bool first = true;
            for (int k = ns - 1; k >= 0; k--) {
                const int64_t j = sl - k;
                int rj = rs - k % R;
                if (rj < 0) rj += R;
                uint64_t part;
                [[maybe_unused]] uint64_t part_o = 0;
                if (j < s0k) {
                    part = tab[(size_t)slot * pwe + 2 + rj];
                    if constexpr (REC) part_o = tab[(size_t)slot * pwe + 2 + R + rj];
                } else {
                    const int at = hi + (int)((j + 1) * d.g - 1 - cnt0);
                    part = sv[at];
                    if constexpr (REC) {
                        part_o = so[at];
                        if (j == s0k && partial0)
                            count_record_fold(op, a.mode, dbl, tab[(size_t)slot * pwe + 2 + rj], tab[(size_t)slot * pwe + 2 + R + rj],
                                              part, part_o, &part, &part_o);
                    } else {
                        if (j == s0k && partial0) part = count_fold(op, tab[(size_t)slot * pwe + 2 + rj], part);
                    }
                }
                if constexpr (REC) {
                    if (first) {
                        acc = part;
                        acc_o = part_o;
                    } else {
                        count_record_fold(op, a.mode, dbl, acc, acc_o, part, part_o, &acc, &acc_o);
                    }
                } else {
                    acc = first ? part : count_fold(op, acc, part);
                }
                first = false;
            }
            loc = atomicAdd(&n_fire, 1u);
        }
        __syncthreads();
        if (t == 0) {
            if (n_fire) {
                fire_base = atomicAdd((unsigned long long*)&a.ctrl->out_count[0], (unsigned long long)n_fire);
                atomicAdd((unsigned long long*)&a.ctrl->fired, (unsigned long long)n_fire);
            }
            if (n_new) atomicAdd((unsigned long long*)&a.ctrl->live_entries, (unsigned long long)n_new);
        }
        __syncthreads();
        if (fire) {
            const unsigned long long o = fire_base + loc;
            if (o < (unsigned long long)a.out_cap) {
                uint64_t r = acc;
                if (dbl_cmp) r = dkey_inv((int64_t)acc);
                else if (a.vtype == FW_T_I32 && !a.is_count && op == CW_ADD_I) r = (uint64_t)(int64_t)(int32_t)(uint32_t)acc;
                a.out_key[o] = mykey;
                a.out_val[o] = r;
                a.out_ws[o] = ws;
                a.out_we[o] = idx + 1;
                a.out_ord[o] = a.ord_base + (int64_t)prow[sp[t]];
                if constexpr (REC) a.out_rord[o] = acc_o;
            } else {
                atomicOr(&a.ctrl->error, ERR_OUTPUT);
            }
        }

        // ---- write back (every ring read of the fires is behind the barriers above): the last row
        // of each (key, slice) run stores the slice, unless a later slice of the tile took its slot
        [[maybe_unused]] int64_t ev[2] = {0, 0};  // REC: this row's events
        [[maybe_unused]] uint32_t n_ev = 0;
        if (live) {
            const int len = hlen[hi];
            const int64_t s_last = (int64_t)udiv((uint64_t)(cnt0 + len - 1), d.g_div);
            const bool slice_end = rank == len - 1 || idx + 1 == (sl + 1) * d.g;
            if (slice_end && sl + R > s_last) {
                uint64_t part = sv[t];
                if constexpr (REC) {
                    uint64_t part_o = so[t];
                    const uint64_t old_o = tab[(size_t)slot * pwe + 2 + R + rs];
                    if (sl == s0k && partial0)
                        count_record_fold(op, a.mode, dbl, tab[(size_t)slot * pwe + 2 + rs], old_o, part, part_o, &part, &part_o);
                    tab[(size_t)slot * pwe + 2 + R + rs] = part_o;
                    // What the slot held before the tile, from the counts alone: the key's slices then
                    // were [max(0, q - R + 1), q] with q = (cnt0 - 1) / g, each in its own slot, so slot rs
                    // held the one slice of them congruent to rs -- this slice begun earlier, or an older
                    // one this store evicts -- unless that slice would lie below 0.
                    bool held = false;
                    if (cnt0 > 0) {
                        const uint64_t q = udiv((uint64_t)(cnt0 - 1), d.g_div);
                        int back = (int)(q - udiv(q, d.r_div) * (uint64_t)R) - rs;
                        if (back < 0) back += R;
                        held = (int64_t)q - back >= 0;
                    }
                    if (!held) {
                        ev[0] = (int64_t)part_o;
                        n_ev = 1;
                    } else if (old_o != part_o) {
                        ev[0] = ORDEV_RELEASE | (int64_t)old_o;
                        ev[1] = (int64_t)part_o;
                        n_ev = 2;
                    }
                } else {
                    if (sl == s0k && partial0) part = count_fold(op, tab[(size_t)slot * pwe + 2 + rs], part);
                }
                tab[(size_t)slot * pwe + 2 + rs] = part;
            }
            if (rank == len - 1) tab[(size_t)slot * pwe + 1] = (uint64_t)(cnt0 + len);
        }
        if constexpr (REC) {  // one claim of the event buffer per tile
            const uint32_t at = n_ev ? atomicAdd(&rl.n_ev, n_ev) : 0u;
            __syncthreads();
            if (t == 0 && rl.n_ev) rl.ev_base = atomicAdd((unsigned long long*)&a.ctrl->n_ordev, (unsigned long long)rl.n_ev);
            __syncthreads();
            for (uint32_t i = 0; i < n_ev; i++) {
                const unsigned long long o = rl.ev_base + at + i;
                if (o < (unsigned long long)a.ordev_cap) a.ordev[o] = ev[i];
                else atomicOr(&a.ctrl->error, ERR_ORDEV);
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

// The payload words (words 2 .. 2 + F of a packed row) of the rows a record push's events and results
// name, gathered beside the event list and the result list: event i's words at ev_words[i * F ..],
// result j's at res_words[j * F ..].  A release event and an ordinal of another push (or one whose
// position is not below n_rows: the host refuses the call) get no words.  The counts are read from
// Ctrl here, so the host launches without knowing them; the loop is bounded by the two capacities.
struct CwGatherArgs {
    const Ctrl* ctrl;
    const int64_t* ordev;
    int64_t ordev_cap;
    const uint64_t* out_rord;
    int64_t out_cap;
    const uint64_t* rows;
    int32_t row_words, F;
    int64_t n_rows;
    uint64_t seq;  // push_seq of the push the buffer belongs to
    uint64_t* ev_words;
    uint64_t* res_words;
};
constexpr int CW_GATHER_THREADS = 256;
__global__ __launch_bounds__(CW_GATHER_THREADS) void k_cw_gather_rec(CwGatherArgs a) {
    const unsigned long long n_ordev = a.ctrl->n_ordev, n_out = a.ctrl->out_count[0];
    const int64_t n_ev = (int64_t)(n_ordev < (unsigned long long)a.ordev_cap ? n_ordev : (unsigned long long)a.ordev_cap);
    const int64_t n_res = (int64_t)(n_out < (unsigned long long)a.out_cap ? n_out : (unsigned long long)a.out_cap);
    const int64_t total = a.ordev_cap + a.out_cap;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const bool is_ev = i < a.ordev_cap;
        const int64_t j = is_ev ? i : i - a.ordev_cap;
        if (j >= (is_ev ? n_ev : n_res)) continue;
        const uint64_t o = is_ev ? (uint64_t)a.ordev[j] : a.out_rord[j];  // (a release has its top bit set: no push_seq matches)
        const uint64_t pos = o & 0xffffffffull;
        if ((o >> 32) != a.seq || pos >= (uint64_t)a.n_rows) continue;
        const uint64_t* src = a.rows + (size_t)pos * (size_t)a.row_words + 2;
        uint64_t* dst = (is_ev ? a.ev_words : a.res_words) + (size_t)j * (size_t)a.F;
        for (int f = 0; f < a.F; f++) dst[f] = src[f];
    }
}

int64_t cw_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

int cw_plan(const fw_config& c, CountOp* op) {
    const bool rec = c.window_kind == FW_WIN_COUNT_RECORD;
    if (c.api != FW_API_DATASTREAM)
        return set_error(FW_E_INVALID, "%s (countWindow) is a DataStream window: api must be FW_API_DATASTREAM",
                         rec ? "FW_WIN_COUNT_RECORD" : "FW_WIN_COUNT");
    if (c.n_aggs != 1) return set_error(FW_E_INVALID, "count windows take one aggregation (n_aggs == 1), got %d", c.n_aggs);
    const fw_agg_desc& g = c.aggs[0];
    const bool by = g.kind == FW_AGG_MINBY || g.kind == FW_AGG_MAXBY;
    if (rec) {
        if (g.kind == FW_AGG_COUNT_STAR)
            return set_error(FW_E_INVALID, "record count windows: aggs[0].kind FW_AGG_COUNT_STAR has no record-shaped form (DataStream has no such count)");
        if (g.kind != FW_AGG_SUM && g.kind != FW_AGG_MIN && g.kind != FW_AGG_MAX && !by)
            return set_error(FW_E_INVALID, "record count windows: aggs[0].kind %d is not sum / min / max / minBy / maxBy", g.kind);
        if (g.flags & ~FW_AGGF_LAST) return set_error(FW_E_INVALID, "record count windows: bad aggs[0].flags %d", g.flags);
        if (g.flags && !by)
            return set_error(FW_E_INVALID, "record count windows: aggs[0].flags FW_AGGF_LAST is the tie rule of minBy / maxBy only");
        if (!c.ds_first_ordinals)
            return set_error(FW_E_INVALID, "record count windows name their records by arrival ordinal (ds_first_ordinals must be 1)");
    } else {
        if (by) return set_error(FW_E_INVALID, "count windows: minBy / maxBy run on the reference operator");
        if (g.kind != FW_AGG_SUM && g.kind != FW_AGG_MIN && g.kind != FW_AGG_MAX && g.kind != FW_AGG_COUNT_STAR)
            return set_error(FW_E_INVALID, "count windows: aggregate kind %d is not sum / min / max / count", g.kind);
        if (g.flags) return set_error(FW_E_INVALID, "count windows: bad aggregate flags %d", g.flags);
    }
    if (g.type != FW_T_I64 && g.type != FW_T_I32 && g.type != FW_T_F64)
        return set_error(FW_E_INVALID, "count windows: bad aggregate type %d", g.type);
    op->is_count = g.kind == FW_AGG_COUNT_STAR;
    if (!op->is_count) {
        if (g.input_col < 0 || g.input_col >= c.n_value_cols) return set_error(FW_E_INVALID, "count windows: bad input_col");
        if (c.value_col_types[g.input_col] != g.type)
            return set_error(FW_E_INVALID, "count windows: type does not match value column type");
    }
    if (c.size_ms < 1) return set_error(FW_E_INVALID, "count window size must be >= 1");
    if (c.slide_ms < 0) return set_error(FW_E_INVALID, "count window slide must be >= 1");
    const int64_t size = c.size_ms, slide = c.slide_ms ? c.slide_ms : c.size_ms;
    const int64_t gg = cw_gcd(size, slide);
    if (size / gg > FW_COUNT_MAX_SLICES)
        return set_error(FW_E_INVALID, "count window size / gcd(size, slide) = %lld exceeds FW_COUNT_MAX_SLICES (%d)",
                         (long long)(size / gg), FW_COUNT_MAX_SLICES);
    if (c.offset_ms != 0) return set_error(FW_E_INVALID, "count windows have no offset (offset_ms must be 0)");
    if (c.allowed_lateness_ms != 0) return set_error(FW_E_INVALID, "count windows have no lateness (allowed_lateness_ms must be 0)");
    if (c.late_side_output) return set_error(FW_E_INVALID, "count windows have no late elements (late_side_output must be 0)");
    if (c.ds_first_ordinals && !rec) return set_error(FW_E_INVALID, "count windows are (key, aggregate) shaped (ds_first_ordinals must be 0)");
    if (c.nullable_cols) return set_error(FW_E_INVALID, "count windows take no NULL inputs (nullable_cols must be 0)");
    if (c.tz_n != 0) return set_error(FW_E_INVALID, "count windows have no time zone (tz_n must be 0)");
    if (c.agg_phase != FW_PHASE_ONE) return set_error(FW_E_INVALID, "count windows are one-phase (agg_phase must be FW_PHASE_ONE)");
    if (c.key_hash != FW_KEYHASH_LONG && c.key_hash != FW_KEYHASH_INT && c.key_hash != FW_KEYHASH_PRECOMPUTED)
        return set_error(FW_E_INVALID, "count windows take LONG, INT or PRECOMPUTED keys (key_hash %d: KEYROW / BINROW keys are not supported)",
                         c.key_hash);
    if (c.max_batch_rows <= 0 || c.max_batch_rows >= (1ll << 31)) return set_error(FW_E_INVALID, "max_batch_rows must be in (0, 2^31)");
    if (c.output_capacity <= 0) return set_error(FW_E_INVALID, "output_capacity must be > 0");

    CountDesc& d = op->d;
    d.size = size;
    d.slide = slide;
    d.g = gg;
    d.R = (int32_t)(size / gg);
    d.g_div = make_udiv((uint64_t)gg);
    d.slide_div = make_udiv((uint64_t)slide);
    d.r_div = make_udiv((uint64_t)d.R);
    const bool f = g.type == FW_T_F64;
    d.op = op->is_count             ? CW_ADD_I
           : g.kind == FW_AGG_SUM ? (f ? CW_ADD_F : CW_ADD_I)
           : g.kind == FW_AGG_MIN || g.kind == FW_AGG_MINBY ? CW_MIN
                                                            : CW_MAX;
    op->vtype = g.type;
    op->val_col = op->is_count ? 0 : g.input_col;
    op->rec = rec;
    op->mode = !by ? CR_FIRST : (g.flags & FW_AGGF_LAST) ? CR_BY_LAST : CR_BY_FIRST;
    op->agg_sig = rec ? (g.kind << 8 | g.flags) : 0;
    op->pwe = rec ? 2 + 2 * d.R : 2 + d.R;
    op->ordev_cap = rec ? 2 * c.max_batch_rows : 0;

    KeySpace& ks = op->ks;
    const int rc = fd_plan_keyspace(c, "count windows", &ks, &op->part);
    if (rc) return rc;
    // <= 50% load at the hinted capacity
    const int64_t keys = std::max<int64_t>(c.state_capacity, 1024);
    const int64_t ce = fd_next_pow2(std::max<int64_t>(64, 2 * ((keys + ks.n_sb - 1) / ks.n_sb)));
    if (ce > (1ll << 24)) return set_error(FW_E_INVALID, "count windows: state_capacity too large per superbucket");
    op->cap_e = (int32_t)ce;
    op->out_cap = c.output_capacity;
    op->on = true;
    return FW_OK;
}

int cw_allocate(CountOp* op, hipStream_t stream, Ctrl* ctrl) {
    op->stream = stream;
    op->ctrl = ctrl;
    int rc;
    const size_t tw = (size_t)op->ks.n_sb * op->cap_e * op->pwe;
    if ((rc = fd_dalloc(&op->table, tw))) return rc;
    FD_TRY(hipMemsetAsync(op->table, 0, tw * 8, stream));
    if ((rc = fd_allocate(&op->part, op->ks))) return rc;
    const size_t oc = (size_t)op->out_cap;
    if ((rc = fd_dalloc(&op->out_key, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_ws, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_we, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_val, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_ord, oc))) return rc;
    if ((rc = fd_dalloc(&op->out_null, oc))) return rc;
    FD_TRY(hipMemsetAsync(op->out_null, 0, oc * 4, stream));
    if (op->rec) {
        if ((rc = fd_dalloc(&op->out_rord, oc))) return rc;
        if ((rc = fd_dalloc(&op->ordev, (size_t)op->ordev_cap))) return rc;
    }
    return FW_OK;
}

void cw_free(CountOp* op) {
    hipFree(op->table);
    fd_free(&op->part);
    hipFree(op->out_key);
    hipFree(op->out_ws);
    hipFree(op->out_we);
    hipFree(op->out_val);
    hipFree(op->out_ord);
    hipFree(op->out_null);
    hipFree(op->out_rord);
    hipFree(op->ordev);
    hipFree(op->g_ev);
    hipFree(op->g_res);
}

// the folds of one call: n rows at d_key[i * stride], d_val[i * stride], split into launches of
// part.cap_rows rows by position.  d_seg_counts: the rows are a padded buffer of segments of seg_len
// rows and the fold is the device form; else a direct push (stride 1)
// (rec_segments: a record handle's padded buffer, cw_push_record_segments -- one launch)
static int cw_fold_call(CountOp* op, int64_t n, const int64_t* d_key, const int32_t* d_khash, const uint64_t* d_val, int32_t stride,
                        const int64_t* d_seg_counts, int64_t seg_len, bool rec_segments = false) {
    if (n >= (1ll << 32) || op->push_seq >= (1ll << 30))
        return set_error(FW_E_INVALID, "arrival ordinals need < 2^32 rows per call and < 2^30 calls");
    if (op->rec && !rec_segments && (d_seg_counts || n > op->part.cap_rows))  // the event buffers hold one push of max_batch_rows rows
        return set_error(FW_E_INVALID, "record count windows: a push takes at most max_batch_rows (%lld) rows, as columns", (long long)op->part.cap_rows);
    hipStream_t s = op->stream;
    const int64_t cap_rows = op->part.cap_rows;
    for (int64_t o = 0; o < n; o += cap_rows) {
        const int64_t m = std::min(cap_rows, n - o);
        const int rc = d_seg_counts ? fd_partition_segments(op->part, op->ks, op->ctrl, s, m, d_key + o * stride, stride,
                                                            d_khash ? d_khash + o : nullptr, d_seg_counts, seg_len, o)
                                    : fd_partition(op->part, op->ks, op->ctrl, s, m, d_key + o, d_khash ? d_khash + o : nullptr);
        if (rc) return rc;
        CwRecFoldArgs fa{};
        fa.key = d_key + o * stride;
        fa.val = op->is_count ? nullptr : d_val + o * stride;
        fa.perm = op->part.perm;
        fa.seg = op->part.seg;
        fa.d = op->d;
        fa.cap_e = op->cap_e;
        fa.pwe = op->pwe;
        fa.is_count = op->is_count;
        fa.vtype = op->vtype;
        fa.table = op->table;
        fa.ctrl = op->ctrl;
        fa.out_key = op->out_key;
        fa.out_ws = op->out_ws;
        fa.out_we = op->out_we;
        fa.out_val = op->out_val;
        fa.out_ord = op->out_ord;
        fa.out_cap = op->out_cap;
        fa.ord_base = (op->push_seq << 32) + o;
        fa.stride = stride;
        fa.mode = op->mode;
        fa.out_rord = op->out_rord;
        fa.ordev = op->ordev;
        fa.ordev_cap = op->ordev_cap;
        if (op->rec && d_seg_counts) hipLaunchKernelGGL((k_cw_fold<true, true>), dim3(op->ks.n_sb), dim3(CW_TILE), 0, s, fa);
        else if (op->rec) hipLaunchKernelGGL((k_cw_fold<false, true>), dim3(op->ks.n_sb), dim3(CW_TILE), 0, s, fa);
        else if (d_seg_counts) hipLaunchKernelGGL((k_cw_fold<true, false>), dim3(op->ks.n_sb), dim3(CW_TILE), 0, s, (const CwFoldArgs&)fa);
        else hipLaunchKernelGGL((k_cw_fold<false, false>), dim3(op->ks.n_sb), dim3(CW_TILE), 0, s, (const CwFoldArgs&)fa);
        FD_TRY(hipGetLastError());
    }
    op->push_seq++;
    return FW_OK;
}

int cw_push(CountOp* op, int64_t n, const int64_t* d_key, const int32_t* d_khash, const uint64_t* d_val) {
    return cw_fold_call(op, n, d_key, d_khash, d_val, 1, nullptr, 0);
}

int cw_push_segments(CountOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_key,
                     const int32_t* d_khash, const uint64_t* d_val, int32_t stride) {
    return cw_fold_call(op, (int64_t)n_segs * seg_len, d_key, d_khash, d_val, stride, d_seg_counts, seg_len);
}

int cw_push_record_segments(CountOp* op, int32_t n_segs, int64_t seg_len, const int64_t* d_seg_counts, const int64_t* d_rows,
                            int32_t row_words) {
    const int64_t n = (int64_t)n_segs * seg_len;
    // one call is one launch: the event buffer holds what one push of max_batch_rows rows can raise,
    // and a retain must name a row of the current call
    if (n > op->part.cap_rows)
        return set_error(FW_E_INVALID, "fw_push_device_count_record_packed_segments: n_segs * seg_len = %lld exceeds max_batch_rows (%lld)",
                         (long long)n, (long long)op->part.cap_rows);
    return cw_fold_call(op, n, d_rows, nullptr, (const uint64_t*)d_rows + 2 + op->val_col, row_words, d_seg_counts, seg_len, true);
}

int cw_record_rows(CountOp* op, const int64_t* d_rows, int32_t row_words, int64_t n_rows, int32_t F) {
    int rc;
    if (!op->g_ev) {  // the first call of a handle behind an exchange; a handle pushed directly never pays
        if ((rc = fd_dalloc(&op->g_ev, (size_t)op->ordev_cap * F))) return rc;
        if ((rc = fd_dalloc(&op->g_res, (size_t)op->out_cap * F))) return rc;
    }
    CwGatherArgs ga{};
    ga.ctrl = op->ctrl;
    ga.ordev = op->ordev;
    ga.ordev_cap = op->ordev_cap;
    ga.out_rord = op->out_rord;
    ga.out_cap = op->out_cap;
    ga.rows = (const uint64_t*)d_rows;
    ga.row_words = row_words;
    ga.F = F;
    ga.n_rows = n_rows;
    ga.seq = (uint64_t)(op->push_seq - 1);
    ga.ev_words = op->g_ev;
    ga.res_words = op->g_res;
    const int64_t total = op->ordev_cap + op->out_cap;
    const int64_t blocks = std::min<int64_t>((total + CW_GATHER_THREADS - 1) / CW_GATHER_THREADS, 1024);
    hipLaunchKernelGGL(k_cw_gather_rec, dim3((unsigned)blocks), dim3(CW_GATHER_THREADS), 0, op->stream, ga);
    FD_TRY(hipGetLastError());
    return FW_OK;
}

// ---- checkpoint: the library's own blob.  Entries are (key, count, key group << 32 | sub-bucket,
// ring[R]); precomputed-hash keys carry no hash in the state, so they are placed by the recorded
// sub-bucket (a restore may not split them finer than the snapshot's), the others are routed again.
namespace {
struct CwHeader {
    uint64_t magic;
    int64_t push_seq;   // at byte 8 of both blobs (runtime/handle.py _snapshot_push_seq)
    int64_t watermark;
    int64_t size, slide;
    int32_t op, vtype, hash_kind, max_p;
    int32_t R, key_group, sb_log2, reserved;
    int64_t n;
};
const uint64_t CW_MAGIC = 0x464c4b5743573031ull;     // "FLKWCW01"
const uint64_t CW_KG_MAGIC = 0x464c4b57434b3031ull;  // "FLKWCK01"
// a record handle's blob: entries carry ord[R] behind ring[R], CwHeader::reserved the aggregate kind and
// tie flag (CountOp::agg_sig), so a blob crosses neither to FW_WIN_COUNT nor between tie rules
const uint64_t CW_REC_MAGIC = 0x464c4b5743523031ull;  // "FLKWCR01"
}  // namespace

int cw_snapshot(CountOp* op, int32_t key_group, void* buf, int64_t capacity, int64_t* size) {
    const KeySpace& ks = op->ks;
    const int L = ks.sb_per_kg_log2, pwe = op->pwe;
    int sb0 = 0, sb1 = ks.n_sb, rc = 0;
    if (key_group >= 0 && (rc = fd_sb_range(ks, key_group, &sb0, &sb1))) return rc;
    FD_TRY(hipStreamSynchronize(op->stream));
    const size_t words = (size_t)(sb1 - sb0) * op->cap_e * pwe;
    std::vector<uint64_t> tab(words);
    FD_TRY(hipMemcpy(tab.data(), op->table + (size_t)sb0 * op->cap_e * pwe, words * 8, hipMemcpyDeviceToHost));
    // the watermark of record: fw_advance_device leaves it in Ctrl::cur only, fw_advance in the host mirror only
    int64_t dev_wm = INT64_MIN;
    FD_TRY(hipMemcpy(&dev_wm, &op->ctrl->cur, sizeof dev_wm, hipMemcpyDeviceToHost));
    const int64_t watermark = std::max(op->watermark, dev_wm);
    std::vector<uint64_t> ent;
    int64_t n = 0;
    for (int sb = sb0; sb < sb1; sb++)
        for (int e = 0; e < op->cap_e; e++) {
            const uint64_t* p = tab.data() + ((size_t)(sb - sb0) * op->cap_e + e) * pwe;
            if (p[1] == 0) continue;
            ent.push_back(p[0]);
            ent.push_back(p[1]);
            ent.push_back((uint64_t)(ks.kg_start + (sb >> L)) << 32 | (uint32_t)(sb & ((1 << L) - 1)));
            ent.insert(ent.end(), p + 2, p + pwe);
            n++;
        }
    const int64_t need = (int64_t)sizeof(CwHeader) + (int64_t)ent.size() * 8;
    *size = need;
    if (!buf) return FW_OK;
    if (capacity < need) return set_error(FW_E_INVALID, "snapshot buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    CwHeader hd{op->rec ? CW_REC_MAGIC : key_group >= 0 ? CW_KG_MAGIC : CW_MAGIC, op->push_seq, watermark, op->d.size, op->d.slide, op->d.op,
                op->vtype, ks.hash_kind, ks.max_p, op->d.R, key_group, L, op->agg_sig, n};
    memcpy(buf, &hd, sizeof hd);
    if (!ent.empty()) memcpy((char*)buf + sizeof hd, ent.data(), ent.size() * 8);
    return FW_OK;
}

int cw_restore(CountOp* op, bool key_group, const void* buf, int64_t size) {
    CwHeader hd;
    if (size < (int64_t)sizeof hd) return set_error(FW_E_INVALID, "count-window snapshot truncated");
    memcpy(&hd, buf, sizeof hd);
    const KeySpace& ks = op->ks;
    const int L = ks.sb_per_kg_log2, pwe = op->pwe, bw = pwe + 1;
    if (op->rec && hd.magic != CW_REC_MAGIC) return set_error(FW_E_INVALID, "not a record count-window snapshot (FW_WIN_COUNT_RECORD)");
    if (!op->rec && hd.magic != (key_group ? CW_KG_MAGIC : CW_MAGIC)) return set_error(FW_E_INVALID, "not a count-window %ssnapshot", key_group ? "key-group " : "");
    if (hd.reserved != op->agg_sig)
        return set_error(FW_E_INVALID, "record count-window snapshot of another aggregate or tie rule (aggs[0].kind / flags)");
    if (hd.size != op->d.size || hd.slide != op->d.slide || hd.op != op->d.op || hd.vtype != op->vtype || hd.R != op->d.R ||
        hd.hash_kind != ks.hash_kind || hd.max_p != ks.max_p)
        return set_error(FW_E_INVALID, "count-window snapshot of a different operator configuration");
    if (hd.n < 0 || size < (int64_t)sizeof hd + hd.n * bw * 8) return set_error(FW_E_INVALID, "count-window snapshot truncated");
    if (ks.hash_kind == KH_PRE && L > hd.sb_log2)
        return set_error(FW_E_INVALID, "precomputed-hash keys cannot be split finer than the snapshot's sub-buckets");
    int sb0 = 0, sb1 = ks.n_sb, rc = 0;
    if (key_group && (rc = fd_sb_range(ks, hd.key_group, &sb0, &sb1))) return rc;
    FD_TRY(hipStreamSynchronize(op->stream));
    const size_t words = (size_t)(sb1 - sb0) * op->cap_e * pwe;
    std::vector<uint64_t> tab(words, 0);
    if (key_group) FD_TRY(hipMemcpy(tab.data(), op->table + (size_t)sb0 * op->cap_e * pwe, words * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> src((size_t)hd.n * bw);
    if (hd.n) memcpy(src.data(), (const char*)buf + sizeof hd, src.size() * 8);
    const uint32_t mask = (uint32_t)op->cap_e - 1u;
    for (int64_t i = 0; i < hd.n; i++) {
        const uint64_t* e = src.data() + (size_t)i * bw;
        const int kg = (int)(e[2] >> 32);
        int sb;
        if ((rc = fd_restore_sb(ks, (int64_t)e[0], e[2], sb0, sb1, &sb))) return rc;
        uint64_t* t = tab.data() + (size_t)(sb - sb0) * op->cap_e * pwe;
        uint32_t s = count_slot_hash((int64_t)e[0], mask);
        int p = 0;
        for (; p < op->cap_e; p++, s = (s + 1) & mask) {
            uint64_t* q = t + (size_t)s * pwe;
            if (q[1] == 0) {
                q[0] = e[0];
                q[1] = e[1];
                memcpy(q + 2, e + 3, (size_t)(pwe - 2) * 8);
                break;
            }
            if (q[0] == e[0]) return set_error(FW_E_STATE, "key group %d already holds state for a restored key", kg);
        }
        if (p == op->cap_e)
            return set_error(FW_E_CAPACITY, "restored state exceeds the key table (%d entries per superbucket)", op->cap_e);
    }
    FD_TRY(hipMemcpy(op->table + (size_t)sb0 * op->cap_e * pwe, tab.data(), words * 8, hipMemcpyHostToDevice));
    Ctrl c;
    if ((rc = fd_restored_ctrl(op->ctrl, key_group, hd.n, hd.watermark, &c))) return rc;
    op->push_seq = key_group ? std::max(op->push_seq, hd.push_seq) : hd.push_seq;
    if (!key_group) op->watermark = hd.watermark;
    if (op->rec) c.n_ordev = 0;  // the blob's ring is the state of record: the shim restores its retained records with it
    FD_TRY(hipMemcpy(op->ctrl, &c, sizeof c, hipMemcpyHostToDevice));
    return FW_OK;
}

}  // namespace fw
