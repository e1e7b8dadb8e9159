// fw_ingest_pack.h -- k_ingest_pack, the early-packing ingest of PF_PACK pushes, and its launcher
// (instantiated per key-hash kind in k_ingest_pack.hip).
#pragma once
#include "fw_kernel_common.h"

namespace fw {
// ======================================================================================
// k_ingest (fw_ingest_impl.h) carries a row's key, slice end and accumulator through its sort and
// its store stage because it serves every window kind, row format and hash kind: nine registers a
// row, 128 VGPRs and 78 KiB of LDS, two workgroups per CU.  A push of a SQL TUMBLE handle with one
// integer accumulator word, no NULLs, no precomputed hash and no LDS fold (Ctrl::fold_skip) finally
// stores one 8-B word per row (PF_PACK, fw_internal.h).  This kernel packs that word as soon as the
// row is routed: a routed row is the word and superbucket | rank, three registers, and the LDS holds
// the histogram, the run bookkeeping and a store stage of (word, destination) rows: at most 80 VGPRs
// and 39 KiB, three workgroups per CU, so one workgroup's column loads overlap the others' sorting
// and stores.
//
// Same chunks (4096 rows: 512 threads x 8 rows or 256 x 16, the template's geometry), same slot, cells, run claims, overflow flags, chunk statistics
// and last-workgroup commit as k_ingest, which the merge kernel and the next push read; it never folds
// and leaves Ctrl::fold_skip alone.  Whatever the packed word cannot hold makes the *chunk* slow: a
// rolled, one-row-per-thread loop that reloads the columns and writes PF_WIDE rows, sorted by
// superbucket, into the chunk's own region with their cell words and overflow flags -- what k_ingest
// writes for such a chunk of a PF_PACK push.  A launch that cannot pack at all (no valid PF_PACK
// fields yet, no watermark yet) sends every chunk that way.  The host's choice between the two
// kernels (fw_api.hip) therefore only costs time when it is wrong.
//
// What its scalar registers hold during the routing matters (loaded at the top, the later phases'
// pointers and strides and the rows' lane masks once spilled 110 of them through VGPR lanes inside
// the per-row code): it takes IngestPackArgs, the few fields of a push it reads, and reads what only
// the later phases need where they need it (`la` below).
//
// It does not fold, so it cannot measure the fold's yield as k_ingest does.  It estimates it: one
// row in eight (each thread's first) goes through a direct-mapped table of IGP_TAGS tags of
// (key hash, slice rank); a row that finds its own tag is a duplicate.  The last workgroup sets
// Ctrl::ig_skew when the push's duplicates reach one in IGP_SKEW_DEN sampled rows, and the host then
// has k_ingest fold and measure (fw_api.hip).
// ======================================================================================
constexpr int IGP_TAGS = 1024;      // tag table words (aliases the store stage, which the routing phase does not use)
constexpr int64_t IGP_SKEW_DEN = 8 * 50;  // duplicates * 8 * 50 >= sampled rows: an estimated fold yield of 2 %
static_assert(igp_stage_rows(IGP_MAX_SB) * 8 >= IGP_TAGS * 4, "the tag table fits the store stage");

// the kernel's parameter as the kernel argument segment holds it (its only parameter: offset 0)
typedef volatile __attribute__((address_space(4))) IngestPackArgs IgpLate;

__device__ __forceinline__ int64_t igp_slice_end(const IngestPackArgs& a, int64_t ts) {
    return wadd(window_start(ts, a.offset, a.slice_div), a.interval);
}
// the same for the phases that read their arguments late
struct IgpSlice {
    int64_t interval, offset;
    UDiv div;
};
__device__ __forceinline__ IgpSlice igp_slice_late(const IgpLate* la) {
    IgpSlice s;
    s.interval = la->interval;
    s.offset = la->offset;
    s.div.d = la->slice_div.d;
    s.div.magic = la->slice_div.magic;
    s.div.shift = la->slice_div.shift;
    s.div.add = la->slice_div.add;
    return s;
}
__device__ __forceinline__ int64_t igp_slice_end(const IgpSlice& s, int64_t ts) {
    return wadd(window_start(ts, s.offset, s.div), s.interval);
}
// route_key (fw_internal.h) on the launch's own copy of the key space
template <int HK>
__device__ __forceinline__ int32_t igp_route(const IngestPackArgs& a, int64_t key, uint32_t* m_out) {
    const uint32_t m = (uint32_t)flink_murmur_hash(java_key_hash(HK, key, 0));
    const uint32_t q = udiv32(m, a.maxp_div);
    const int32_t kg = (int32_t)(m - q * (uint32_t)a.max_p);
    *m_out = m;
    return ((kg - a.kg_start) << a.sb_log2) + (int32_t)(q & ((1u << a.sb_log2) - 1u));
}

// a routed row that is no partial: not this chunk's (past its end, another subtask's key, too far from
// the chunk's base), or late and counted as dropped.  (A partial's word is < 2^28.)
constexpr uint32_t IGP_NONE = 0xFFFFFFFFu, IGP_LATE = 0xFFFFFFFEu;
__device__ __forceinline__ bool igp_void(uint32_t r) { return (int32_t)r < 0; }

// the LDS behind the header and the histogram: rbound (u16), roff (u32), the store stage's words and
// destinations
struct IgpLds {
    uint16_t* rbound;
    uint32_t* roff;
    uint64_t* stage;  // 16-B aligned (igp_fixed_bytes)
    uint32_t* sdst;
    uint32_t wrows;
};
__device__ __forceinline__ IgpLds igp_lds(uint64_t* lds, int n_sb) {
    const int n_pad = (n_sb + 7) & ~7;
    IgpLds l;
    l.rbound = (uint16_t*)(lds + IG_HDR_WORDS + ig_hist_words(n_sb));
    l.roff = (uint32_t*)(l.rbound + n_pad);
    l.stage = (uint64_t*)(l.roff + n_pad);
    l.wrows = (uint32_t)igp_stage_rows(n_sb);
    l.sdst = (uint32_t*)(l.stage + l.wrows);
    return l;
}

// HK: the key-hash kind (KH_*, not KH_PRE), resolved per launch.  BLK threads x RPT rows, registers
// bounded for WAVES waves per SIMD: the geometry (fw_internal.h), resolved per launch (fw_api.hip)
template <int HK, int BLK, int RPT, int WAVES>
__global__ __launch_bounds__(BLK, WAVES) void k_ingest_pack(IngestPackArgs a) {
    constexpr int CH = BLK * RPT, NWV = BLK / 64, KMAX = igp_kmax(BLK);
    constexpr int AHEAD = IGP_AHEAD < RPT ? IGP_AHEAD : RPT;
    constexpr int PW = 3;  // words of a PF_WIDE row: key, slice end, one accumulator word
    static_assert(CH == IGP_BLOCK * IGP_RPT && CH <= 4096, "a chunk position and a superbucket share a 32-bit word");
    static_assert(BLK % 64 == 0 && NWV <= 8 && KMAX * BLK == IGP_MAX_SB, "wsum holds the waves' sums; the threads claim every superbucket");
    static_assert((RPT - AHEAD) % 2 == 0, "rows past the first AHEAD are loaded two at a time");
    static_assert(igp_stage_rows(IGP_MAX_SB) * 8 >= 10 * NWV * 8, "the last workgroup's reduction fits the stage");
    // dynamic LDS: [header 16 words][hist: n_sb u16][rbound: n_sb u16][roff: n_sb u32][stage words][stage destinations]
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    int64_t* s_min = (int64_t*)&lds[0];
    unsigned long long* s_drop = (unsigned long long*)&lds[1];
    uint32_t* s_samp = (uint32_t*)&lds[2];  // sampled rows, duplicates among them
    int32_t* s_last = (int32_t*)&lds[3];
    uint32_t* wsum = (uint32_t*)&lds[4];  // NWV words
    int64_t* s_pk = (int64_t*)&lds[12];   // key min / max, accumulator min / max of the chunk's partials
    uint16_t* hist = (uint16_t*)(lds + IG_HDR_WORDS);
    uint32_t* hist2 = (uint32_t*)hist;
    // what only the phases after the routing read comes from the kernel argument segment when it is
    // needed (volatile: not hoisted), so the routing phase's scalar registers do not hold it; the
    // rest of the LDS layout is one of those things (igp_lds below)
    const IgpLate* la = (const IgpLate*)__builtin_amdgcn_kernarg_segment_ptr();

    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    kt_start(a.kt);
    Ctrl* ctrl0 = a.ctrl;
    const int n_sb0 = a.n_sb;  // (pass_log2 == 0: ingest superbuckets are the state's)
    uint32_t* tags = (uint32_t*)igp_lds(lds, n_sb0).stage;  // [IGP_TAGS], until the store phase
    const int64_t slot = uni64(__hip_atomic_load(&ctrl0->pending_pushes, __ATOMIC_RELAXED, DEV_SCOPE));
    const int64_t cur_wm = uni64(__hip_atomic_load(&ctrl0->cur, __ATOMIC_RELAXED, DEV_SCOPE));
    // the epoch's first push (slot 0) takes the PF_PACK fields the previous push measured
    const int64_t pk_k = uni64(__hip_atomic_load(slot == 0 ? &ctrl0->pk_next_k : &ctrl0->pk_cur_k, __ATOMIC_RELAXED, DEV_SCOPE));
    const int64_t pk_v = uni64(__hip_atomic_load(slot == 0 ? &ctrl0->pk_next_v : &ctrl0->pk_cur_v, __ATOMIC_RELAXED, DEV_SCOPE));
    const uint32_t pk_bits = uni32(__hip_atomic_load(slot == 0 ? &ctrl0->pk_next_bits : &ctrl0->pk_cur_bits, __ATOMIC_RELAXED, DEV_SCOPE));
    if (slot >= FW_MAX_PENDING) {  // (uniform) the partial buffer is full: the host sizes pushes so it never is
        if (tid == 0) __hip_atomic_fetch_or(&ctrl0->error, ERR_CHUNKS, __ATOMIC_RELAXED, DEV_SCOPE);
        return;
    }
    const uint32_t kb = pk_bits & 255u, rb = (pk_bits >> 8) & 255u, vb = (pk_bits >> 16) & 255u;
    // PF_PACK launch: the epoch's fields are valid and the watermark is one the 32-bit slice
    // arithmetic below can be measured against
    const bool pk = (pk_bits & PK_OK) && a.can_pack && cur_wm > -(1ll << 62) && cur_wm < (1ll << 62);
    if (tid == 0) {
        *s_min = INT64_MAX;
        *s_drop = 0;
        s_samp[0] = s_samp[1] = 0;
        s_pk[0] = s_pk[2] = INT64_MAX;
        s_pk[1] = s_pk[3] = INT64_MIN;
    }
    for (int s = tid; s < (n_sb0 + 1) >> 1; s += BLK) hist2[s] = 0;
    if (pk)
        for (int s = tid; s < IGP_TAGS; s += BLK) tags[s] = 0;

    const int64_t base = c * CH;
    const uint32_t last = (uint32_t)min((int64_t)CH - 1, a.n - 1 - base);  // last row of the chunk
    const int64_t* kp = a.key + base;
    const int64_t* tp = a.ts + base;
    const int64_t* vp = a.val + base;
    const uint32_t iv = (uint32_t)a.interval;
    // ranks count from the epoch's rank base (slot 0's: every later row's slice end is >= it)
    const int64_t nbase = uni64(!pk ? 0 : slot > 0 ? a.slot_base[0] : igp_slice_end(a, wadd(cur_wm, 1)));

    uint64_t rw[RPT];   // the row's run word
    uint32_t rsr[RPT];  // superbucket | rank within it (later: chunk position) << 16; IGP_NONE / IGP_LATE: not a partial
    int64_t lmin = INT64_MAX;
    uint32_t ldrop = 0, total = 0;
    bool bad = !pk;
    __syncthreads();  // the header, the histogram and the tags are initialised
    if (pk) {
        // ---- every column load of the chunk in flight at once (a partial last chunk clamps its row
        // index), consumed row by row: route, slice end on the 32-bit path, late test, pack
        int64_t rk[RPT], rs[RPT], rv[RPT];
        auto issue = [&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t o = min((uint32_t)(j * BLK + tid), last);
            // (non-temporal: the columns are read once and should not push the run lines other chunks
            // are still completing out of the L2; round 10: about -2 us per launch in the 512 x 8
            // geometry, up to -5.9 us in the 256 x 16 one)
            rk[j] = __builtin_nontemporal_load(kp + o);
            rs[j] = __builtin_nontemporal_load(tp + o);
            rv[j] = __builtin_nontemporal_load(vp + o);
        };
        const int64_t ts0v = a.ts[base];  // chunk base of the 32-bit slice arithmetic (loaded first: waited for alone)
        static_for<AHEAD>(issue);
        const int64_t ts0 = uni64(ts0v);
        // slice-aligned base 2^30 ms below the chunk's first row (as k_ingest): a row within 2^31 ms
        // of it has the slice end tbase + (q + 1) * interval, q = (ts - tbase) / interval in 32 bits
        const bool fast = ts0 > -(1ll << 61) && ts0 < (1ll << 61);
        const int64_t tbase = uni64(fast ? window_start(ts0, a.offset, a.slice_div) - a.back : 0);
        // watermark and rank base against tbase; both lie on tbase's slice grid, so a row's rank is
        // q + 1 - nbq.  (fast: |tbase| < 2^62, so neither difference overflows)
        const int64_t wm1 = cur_wm - tbase + 1;  // the row is late when its slice end - tbase <= wm1
        const int64_t nbd = wsub(nbase, tbase);
        const uint64_t nbu = udiv((uint64_t)(nbd < 0 ? -nbd : nbd), a.slice_div);
        const int64_t nbq = uni64(nbd < 0 ? -(int64_t)nbu : (int64_t)nbu);  // exact (checked below)
        const uint32_t nbq1 = 1u - (uint32_t)nbq;
        const uint32_t rlimq = min(a.rank_q, 1u << rb);
        const uint64_t kmax = (1ull << kb) - 1ull, vmax = (1ull << vb) - 1ull;
        // a row the word cannot hold sends the chunk the slow way; so does a rank base off the grid or
        // too far from tbase for 32-bit ranks (q + 1 - nbq then cannot wrap into the rank field)
        bad = !fast || nbq * a.interval != nbd || nbq < -(1ll << 30) || nbq > (1ll << 30);
        bool foreign = false, samp = false, dup = false;
        uint32_t lminr = 0xFFFFFFFFu;
        auto eat = [&](auto J) {
            constexpr int j = decltype(J)::value;
            const bool live = (uint32_t)(j * BLK + tid) <= last;
            uint32_t m;
            const int32_t sb = igp_route<HK>(a, rk[j], &m);
            const uint64_t d = (uint64_t)rs[j] - (uint64_t)tbase;
            const uint32_t q = udiv32((uint32_t)d, a.slice_div32);
            const uint32_t ser = q * iv + iv;  // slice end - tbase (< 2^31 + 2^30)
            const bool near = d < (1ull << 31);
            const bool own = (uint32_t)sb < (uint32_t)n_sb0;
            // (plain & and |: straight-line code, every lane mask is consumed where it is made)
            foreign |= live & !own;
            const bool late = (int64_t)ser <= wm1;  // the slice's only window has fired: dropped
            const bool mine = live & own & near;
            const bool ok = mine & !late;
            lminr = min(lminr, ok ? ser : 0xFFFFFFFFu);
            const uint32_t rank = q + nbq1;
            const uint64_t ko = (uint64_t)rk[j] - (uint64_t)pk_k, ao = (uint64_t)rv[j] - (uint64_t)pk_v;
            bad |= (live & !near) | (ok & ((rank >= rlimq) | (ko > kmax) | (ao > vmax)));
            rw[j] = (ko << (64u - kb)) | ((uint64_t)rank << vb) | ao;
            rsr[j] = ok ? (uint32_t)sb : (mine & late) ? IGP_LATE : IGP_NONE;
            if constexpr (j == 0) {  // the sampled row: did the tag table last see this (key, slice)?
                // (a row that is no partial leaves tag 0, which no partial carries)
                const uint32_t tag = ok ? (m ^ (rank * 0x9E3779B9u)) | 1u : 0u;
                samp = ok;
                dup = ok & (atomicExch(&tags[(m >> 8) & (uint32_t)(IGP_TAGS - 1)], tag) == tag);
            }
        };
        // (rows AHEAD.. are loaded two at a time as two earlier rows have shrunk to their words: the
        // registers hold AHEAD loaded rows at most, the CU's workgroups keep HBM busy)
        static_for<(RPT - AHEAD) / 2>([&](auto S) {
            constexpr int s2 = 2 * decltype(S)::value;
            eat(std::integral_constant<int, s2>{});
            eat(std::integral_constant<int, s2 + 1>{});
            issue(std::integral_constant<int, AHEAD + s2>{});
            issue(std::integral_constant<int, AHEAD + s2 + 1>{});
        });
        static_for<AHEAD>([&](auto J) { eat(std::integral_constant<int, RPT - AHEAD + decltype(J)::value>{}); });
        if (foreign)  // key group not owned by this subtask
            __hip_atomic_fetch_or(&la->ctrl->error, ERR_KEYGROUP, __ATOMIC_RELAXED, DEV_SCOPE);
        // rank the partials per superbucket (16-bit counters, 32-bit LDS adds on the counter's half)
        static_for<RPT>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (igp_void(rsr[j])) return;
            const uint32_t sh = (rsr[j] & 1u) << 4;
            rsr[j] |= ((atomicAdd(&hist2[rsr[j] >> 1], 1u << sh) >> sh) & 0xFFFFu) << 16;
        });
        {
            const uint64_t bs = __ballot(samp), bd = __ballot(dup);
            if ((tid & 63) == 0) {
                atomicAdd(&s_samp[0], (uint32_t)__popcll(bs));
                if (bd) atomicAdd(&s_samp[1], (uint32_t)__popcll(bd));
            }
        }
        if (lminr != 0xFFFFFFFFu) lmin = tbase + (int64_t)lminr;
    }
    // (also: the histogram is complete.  Voted on outside the branch, so that the fast path is not the
    // routing code's own successor: the compiler then forms the packed words where the rows are routed
    // and not behind the vote, where every row would hold five registers instead of two until then)
    const bool slowc = !__syncthreads_and(!bad);

    // ---- from here on the arguments and the LDS layout come from the argument segment (see `la`)
    Ctrl* ctrl = la->ctrl;
    const int n_sb = la->n_sb;
    const IgpLds L = igp_lds(lds, n_sb);
    uint16_t* rbound = L.rbound;
    uint32_t* roff = L.roff;
    uint64_t* stage = L.stage;
    uint32_t* sdst = L.sdst;
    const uint32_t wrows = L.wrows;
    uint32_t* cells = la->cells + (size_t)slot * la->cell_stride;
    uint64_t* out = la->parts + (size_t)slot * la->part_stride + (size_t)base * PW;
    const int per = (n_sb + BLK - 1) / BLK;
    const int sb0 = min(tid * per, n_sb), sb1 = min(sb0 + per, n_sb);
    if (!slowc) {
        static_for<RPT>([&](auto J) { ldrop += rsr[decltype(J)::value] == IGP_LATE ? 1u : 0u; });
        // ---- the chunk's key and accumulator ranges, from the words' fields (every partial fits them).
        // A field of at most 32 bits (uniform over the launch; the key's usually is, the accumulator's
        // takes the word's spare bits) is reduced with 32-bit min / max and widened at the wave
        // reduction; a wave whose rows are all partials needs no selects.
        {
            uint32_t inv = 0, none = 0xFFFFFFFFu;
            static_for<RPT>([&](auto J) {
                inv |= rsr[decltype(J)::value];
                none &= rsr[decltype(J)::value];
            });
            const bool allv = __ballot(igp_void(inv)) == 0;    // every row of the wave is a partial
            const bool wany = __ballot(!igp_void(none)) != 0;  // the wave has a partial
            auto range32 = [&](auto field, uint64_t* lo, uint64_t* hi) {
                uint32_t mn = 0xFFFFFFFFu, mx = 0;
                if (allv) {
                    static_for<RPT>([&](auto J) {
                        const uint32_t f = field(rw[decltype(J)::value]);
                        mn = min(mn, f);
                        mx = max(mx, f);
                    });
                } else {
                    static_for<RPT>([&](auto J) {
                        constexpr int j = decltype(J)::value;
                        const uint32_t f = field(rw[j]);
                        mn = min(mn, igp_void(rsr[j]) ? 0xFFFFFFFFu : f);
                        mx = max(mx, igp_void(rsr[j]) ? 0u : f);
                    });
                }
                *lo = wred_min_u32(mn);
                *hi = wred_max_u32(mx);
            };
            auto range64 = [&](auto field, uint64_t* lo, uint64_t* hi) {  // (the fields are < 2^62: signed reductions order them)
                int64_t mn = INT64_MAX, mx = INT64_MIN;
                static_for<RPT>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const int64_t f = (int64_t)field(rw[j]);
                    const bool v = allv | !igp_void(rsr[j]);
                    mn = v ? min(mn, f) : mn;
                    mx = v ? max(mx, f) : mx;
                });
                *lo = (uint64_t)wred_min_i64(mn);
                *hi = (uint64_t)wred_max_i64(mx);
            };
            uint64_t kmn, kmx, vmn, vmx;
            if (kb <= 32u) {
                const uint32_t ksh = 32u - kb;
                range32([&](uint64_t w) { return (uint32_t)(w >> 32) >> ksh; }, &kmn, &kmx);
            } else {
                const uint32_t ksh = 64u - kb;
                range64([&](uint64_t w) { return w >> ksh; }, &kmn, &kmx);
            }
            if (vb <= 32u) {
                const uint32_t vmask = 0xFFFFFFFFu >> (32u - vb);
                range32([&](uint64_t w) { return (uint32_t)w & vmask; }, &vmn, &vmx);
            } else {
                const uint64_t vmask = (1ull << vb) - 1ull;
                range64([&](uint64_t w) { return w & vmask; }, &vmn, &vmx);
            }
            if ((tid & 63) == 0 && wany) {
                __hip_atomic_fetch_min(&s_pk[0], (int64_t)((uint64_t)pk_k + kmn), __ATOMIC_RELAXED, LDS_SCOPE);
                __hip_atomic_fetch_max(&s_pk[1], (int64_t)((uint64_t)pk_k + kmx), __ATOMIC_RELAXED, LDS_SCOPE);
                __hip_atomic_fetch_min(&s_pk[2], (int64_t)((uint64_t)pk_v + vmn), __ATOMIC_RELAXED, LDS_SCOPE);
                __hip_atomic_fetch_max(&s_pk[3], (int64_t)((uint64_t)pk_v + vmx), __ATOMIC_RELAXED, LDS_SCOPE);
            }
        }
        // ---- claim this chunk's stretch of every superbucket's sub-run (the counts are final), so
        // the claims' round trip overlaps the scan; superbuckets strided over the threads
        const uint32_t xr = (uint32_t)c & (RUN_X - 1);
        uint32_t* fill = la->run_fill + ((size_t)slot * RUN_X + xr) * n_sb;
        uint32_t pos[KMAX], cnt[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            const int i = tid + k * BLK;
            cnt[k] = i < n_sb ? hist[i] : 0u;
            pos[k] = cnt[k] ? atomicAdd(fill + i, cnt[k]) : 0u;
        }
        uint32_t seg = 0;
        for (int i = sb0; i < sb1; i++) seg += hist[i];
        const uint32_t incl = block_incl_scan<BLK>(seg, wsum, &total);
        uint32_t run = incl - seg;
        for (int i = sb0; i < sb1; i++) {
            const uint32_t v = hist[i];
            hist[i] = (uint16_t)run;
            run += v;
        }
        __syncthreads();
        // per superbucket: chunk positions below rbound go to the run at position + roff, the rest
        // stay in the chunk's region (overflow flag)
        const uint32_t scap = la->sub_cap;
        uint32_t* ovf = la->run_ovf + (size_t)slot * n_sb;
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            const int i = tid + k * BLK;
            if (i >= n_sb) break;
            const uint32_t st0 = hist[i], v = cnt[k];
            const uint32_t n_in = pos[k] >= scap ? 0u : min(v, scap - pos[k]);
            rbound[i] = (uint16_t)(st0 + n_in);
            roff[i] = (uint32_t)(((size_t)i * RUN_X + xr) * scap + pos[k]) - st0;
            cells[cell_index(c, n_sb, i)] = (st0 + n_in) | ((v - n_in) << 16) | (PF_PACK << 30);
            if (n_in < v) ovf[i] = 1u;
        }
        static_for<RPT>([&](auto J) {  // rank within the superbucket -> position in the chunk
            constexpr int j = decltype(J)::value;
            if (igp_void(rsr[j])) return;
            rsr[j] += (uint32_t)hist[rsr[j] & 0xFFFFu] << 16;
        });
        // ---- store the words through an LDS stage of wrows (word, destination) rows, so neighbouring
        // lanes store neighbouring words of a superbucket's stretch
        uint64_t* rslot = la->runs + (size_t)slot * la->run_stride;  // (a slot is sized for PF_WIDE rows)
        for (uint32_t w0 = 0; w0 < total; w0 += wrows) {
            __syncthreads();  // rbound / roff are written; the previous window is stored
            static_for<RPT>([&](auto J) {
                constexpr int j = decltype(J)::value;
                const uint32_t p = rsr[j] >> 16, d = p - w0, i = rsr[j] & 0xFFFFu;
                if (igp_void(rsr[j]) || d >= wrows) return;
                stage[d] = rw[j];
                sdst[d] = p < rbound[i] ? p + roff[i] : (RUN_LOCAL | p);
            });
            __syncthreads();
            const uint32_t nr = min(wrows, total - w0);
            for (uint32_t r = tid; r < nr; r += BLK) {
                const uint32_t dd = sdst[r];
                st8((dd & RUN_LOCAL) ? out + (dd & ~RUN_LOCAL) : rslot + dd, stage[r]);
            }
        }
    } else {
        // ---- slow chunk: one row per thread per iteration, the general slice assignment, PF_WIDE rows
        // sorted by superbucket into the chunk's region.  Starts over: the fast path's counts are void.
        __syncthreads();  // every thread is done with the fast path's histogram
        if (tid == 0) {
            s_samp[0] = s_samp[1] = 0;
            s_pk[0] = s_pk[2] = INT64_MAX;
            s_pk[1] = s_pk[3] = INT64_MIN;
        }
        for (int s = tid; s < (n_sb + 1) >> 1; s += BLK) hist2[s] = 0;
        lmin = INT64_MAX;
        ldrop = 0;
        uint16_t* rrank = (uint16_t*)stage;  // [CH] rank within the superbucket; 0xFFFF: not a partial
        const IgpSlice sl = igp_slice_late(la);
        const int64_t wm_now = uni64(__hip_atomic_load(&ctrl->cur, __ATOMIC_RELAXED, DEV_SCOPE));  // (= cur_wm: no merge runs beside a push)
        const int64_t* skp = la->key + base;
        const int64_t* stp = la->ts + base;
        const int64_t* svp = la->val + base;
        uint32_t* ovf = la->run_ovf + (size_t)slot * n_sb;
        int64_t kmn = INT64_MAX, kmx = INT64_MIN, vmn = INT64_MAX, vmx = INT64_MIN;
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < RPT; it++) {
            const uint32_t o = (uint32_t)(it * BLK + tid);
            uint32_t r = 0xFFFFu;
            if (o <= last) {
                const int64_t key = skp[o], ts = stp[o], acc = svp[o];
                uint32_t m;
                const int32_t sb = igp_route<HK>(a, key, &m);
                if ((uint32_t)sb >= (uint32_t)n_sb) {
                    __hip_atomic_fetch_or(&ctrl->error, ERR_KEYGROUP, __ATOMIC_RELAXED, DEV_SCOPE);
                } else {
                    const int64_t se = igp_slice_end(sl, ts);
                    if (is_fired(se, wm_now)) {  // TUMBLE, UTC: late for its only window
                        ldrop++;
                    } else {
                        lmin = min(lmin, se);
                        kmn = min(kmn, key);
                        kmx = max(kmx, key);
                        vmn = min(vmn, acc);
                        vmx = max(vmx, acc);
                        const uint32_t sh = ((uint32_t)sb & 1u) << 4;
                        r = (atomicAdd(&hist2[(uint32_t)sb >> 1], 1u << sh) >> sh) & 0xFFFFu;
                    }
                }
            }
            rrank[o] = (uint16_t)r;
        }
        kmn = wred_min_i64(kmn);
        kmx = wred_max_i64(kmx);
        vmn = wred_min_i64(vmn);
        vmx = wred_max_i64(vmx);
        if ((tid & 63) == 0 && kmn <= kmx) {
            __hip_atomic_fetch_min(&s_pk[0], kmn, __ATOMIC_RELAXED, LDS_SCOPE);
            __hip_atomic_fetch_max(&s_pk[1], kmx, __ATOMIC_RELAXED, LDS_SCOPE);
            __hip_atomic_fetch_min(&s_pk[2], vmn, __ATOMIC_RELAXED, LDS_SCOPE);
            __hip_atomic_fetch_max(&s_pk[3], vmx, __ATOMIC_RELAXED, LDS_SCOPE);
        }
        __syncthreads();
        uint32_t seg = 0;
        for (int i = sb0; i < sb1; i++) seg += hist[i];
        const uint32_t incl = block_incl_scan<BLK>(seg, wsum, &total);
        uint32_t run = incl - seg;
        for (int i = sb0; i < sb1; i++) {  // every row stays in the chunk's region
            const uint32_t v = hist[i];
            hist[i] = (uint16_t)run;
            cells[cell_index(c, n_sb, i)] = run | (v << 16) | (PF_WIDE << 30);
            if (v) ovf[i] = 1u;
            run += v;
        }
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < RPT; it++) {
            const uint32_t o = (uint32_t)(it * BLK + tid);
            const uint32_t r = rrank[o];
            if (r == 0xFFFFu) continue;
            const int64_t key = skp[o], ts = stp[o], acc = svp[o];
            uint32_t m;
            const int32_t sb = igp_route<HK>(a, key, &m);
            uint64_t* p = out + (size_t)(r + hist[sb]) * PW;
            p[0] = (uint64_t)key;
            p[1] = (uint64_t)igp_slice_end(sl, ts);
            p[2] = (uint64_t)acc;
        }
    }
    const uint32_t fmt = slowc ? PF_WIDE : PF_PACK;
    const uint32_t push_fmt = pk ? PF_PACK : PF_WIDE;  // (uniform over the launch)

    // ---- control counters, as k_ingest: each chunk publishes its stats with agent-scope stores, then
    // takes a ticket; the last workgroup of the launch reduces them into the control block and
    // commits the push's slot.  (The chunk's accepted rows are its partials: nothing folds.)
    {
        const int64_t wm = wred_min_i64(lmin);
        const uint32_t wd = wred_sum_u32(ldrop);
        if ((tid & 63) == 0) {
            if (wm != INT64_MAX) __hip_atomic_fetch_min(s_min, wm, __ATOMIC_RELAXED, LDS_SCOPE);
            if (wd) atomicAdd(s_drop, (unsigned long long)wd);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int64_t* cs = la->chunk_stats + CS_WORDS * c;
        __hip_atomic_store(&cs[0], *s_min, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&cs[1], (int64_t)*s_drop, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&cs[2], (int64_t)total, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&cs[3], (int64_t)total, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&cs[4],
                           (int64_t)total * 8 * pf_stride(fmt, 1) | ((int64_t)(fmt != PF_WIDE) << 40), __ATOMIC_RELAXED,
                           DEV_SCOPE);
        __hip_atomic_store(&cs[5], (int64_t)s_samp[0], __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&cs[6], (int64_t)s_samp[1], __ATOMIC_RELAXED, DEV_SCOPE);
#pragma unroll
        for (int q = 0; q < 4; q++) __hip_atomic_store(&cs[8 + q], s_pk[q], __ATOMIC_RELAXED, DEV_SCOPE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *s_last = grid_last_wg(la->tickets->c[0]);
    }
    __syncthreads();
    if (!*s_last) return;
    int64_t m = INT64_MAX, d = 0, q = 0, y = 0, sm = 0, dp = 0;
    int64_t kmn = INT64_MAX, kmx = INT64_MIN, vmn = INT64_MAX, vmx = INT64_MIN;
    for (int64_t i = tid; i < (int64_t)gridDim.x; i += BLK) {
        const int64_t* cs = la->chunk_stats + CS_WORDS * i;
        m = min(m, __hip_atomic_load(&cs[0], __ATOMIC_RELAXED, DEV_SCOPE));
        d += __hip_atomic_load(&cs[1], __ATOMIC_RELAXED, DEV_SCOPE);
        q += __hip_atomic_load(&cs[3], __ATOMIC_RELAXED, DEV_SCOPE);
        y += __hip_atomic_load(&cs[4], __ATOMIC_RELAXED, DEV_SCOPE);  // no carry: < 2^40 per chunk
        sm += __hip_atomic_load(&cs[5], __ATOMIC_RELAXED, DEV_SCOPE);
        dp += __hip_atomic_load(&cs[6], __ATOMIC_RELAXED, DEV_SCOPE);
        kmn = min(kmn, __hip_atomic_load(&cs[8], __ATOMIC_RELAXED, DEV_SCOPE));
        kmx = max(kmx, __hip_atomic_load(&cs[9], __ATOMIC_RELAXED, DEV_SCOPE));
        vmn = min(vmn, __hip_atomic_load(&cs[10], __ATOMIC_RELAXED, DEV_SCOPE));
        vmx = max(vmx, __hip_atomic_load(&cs[11], __ATOMIC_RELAXED, DEV_SCOPE));
    }
    m = wred_min_i64(m);
    d = wred_sum_i64(d);
    q = wred_sum_i64(q);
    y = wred_sum_i64(y);
    sm = wred_sum_i64(sm);
    dp = wred_sum_i64(dp);
    kmn = wred_min_i64(kmn);
    kmx = wred_max_i64(kmx);
    vmn = wred_min_i64(vmn);
    vmx = wred_max_i64(vmx);
    int64_t* red = (int64_t*)stage;  // [10][NWV]
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[w] = m;
        red[NWV + w] = d;
        red[2 * NWV + w] = sm;
        red[3 * NWV + w] = q;
        red[4 * NWV + w] = y;
        red[5 * NWV + w] = kmn;
        red[6 * NWV + w] = kmx;
        red[7 * NWV + w] = vmn;
        red[8 * NWV + w] = vmx;
        red[9 * NWV + w] = dp;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll 1
    for (int v = 1; v < NWV; v++) {
        m = min(m, red[v]);
        d += red[NWV + v];
        sm += red[2 * NWV + v];
        q += red[3 * NWV + v];
        y += red[4 * NWV + v];
        kmn = min(kmn, red[5 * NWV + v]);
        kmx = max(kmx, red[6 * NWV + v]);
        vmn = min(vmn, red[7 * NWV + v]);
        vmx = max(vmx, red[8 * NWV + v]);
        dp += red[9 * NWV + v];
    }
    la->slot_nch[slot] = (int32_t)gridDim.x;
    la->slot_base[slot] = igp_slice_end(igp_slice_late(la), wadd(ctrl->cur, 1));
    la->slot_fmt[slot] = (int32_t)push_fmt;
    ctrl->pending_pushes = slot + 1;
    ctrl->min_pending = min(ctrl->min_pending, m);
    ctrl->pending_rows += (uint64_t)q;
    ctrl->partials += (uint64_t)q;
    ctrl->part_bytes += (uint64_t)(y & ((1ll << 40) - 1));
    ctrl->compact_chunks += (uint64_t)(y >> 40);
    ctrl->push_count += 1;  // (fold_skip stands: this kernel measures no fold)
    ctrl->late_dropped += (uint64_t)d;
    // the sampled fold estimate: a push without samples (no packed chunk) clears the hint
    ctrl->ig_skew = sm > 0 && dp * IGP_SKEW_DEN >= sm;
    if (slot == 0) {  // this push opened the flush epoch with the parameters it read
        ctrl->pk_cur_k = pk_k;
        ctrl->pk_cur_v = pk_v;
        ctrl->pk_cur_bits = pk_bits;
    }
    ctrl->pk_next_bits = pack_fields(kmn, kmx, vmn, vmx, &ctrl->pk_next_k, &ctrl->pk_next_v, ctrl->pk_next_bits);
    ig_mirror_store(la->tickets, ctrl);
    kt_end(la->kt);
}

// the handle's plan and this push are ones k_ingest_pack serves (fw_api.hip checks the same before it
// chooses the kernel; a mismatch is a planning error, not a fallback)
inline bool igp_serves(const IngestArgs& a) {
    bool plain = a.khash == nullptr && a.seg_counts == nullptr && a.stride == 1 && !a.no_fold;
    for (int q = 0; q < MAX_KCOLS; q++) plain = plain && a.nulls[q] == nullptr;
    return plain && a.pack && a.runs && !a.narrow && a.nv == 1 && a.wd.nw == 1 && a.wd.op[0] != W_CNT && !a.wd.has_ord && !a.wd.has_q &&
           a.win.kind == FW_WIN_TUMBLE && !a.win.ds && !a.global && !a.local && a.win.tz.n == 0 && a.win.fast32 &&
           a.ks.pass_log2 == 0 && a.ks.n_sb <= IGP_MAX_SB && a.ks.hash_kind != KH_PRE;
}

// the kernel's arguments of a push igp_serves accepted
inline IngestPackArgs igp_args(const IngestArgs& a) {
    IngestPackArgs p{};
    p.key = a.key;
    p.ts = a.ts;
    p.val = (const int64_t*)a.vals[0];
    p.n = a.n;
    p.ctrl = a.ctrl;
    p.tickets = a.tickets;
    p.chunk_stats = a.chunk_stats;
    p.kt = a.kt;
    p.parts = a.parts;
    p.runs = a.runs;
    p.cells = a.cells;
    p.run_fill = a.run_fill;
    p.run_ovf = a.run_ovf;
    p.slot_base = a.slot_base;
    p.slot_nch = a.slot_nch;
    p.slot_fmt = a.slot_fmt;
    p.part_stride = a.cap_rows * 3;
    p.run_stride = a.run_rows * 3;
    p.cell_stride = (int64_t)a.ks.n_sb * a.max_nch;
    p.interval = a.win.interval;
    p.offset = a.win.offset;
    p.back = (int64_t)((1u << 30) / (uint32_t)a.win.interval) * a.win.interval;  // (fast32: interval < 2^30)
    p.slice_div = a.win.slice_div;
    p.slice_div32 = a.win.slice_div32;
    p.maxp_div = a.ks.maxp_div;
    p.max_p = a.ks.max_p;
    p.kg_start = a.ks.kg_start;
    p.sb_log2 = a.ks.sb_per_kg_log2;
    p.n_sb = a.ks.n_sb;
    p.rank_q = (uint32_t)(a.rank_lim / a.win.interval);
    p.sub_cap = (uint32_t)a.sub_cap;
    p.can_pack = a.pack && a.runs && !a.local;
    return p;
}

template <int HK, int BLK, int RPT, int WAVES>
static hipError_t ingest_pack_hk(const IngestArgs& a, hipStream_t s, KTimer* t) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_ingest_pack<HK, BLK, RPT, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, IGP_LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    kt_mark(t, FW_KT_REDUCE, false, s);
    hipLaunchKernelGGL((k_ingest_pack<HK, BLK, RPT, WAVES>), dim3((unsigned)a.n_chunks), dim3(BLK), IGP_LDS, s, igp_args(a));
    kt_mark(t, FW_KT_REDUCE, true, s);
    return hipGetLastError();
}
// one geometry's launcher: the instantiations of the four key-hash kinds
template <int BLK, int RPT, int WAVES>
static hipError_t ingest_pack_geom(const IngestArgs& a, hipStream_t s, KTimer* t) {
    if (a.n_chunks == 0) return hipSuccess;
    if (!igp_serves(a)) return hipErrorInvalidValue;
    switch (a.ks.hash_kind) {
        case KH_LONG: return ingest_pack_hk<KH_LONG, BLK, RPT, WAVES>(a, s, t);
        case KH_INT: return ingest_pack_hk<KH_INT, BLK, RPT, WAVES>(a, s, t);
        case KH_BINROW_BIGINT: return ingest_pack_hk<KH_BINROW_BIGINT, BLK, RPT, WAVES>(a, s, t);
        default: return ingest_pack_hk<KH_BINROW_INT, BLK, RPT, WAVES>(a, s, t);
    }
}
// workgroups of the CFG2 instance (KH_BINROW_BIGINT) a CU holds; < 0: the runtime's error, negated
template <int BLK, int RPT, int WAVES>
static int ingest_pack_wg_per_cu() {
    int n = 0;
    hipError_t e = hipFuncSetAttribute((const void*)k_ingest_pack<KH_BINROW_BIGINT, BLK, RPT, WAVES>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, IGP_LDS);
    if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)k_ingest_pack<KH_BINROW_BIGINT, BLK, RPT, WAVES>, BLK, IGP_LDS);
    return e == hipSuccess ? n : -(int)e;
}

}  // namespace fw
