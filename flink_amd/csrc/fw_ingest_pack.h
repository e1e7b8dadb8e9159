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
// the histogram, the run bookkeeping and a store stage of (word, destination) rows: 64 VGPRs and
// 39 KiB, four workgroups per CU, so one workgroup's column loads overlap the others' sorting and
// stores.
//
// Same chunks (512 threads x 8 rows), same slot, cells, run claims, overflow flags, chunk statistics
// and last-workgroup commit as k_ingest, which the merge kernel and the next push read; it never folds
// and leaves Ctrl::fold_skip alone.  Whatever the packed word cannot hold makes the *chunk* slow: a
// rolled, one-row-per-thread loop that reloads the columns and writes PF_WIDE rows, sorted by
// superbucket, into the chunk's own region with their cell words and overflow flags -- what k_ingest
// writes for such a chunk of a PF_PACK push.  A launch that cannot pack at all (no valid PF_PACK
// fields yet, no watermark yet) sends every chunk that way.  The host's choice between the two
// kernels (fw_api.hip) therefore only costs time when it is wrong.
// ======================================================================================

// HK: the key-hash kind (KH_*, not KH_PRE), resolved per launch
template <int HK>
__global__ __launch_bounds__(IGP_BLOCK, IGP_WAVES) void k_ingest_pack(IngestArgs a) {
    constexpr int BLK = IGP_BLOCK, RPT = IGP_RPT, CH = BLK * RPT, NWV = BLK / 64;
    constexpr int PW = 3;  // words of a PF_WIDE row: key, slice end, one accumulator word
    static_assert(CH <= 4096, "a chunk position and a superbucket share a 32-bit word");
    // dynamic LDS: [header 16 words][hist: n_sb u16][rbound: n_sb u16][roff: n_sb u32][stage words][stage destinations]
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    int64_t* s_min = (int64_t*)&lds[0];
    unsigned long long* s_drop = (unsigned long long*)&lds[1];
    unsigned long long* s_rows = (unsigned long long*)&lds[2];
    int32_t* s_last = (int32_t*)&lds[3];
    uint32_t* wsum = (uint32_t*)&lds[4];  // NWV words
    int64_t* s_pk = (int64_t*)&lds[12];   // key min / max, accumulator min / max of the chunk's partials
    const int n_sb = a.ks.n_sb;           // (pass_log2 == 0: ingest superbuckets are the state's)
    const int n_pad = (n_sb + 7) & ~7;
    uint16_t* hist = (uint16_t*)(lds + IG_HDR_WORDS);
    uint32_t* hist2 = (uint32_t*)hist;
    uint16_t* rbound = (uint16_t*)(lds + IG_HDR_WORDS + ig_hist_words(n_sb));
    uint32_t* roff = (uint32_t*)(rbound + n_pad);
    uint64_t* stage = (uint64_t*)(roff + n_pad);  // 16-B aligned (igp_fixed_bytes)
    const uint32_t wrows = (uint32_t)igp_stage_rows(n_sb);
    uint32_t* sdst = (uint32_t*)(stage + wrows);

    const int tid = threadIdx.x;
    Ctrl* ctrl = a.ctrl;
    const int64_t c = blockIdx.x;
    kt_start(a.kt);
    const int64_t slot = uni64(__hip_atomic_load(&ctrl->pending_pushes, __ATOMIC_RELAXED, DEV_SCOPE));
    const int64_t cur_wm = uni64(__hip_atomic_load(&ctrl->cur, __ATOMIC_RELAXED, DEV_SCOPE));
    // the epoch's first push (slot 0) takes the PF_PACK fields the previous push measured
    const int64_t pk_k = uni64(__hip_atomic_load(slot == 0 ? &ctrl->pk_next_k : &ctrl->pk_cur_k, __ATOMIC_RELAXED, DEV_SCOPE));
    const int64_t pk_v = uni64(__hip_atomic_load(slot == 0 ? &ctrl->pk_next_v : &ctrl->pk_cur_v, __ATOMIC_RELAXED, DEV_SCOPE));
    const uint32_t pk_bits = uni32(__hip_atomic_load(slot == 0 ? &ctrl->pk_next_bits : &ctrl->pk_cur_bits, __ATOMIC_RELAXED, DEV_SCOPE));
    if (slot >= FW_MAX_PENDING) {  // (uniform) the partial buffer is full: the host sizes pushes so it never is
        if (tid == 0) __hip_atomic_fetch_or(&ctrl->error, ERR_CHUNKS, __ATOMIC_RELAXED, DEV_SCOPE);
        return;
    }
    if (tid == 0) {
        *s_min = INT64_MAX;
        *s_drop = 0;
        *s_rows = 0;
        s_pk[0] = s_pk[2] = INT64_MAX;
        s_pk[1] = s_pk[3] = INT64_MIN;
    }
    for (int s = tid; s < (n_sb + 1) >> 1; s += BLK) hist2[s] = 0;

    const int64_t base = c * CH;
    const uint32_t last = (uint32_t)min((int64_t)CH - 1, a.n - 1 - base);  // last row of the chunk
    const int64_t* kp = a.key + base;
    const int64_t* tp = a.ts + base;
    const int64_t* vp = (const int64_t*)a.vals[0] + base;
    const uint32_t iv = (uint32_t)a.win.interval;
    const uint32_t kb = pk_bits & 255u, rb = (pk_bits >> 8) & 255u, vb = (pk_bits >> 16) & 255u;
    // PF_PACK launch: the epoch's fields are valid and the watermark is one the 32-bit slice
    // arithmetic below can be measured against
    const bool pk = (pk_bits & PK_OK) && a.pack && a.runs && !a.local && cur_wm > -(1ll << 62) && cur_wm < (1ll << 62);
    // ranks count from the epoch's rank base (slot 0's: every later row's slice end is >= it)
    const int64_t nbase = uni64(!pk ? 0 : slot > 0 ? a.slot_base[0] : slice_end_of(a.win, wadd(cur_wm, 1)));

    uint64_t rw[RPT];   // the row's run word
    uint32_t rsr[RPT];  // superbucket | rank within it (later: chunk position) << 16; ~0: not a partial
    int64_t lmin = INT64_MAX;
    uint32_t ldrop = 0, lrows = 0, total = 0;
    bool slowc = true;
    __syncthreads();  // the header and the histogram are initialised
    if (pk) {
        // ---- every column load of the chunk in flight at once (a partial last chunk clamps its row
        // index), consumed row by row: route, slice end on the 32-bit path, late test, pack
        int64_t rk[RPT], rs[RPT], rv[RPT];
        auto issue = [&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t o = min((uint32_t)(j * BLK + tid), last);
            rk[j] = kp[o];
            rs[j] = tp[o];
            rv[j] = vp[o];
        };
        const int64_t ts0v = a.ts[base];  // chunk base of the 32-bit slice arithmetic (loaded first: waited for alone)
        static_for<IGP_AHEAD>(issue);
        const int64_t ts0 = uni64(ts0v);
        // slice-aligned base 2^30 ms below the chunk's first row (as k_ingest): a row within 2^31 ms
        // of it has the slice end tbase + (q + 1) * interval, q = (ts - tbase) / interval in 32 bits
        const bool fast = ts0 > -(1ll << 61) && ts0 < (1ll << 61);
        const int64_t tbase =
            uni64(fast ? window_start(ts0, a.win.offset, a.win.slice_div) - (int64_t)((1u << 30) / iv) * a.win.interval : 0);
        // watermark and rank base against tbase; both lie on tbase's slice grid, so a row's rank is
        // q + 1 - nbq.  (fast: |tbase| < 2^62, so neither difference overflows)
        const int64_t wm1 = cur_wm - tbase + 1;                   // the row is late when its slice end - tbase <= wm1
        const int64_t nbq = uni64(wsub(nbase, tbase) / a.win.interval);  // exact (checked below)
        const uint32_t nbq1 = 1u - (uint32_t)nbq;
        const uint32_t rlimq = uni32((uint32_t)(min((uint64_t)a.rank_lim, (uint64_t)a.win.interval << rb) / (uint64_t)a.win.interval));
        const uint64_t kmax = (1ull << kb) - 1ull, vmax = (1ull << vb) - 1ull;
        // a row the word cannot hold sends the chunk the slow way; so does a rank base off the grid or
        // too far from tbase for 32-bit ranks (q + 1 - nbq then cannot wrap into the rank field)
        bool bad = !fast || nbq * a.win.interval != wsub(nbase, tbase) || nbq < -(1ll << 30) || nbq > (1ll << 30);
        bool foreign = false;
        uint32_t lminr = 0xFFFFFFFFu;
        auto eat = [&](auto J) {
            constexpr int j = decltype(J)::value;
            const bool live = (uint32_t)(j * BLK + tid) <= last;
            uint32_t m;
            const int32_t sb = route_key(a.ks, rk[j], 0, &m, HK);
            const uint64_t d = (uint64_t)rs[j] - (uint64_t)tbase;
            const uint32_t q = udiv32((uint32_t)d, a.win.slice_div32);
            const uint32_t ser = q * iv + iv;  // slice end - tbase (< 2^31 + 2^30)
            const bool near = d < (1ull << 31);
            const bool own = (uint32_t)sb < (uint32_t)n_sb;
            foreign |= live && !own;
            const bool late = (int64_t)ser <= wm1;  // the slice's only window has fired: dropped
            const bool ok = live && own && near && !late;
            ldrop += (live && own && near && late) ? 1u : 0u;
            lrows += ok ? 1u : 0u;
            lminr = ok ? min(lminr, ser) : lminr;
            const uint32_t rank = q + nbq1;
            const uint64_t ko = (uint64_t)rk[j] - (uint64_t)pk_k, ao = (uint64_t)rv[j] - (uint64_t)pk_v;
            bad |= (live && !near) || (ok && (rank >= rlimq || ko > kmax || ao > vmax));
            rw[j] = (ko << (64u - kb)) | ((uint64_t)rank << vb) | ao;
            rsr[j] = ok ? (uint32_t)sb : 0xFFFFFFFFu;
        };
        // (rows IGP_AHEAD.. are loaded two at a time as two earlier rows have shrunk to their words: the
        // registers hold IGP_AHEAD loaded rows at most, the CU's four workgroups keep HBM busy)
        static_for<(RPT - IGP_AHEAD) / 2>([&](auto S) {
            constexpr int s2 = 2 * decltype(S)::value;
            eat(std::integral_constant<int, s2>{});
            eat(std::integral_constant<int, s2 + 1>{});
            issue(std::integral_constant<int, IGP_AHEAD + s2>{});
            issue(std::integral_constant<int, IGP_AHEAD + s2 + 1>{});
        });
        static_for<IGP_AHEAD>([&](auto J) { eat(std::integral_constant<int, RPT - IGP_AHEAD + decltype(J)::value>{}); });
        if (foreign)  // key group not owned by this subtask
            __hip_atomic_fetch_or(&ctrl->error, ERR_KEYGROUP, __ATOMIC_RELAXED, DEV_SCOPE);
        // rank the partials per superbucket (16-bit counters, 32-bit LDS adds on the counter's half)
        static_for<RPT>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (rsr[j] == 0xFFFFFFFFu) return;
            const uint32_t sh = (rsr[j] & 1u) << 4;
            rsr[j] |= ((atomicAdd(&hist2[rsr[j] >> 1], 1u << sh) >> sh) & 0xFFFFu) << 16;
        });
        if (lminr != 0xFFFFFFFFu) lmin = tbase + (int64_t)lminr;
        slowc = !__syncthreads_and(!bad);  // (also: the histogram is complete)
    }

    uint32_t* cells = a.cells + (size_t)slot * n_sb * a.max_nch;
    uint64_t* out = a.parts + ((size_t)slot * a.cap_rows + (size_t)base) * PW;
    const int per = (n_sb + BLK - 1) / BLK;
    const int sb0 = min(tid * per, n_sb), sb1 = min(sb0 + per, n_sb);
    if (!slowc) {
        // ---- the chunk's key and accumulator ranges, from the words' fields (every partial fits them)
        {
            const uint64_t vmask = (1ull << vb) - 1ull;
            uint64_t kmn = ~0ull, kmx = 0, vmn = ~0ull, vmx = 0;
            bool any = false;
            static_for<RPT>([&](auto J) {
                constexpr int j = decltype(J)::value;
                const bool v = rsr[j] != 0xFFFFFFFFu;
                const uint64_t kf = rw[j] >> (64u - kb), vf = rw[j] & vmask;
                any |= v;
                kmn = v ? min(kmn, kf) : kmn;
                kmx = v ? max(kmx, kf) : kmx;
                vmn = v ? min(vmn, vf) : vmn;
                vmx = v ? max(vmx, vf) : vmx;
            });
            // (the fields are < 2^62: signed reductions order them)
            const bool wany = __ballot(any) != 0;
            kmn = (uint64_t)wred_min_i64(any ? (int64_t)kmn : INT64_MAX);
            kmx = (uint64_t)wred_max_i64(any ? (int64_t)kmx : INT64_MIN);
            vmn = (uint64_t)wred_min_i64(any ? (int64_t)vmn : INT64_MAX);
            vmx = (uint64_t)wred_max_i64(any ? (int64_t)vmx : INT64_MIN);
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
        uint32_t pos[IGP_KMAX], cnt[IGP_KMAX];
#pragma unroll
        for (int k = 0; k < IGP_KMAX; k++) {
            const int i = tid + k * BLK;
            cnt[k] = i < n_sb ? hist[i] : 0u;
            pos[k] = cnt[k] ? atomicAdd(a.run_fill + ((size_t)slot * RUN_X + xr) * n_sb + i, cnt[k]) : 0u;
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
        const uint32_t scap = (uint32_t)a.sub_cap;
#pragma unroll
        for (int k = 0; k < IGP_KMAX; k++) {
            const int i = tid + k * BLK;
            if (i >= n_sb) break;
            const uint32_t st0 = hist[i], v = cnt[k];
            const uint32_t n_in = pos[k] >= scap ? 0u : min(v, scap - pos[k]);
            rbound[i] = (uint16_t)(st0 + n_in);
            roff[i] = (uint32_t)(((size_t)i * RUN_X + xr) * scap + pos[k]) - st0;
            cells[cell_index(c, n_sb, i)] = (st0 + n_in) | ((v - n_in) << 16) | (PF_PACK << 30);
            if (n_in < v) a.run_ovf[(size_t)slot * n_sb + i] = 1u;
        }
        static_for<RPT>([&](auto J) {  // rank within the superbucket -> position in the chunk
            constexpr int j = decltype(J)::value;
            if (rsr[j] == 0xFFFFFFFFu) return;
            rsr[j] += (uint32_t)hist[rsr[j] & 0xFFFFu] << 16;
        });
        // ---- store the words through an LDS stage of wrows (word, destination) rows, so neighbouring
        // lanes store neighbouring words of a superbucket's stretch
        uint64_t* rslot = a.runs + (size_t)slot * a.run_rows * PW;  // (a slot is sized for PF_WIDE rows)
        for (uint32_t w0 = 0; w0 < total; w0 += wrows) {
            __syncthreads();  // rbound / roff are written; the previous window is stored
            static_for<RPT>([&](auto J) {
                constexpr int j = decltype(J)::value;
                const uint32_t p = rsr[j] >> 16, d = p - w0, i = rsr[j] & 0xFFFFu;
                if (rsr[j] == 0xFFFFFFFFu || d >= wrows) return;
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
            s_pk[0] = s_pk[2] = INT64_MAX;
            s_pk[1] = s_pk[3] = INT64_MIN;
        }
        for (int s = tid; s < (n_sb + 1) >> 1; s += BLK) hist2[s] = 0;
        lmin = INT64_MAX;
        ldrop = 0;
        lrows = 0;
        uint16_t* rrank = (uint16_t*)stage;  // [CH] rank within the superbucket; 0xFFFF: not a partial
        int64_t kmn = INT64_MAX, kmx = INT64_MIN, vmn = INT64_MAX, vmx = INT64_MIN;
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < RPT; it++) {
            const uint32_t o = (uint32_t)(it * BLK + tid);
            uint32_t r = 0xFFFFu;
            if (o <= last) {
                const int64_t key = kp[o], ts = tp[o], acc = vp[o];
                uint32_t m;
                const int32_t sb = route_key(a.ks, key, 0, &m, HK);
                if ((uint32_t)sb >= (uint32_t)n_sb) {
                    __hip_atomic_fetch_or(&ctrl->error, ERR_KEYGROUP, __ATOMIC_RELAXED, DEV_SCOPE);
                } else {
                    const int64_t se = slice_end_of(a.win, ts);
                    if (!a.local && win_fired(a.win, se, cur_wm)) {  // TUMBLE: late for its only window
                        ldrop++;
                    } else {
                        lrows++;
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
            if (v) a.run_ovf[(size_t)slot * n_sb + i] = 1u;
            run += v;
        }
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < RPT; it++) {
            const uint32_t o = (uint32_t)(it * BLK + tid);
            const uint32_t r = rrank[o];
            if (r == 0xFFFFu) continue;
            const int64_t key = kp[o], ts = tp[o], acc = vp[o];
            uint32_t m;
            const int32_t sb = route_key(a.ks, key, 0, &m, HK);
            uint64_t* p = out + (size_t)(r + hist[sb]) * PW;
            p[0] = (uint64_t)key;
            p[1] = (uint64_t)slice_end_of(a.win, ts);
            p[2] = (uint64_t)acc;
        }
    }
    const uint32_t fmt = slowc ? PF_WIDE : PF_PACK;
    const uint32_t push_fmt = pk ? PF_PACK : PF_WIDE;  // (uniform over the launch)

    // ---- control counters, as k_ingest: each chunk publishes its stats with agent-scope stores, then
    // takes a ticket; the last workgroup of the launch reduces them into the control block and
    // commits the push's slot
    {
        const int64_t wm = wred_min_i64(lmin);
        const uint32_t wd = wred_sum_u32(ldrop), wr = wred_sum_u32(lrows);
        if ((tid & 63) == 0) {
            if (wm != INT64_MAX) __hip_atomic_fetch_min(s_min, wm, __ATOMIC_RELAXED, LDS_SCOPE);
            if (wd) atomicAdd(s_drop, (unsigned long long)wd);
            if (wr) atomicAdd(s_rows, (unsigned long long)wr);
        }
    }
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(&a.chunk_stats[CS_WORDS * c], *s_min, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&a.chunk_stats[CS_WORDS * c + 1], (int64_t)*s_drop, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&a.chunk_stats[CS_WORDS * c + 2], (int64_t)*s_rows, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&a.chunk_stats[CS_WORDS * c + 3], (int64_t)total, __ATOMIC_RELAXED, DEV_SCOPE);
        __hip_atomic_store(&a.chunk_stats[CS_WORDS * c + 4],
                           (int64_t)total * 8 * pf_stride(fmt, 1) | ((int64_t)(fmt != PF_WIDE) << 40), __ATOMIC_RELAXED,
                           DEV_SCOPE);
#pragma unroll
        for (int q = 0; q < 4; q++) __hip_atomic_store(&a.chunk_stats[CS_WORDS * c + 8 + q], s_pk[q], __ATOMIC_RELAXED, DEV_SCOPE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *s_last = grid_last_wg(a.tickets->c[0]);
    }
    __syncthreads();
    if (!*s_last) return;
    int64_t m = INT64_MAX, d = 0, r = 0, q = 0, y = 0;
    int64_t kmn = INT64_MAX, kmx = INT64_MIN, vmn = INT64_MAX, vmx = INT64_MIN;
    for (int64_t i = tid; i < (int64_t)gridDim.x; i += BLK) {
        const int64_t* cs = a.chunk_stats + CS_WORDS * i;
        m = min(m, __hip_atomic_load(&cs[0], __ATOMIC_RELAXED, DEV_SCOPE));
        d += __hip_atomic_load(&cs[1], __ATOMIC_RELAXED, DEV_SCOPE);
        r += __hip_atomic_load(&cs[2], __ATOMIC_RELAXED, DEV_SCOPE);
        q += __hip_atomic_load(&cs[3], __ATOMIC_RELAXED, DEV_SCOPE);
        y += __hip_atomic_load(&cs[4], __ATOMIC_RELAXED, DEV_SCOPE);  // no carry: < 2^40 per chunk
        kmn = min(kmn, __hip_atomic_load(&cs[8], __ATOMIC_RELAXED, DEV_SCOPE));
        kmx = max(kmx, __hip_atomic_load(&cs[9], __ATOMIC_RELAXED, DEV_SCOPE));
        vmn = min(vmn, __hip_atomic_load(&cs[10], __ATOMIC_RELAXED, DEV_SCOPE));
        vmx = max(vmx, __hip_atomic_load(&cs[11], __ATOMIC_RELAXED, DEV_SCOPE));
    }
    m = wred_min_i64(m);
    d = wred_sum_i64(d);
    r = wred_sum_i64(r);
    q = wred_sum_i64(q);
    y = wred_sum_i64(y);
    kmn = wred_min_i64(kmn);
    kmx = wred_max_i64(kmx);
    vmn = wred_min_i64(vmn);
    vmx = wred_max_i64(vmx);
    int64_t* red = (int64_t*)stage;  // [9][NWV]
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[w] = m;
        red[NWV + w] = d;
        red[2 * NWV + w] = r;
        red[3 * NWV + w] = q;
        red[4 * NWV + w] = y;
        red[5 * NWV + w] = kmn;
        red[6 * NWV + w] = kmx;
        red[7 * NWV + w] = vmn;
        red[8 * NWV + w] = vmx;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll 1
    for (int v = 1; v < NWV; v++) {
        m = min(m, red[v]);
        d += red[NWV + v];
        r += red[2 * NWV + v];
        q += red[3 * NWV + v];
        y += red[4 * NWV + v];
        kmn = min(kmn, red[5 * NWV + v]);
        kmx = max(kmx, red[6 * NWV + v]);
        vmn = min(vmn, red[7 * NWV + v]);
        vmx = max(vmx, red[8 * NWV + v]);
    }
    a.slot_nch[slot] = (int32_t)gridDim.x;
    a.slot_base[slot] = slice_end_of(a.win, wadd(cur_wm, 1));
    a.slot_fmt[slot] = (int32_t)push_fmt;
    ctrl->pending_pushes = slot + 1;
    ctrl->min_pending = min(ctrl->min_pending, m);
    ctrl->pending_rows += (uint64_t)r;
    ctrl->partials += (uint64_t)q;
    ctrl->part_bytes += (uint64_t)(y & ((1ll << 40) - 1));
    ctrl->compact_chunks += (uint64_t)(y >> 40);
    ctrl->push_count += 1;  // (fold_skip stands: this kernel measures no fold)
    ctrl->late_dropped += (uint64_t)d;
    if (slot == 0) {  // this push opened the flush epoch with the parameters it read
        ctrl->pk_cur_k = pk_k;
        ctrl->pk_cur_v = pk_v;
        ctrl->pk_cur_bits = pk_bits;
    }
    ctrl->pk_next_bits = pack_fields(kmn, kmx, vmn, vmx, &ctrl->pk_next_k, &ctrl->pk_next_v, ctrl->pk_next_bits);
    ig_mirror_store(a.tickets, ctrl);
    kt_end(a.kt);
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

template <int HK>
static hipError_t ingest_pack_hk(const IngestArgs& a, hipStream_t s, KTimer* t) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)k_ingest_pack<HK>, hipFuncAttributeMaxDynamicSharedMemorySize, IGP_LDS);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    kt_mark(t, FW_KT_REDUCE, false, s);
    hipLaunchKernelGGL((k_ingest_pack<HK>), dim3((unsigned)a.n_chunks), dim3(IGP_BLOCK), IGP_LDS, s, a);
    kt_mark(t, FW_KT_REDUCE, true, s);
    return hipGetLastError();
}

}  // namespace fw
