// fw_folded.h -- what the folded paths share: the count windows (fw_count.h) and the session windows
// (fw_session.h) fold a push into their state when it is pushed, one workgroup per superbucket walking
// its rows in arrival order.  Both first group the push's rows by superbucket with the same stable
// partition (fw_folded.hip, DESIGN.md "The folded paths' partition"), plan their key space the same
// way and place restored entries by the same rules.
//
// This header holds the workgroup helpers the partition and the two folds use, the partition's
// per-handle buffers (FoldedPart) and the host entry points of fw_folded.hip.
#pragma once
#include <algorithm>

#include "fw_internal.h"

namespace fw {

constexpr int FD_TILE = 1024;                       // rows per tile / partition chunk = threads per workgroup
constexpr int64_t FD_MAX_HIST = (int64_t)1 << 26;   // [superbucket][chunk] partition counters a handle may hold
constexpr uint32_t FD_PAD = 0x80000000u;            // position word of a padding element: sorts after every row

__device__ __forceinline__ int fd_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// (padding, key, position) order; positions are unique, so the order is total and the sort stable
__device__ __forceinline__ bool fd_less(uint64_t ka, uint32_t pa, uint64_t kb, uint32_t pb) {
    const uint32_t ia = pa >> 31, ib = pb >> 31;
    if (ia != ib) return ia < ib;
    if (ka != kb) return ka < kb;
    return pa < pb;
}

// bitonic sort of the first n2 (a power of two <= FD_TILE) pairs; every thread of the workgroup
// calls it, after a barrier behind the stores that filled k / p; it ends with a barrier
__device__ inline void fd_sort(uint64_t* k, uint32_t* p, int n2) {
    const int t = threadIdx.x;
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int x = t ^ j;
            if (t < n2 && x > t) {
                const bool asc = (t & kk) == 0;
                const uint64_t ka = k[t], kb = k[x];
                const uint32_t pa = p[t], pb = p[x];
                if (fd_less(kb, pb, ka, pa) == asc) {
                    k[t] = kb;
                    k[x] = ka;
                    p[t] = pb;
                    p[x] = pa;
                }
            }
            __syncthreads();
        }
}

// inclusive max scan of a[0 .. n2); every thread calls it after a barrier; ends with a barrier
__device__ inline void fd_max_scan(int32_t* a, int n2) {
    const int t = threadIdx.x;
    for (int d = 1; d < n2; d <<= 1) {
        const bool on = t < n2 && t >= d;
        const int32_t v = on ? a[t - d] : 0;
        __syncthreads();
        if (on && v > a[t]) a[t] = v;
        __syncthreads();
    }
}

// inclusive scan over the workgroup's NT threads; every thread calls it; *total = the sum
template <int NT>
__device__ inline int32_t fd_block_scan(int32_t x, int32_t* buf, int32_t* total) {
    const int t = threadIdx.x;
    buf[t] = x;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const int32_t v = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += v;
        __syncthreads();
    }
    const int32_t r = buf[t];
    *total = buf[NT - 1];
    __syncthreads();
    return r;
}

// The partition's per-handle buffers: the scratch of one launch.
struct FoldedPart {
    int64_t cap_rows = 0;          // rows per launch (max_batch_rows)
    int64_t max_nch = 0;           // partition chunks per launch
    int32_t* hist = nullptr;       // [n_sb][n_chunks]: rows of chunk in superbucket, then their exclusive scan
    int32_t* seg = nullptr;        // [n_sb + 1]: rows per superbucket, then segment starts
    int32_t* s_sb = nullptr;       // [cap_rows] chunk-sorted: superbucket (-1: dropped), row, rank in (chunk, sb)
    uint32_t* s_row = nullptr;
    int32_t* s_rank = nullptr;
    uint32_t* perm = nullptr;      // [cap_rows] row indices grouped by superbucket, arrival order inside
};

// error reporting of fw_api.hip (fw_last_error): returns code
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define FD_TRY(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return set_error(FW_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int fd_dalloc(T** p, size_t count) {
    void* v = nullptr;
    FD_TRY(hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T)));
    *p = (T*)v;
    return FW_OK;
}

inline int64_t fd_next_pow2(int64_t x) {
    int64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// The key space of a folded handle and its partition's sizes: the subtask's key groups, each split
// into a power of two of superbuckets.  `what` names the path in the one message ("count windows").
int fd_plan_keyspace(const fw_config& c, const char* what, KeySpace* ks, FoldedPart* part);
int fd_allocate(FoldedPart* part, const KeySpace& ks);
void fd_free(FoldedPart* part);
// part->perm = the n (<= cap_rows) rows' indices grouped by superbucket, arrival order inside, and
// part->seg the groups' starts; a row of a key group the subtask does not own is left out and raises
// ERR_KEYGROUP.  Stream-ordered; the launches' errors are the caller's hipGetLastError to collect.
int fd_partition(const FoldedPart& part, const KeySpace& ks, Ctrl* ctrl, hipStream_t stream, int64_t n, const int64_t* d_key,
                 const int32_t* d_khash);
// The same over a launch's part of a padded exchange receive buffer: n_segs segments of seg_len rows,
// segment s holding min(d_seg_counts[s], seg_len) live rows in front of its padding.  The launch covers
// the buffer's rows [row0, row0 + n) (a call longer than cap_rows is split by buffer position, so a
// segment may straddle launches); its row i has its key at d_key[i * stride] (1: a column, row_words:
// packed rows) and its hash at d_khash[i].  A padding row is left out like a chunk's tile padding: it
// is never routed and raises nothing, whatever bytes it holds; a live row of a foreign key group is
// left out and raises ERR_KEYGROUP.  part->perm holds launch-local indices, buffer position order
// inside a superbucket.
int fd_partition_segments(const FoldedPart& part, const KeySpace& ks, Ctrl* ctrl, hipStream_t stream, int64_t n, const int64_t* d_key,
                          int32_t stride, const int32_t* d_khash, const int64_t* d_seg_counts, int64_t seg_len, int64_t row0);

// ---- snapshot / restore
// the superbuckets [*sb0, *sb1) of key group `key_group`, which the subtask must own
int fd_sb_range(const KeySpace& ks, int32_t key_group, int* sb0, int* sb1);
// *sb = the superbucket of a restored entry whose blob word `where` is key group << 32 | sub-bucket:
// the recorded sub-bucket's for precomputed-hash keys, which carry no hash in the state, else where the
// key routes now; it must be the recorded key group's and inside the restored range [sb0, sb1)
int fd_restore_sb(const KeySpace& ks, int64_t key, uint64_t where, int sb0, int sb1, int* sb);
// *c = the handle's control block as a restore of n entries leaves it: a key group adds its entries, a
// whole-handle restore also clears the error bits and the uncollected rows and takes the watermark.
// The caller adds what is its own and writes *c back.
int fd_restored_ctrl(const Ctrl* d_ctrl, bool key_group, int64_t n, int64_t watermark, Ctrl* c);

}  // namespace fw
