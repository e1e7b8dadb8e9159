// fw_folded.hip -- the folded paths' shared part (fw_folded.h): the stable superbucket partition, the
// key-space plan and the placement of restored entries.
//
// The partition groups the rows of one launch by superbucket, arrival order kept inside a group, in
// four stream-ordered launches:
//   k_fd_part     per chunk of FD_TILE rows: route every key to its superbucket, sort (superbucket,
//                 position) in LDS, and write the chunk's rows grouped by superbucket with each row's
//                 rank inside its (chunk, superbucket) group, and the group sizes (hist)
//   k_fd_scan     per superbucket: exclusive scan of its group sizes over the chunks
//   k_fd_seg      exclusive scan of the superbucket totals: segment starts
//   k_fd_scatter  row indices to their segment, input order kept inside a superbucket
// No workgroup waits on another.
// k_fd_part_seg is k_fd_part over a padded exchange receive buffer (fd_partition_segments): the same
// body, with the rows behind a segment's count treated as tile padding.  The unsegmented k_fd_part is
// the instance the count path and direct pushes launch, unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fw_folded.h"

namespace fw {
namespace {

struct PartArgs {
    const int64_t* key;
    const int32_t* khash;
    int64_t n;
    int32_t n_chunks;
    KeySpace ks;
    Ctrl* ctrl;
    int32_t* hist;
    int32_t* s_sb;
    uint32_t* s_row;
    int32_t* s_rank;
};

// The segmented form's view of the launch (fd_partition_segments): the launch's row i is row row0 + i
// of a padded buffer of segments of seg_len rows, live iff its index inside its segment is below
// min(seg_counts[segment], seg_len) (a count above seg_len: the overflow went to the spill, as in the
// ingest's seg_counts test), and its key is a.key[i * stride].
struct PartSegArgs {
    const int64_t* seg_counts;
    int64_t seg_len;
    int64_t row0;
    int32_t stride;
};

// SEG: a padding row is sorted out like tile padding, whatever bytes it holds -- it is not routed,
// so it raises nothing
template <bool SEG>
__device__ __forceinline__ void fd_part_body(const PartArgs& a, const PartSegArgs& g) {
    __shared__ uint64_t sk[FD_TILE];
    __shared__ uint32_t sp[FD_TILE];
    __shared__ int32_t hx[FD_TILE];
    const int t = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * FD_TILE;
    const int nrows = (int)(a.n - c0 < FD_TILE ? a.n - c0 : FD_TILE);
    const int n2 = fd_pow2(nrows);
    int32_t sb = -1;
    bool live = t < nrows;
    if (SEG && live) {
        const int64_t pos = g.row0 + c0 + t;
        const int64_t sg = pos / g.seg_len;
        live = pos - sg * g.seg_len < g.seg_counts[sg];  // (an index is below seg_len already)
    }
    if (live) {
        uint32_t m;
        sb = route_key(a.ks, a.key[SEG ? (c0 + t) * g.stride : c0 + t], a.khash ? a.khash[c0 + t] : 0, &m);
        if (sb < 0 || sb >= a.ks.n_sb) {  // key group outside the subtask's range: the row is dropped
            atomicOr(&a.ctrl->error, ERR_KEYGROUP);
            sb = -1;
        }
    }
    sk[t] = sb >= 0 ? (uint64_t)sb : ~0ull;
    sp[t] = sb >= 0 ? (uint32_t)t : (FD_PAD | (uint32_t)t);
    __syncthreads();
    fd_sort(sk, sp, n2);
    const bool v = t < n2 && !(sp[t] >> 31);
    const bool head = v && (t == 0 || sk[t - 1] != sk[t]);
    hx[t] = head ? t : 0;
    __syncthreads();
    fd_max_scan(hx, n2);
    if (v) {
        const int32_t rank = t - hx[t];
        const int32_t s = (int32_t)sk[t];
        a.s_sb[c0 + t] = s;
        a.s_row[c0 + t] = (uint32_t)(c0 + sp[t]);
        a.s_rank[c0 + t] = rank;
        const bool tail = t == n2 - 1 || (sp[t + 1] >> 31) || sk[t + 1] != sk[t];
        if (tail) a.hist[(size_t)s * a.n_chunks + blockIdx.x] = rank + 1;
    } else if (t < nrows) {
        a.s_sb[c0 + t] = -1;
    }
}

__global__ __launch_bounds__(FD_TILE) void k_fd_part(PartArgs a) { fd_part_body<false>(a, PartSegArgs{}); }
__global__ __launch_bounds__(FD_TILE) void k_fd_part_seg(PartArgs a, PartSegArgs g) { fd_part_body<true>(a, g); }

// superbucket blockIdx.x: hist[sb][0 .. n_chunks) -> its exclusive scan; seg[sb] = the total
__global__ __launch_bounds__(256) void k_fd_scan(int32_t* hist, int32_t* seg, int32_t n_chunks) {
    __shared__ int32_t buf[256];
    int32_t* row = hist + (size_t)blockIdx.x * n_chunks;
    int32_t carry = 0;
    for (int base = 0; base < n_chunks; base += 256) {
        const int i = base + threadIdx.x;
        const int32_t x = i < n_chunks ? row[i] : 0;
        int32_t tot;
        const int32_t inc = fd_block_scan<256>(x, buf, &tot);
        if (i < n_chunks) row[i] = carry + inc - x;
        carry += tot;
    }
    if (threadIdx.x == 0) seg[blockIdx.x] = carry;
}

// seg[0 .. n_sb) totals -> seg[0 .. n_sb] segment starts (one workgroup)
__global__ __launch_bounds__(FD_TILE) void k_fd_seg(int32_t* seg, int32_t n_sb) {
    __shared__ int32_t buf[FD_TILE];
    int32_t carry = 0;
    for (int base = 0; base < n_sb; base += FD_TILE) {
        const int i = base + threadIdx.x;
        const int32_t x = i < n_sb ? seg[i] : 0;
        int32_t tot;
        const int32_t inc = fd_block_scan<FD_TILE>(x, buf, &tot);
        if (i < n_sb) seg[i] = carry + inc - x;
        carry += tot;
    }
    if (threadIdx.x == 0) seg[n_sb] = carry;
}

__global__ __launch_bounds__(256) void k_fd_scatter(int64_t n, int32_t n_chunks, const int32_t* hist, const int32_t* seg,
                                                     const int32_t* s_sb, const uint32_t* s_row, const int32_t* s_rank,
                                                     uint32_t* perm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t sb = s_sb[i];
    if (sb < 0) return;
    const int64_t dst = (int64_t)seg[sb] + hist[(size_t)sb * n_chunks + (i / FD_TILE)] + s_rank[i];
    if (dst < n) perm[dst] = s_row[i];  // (always: the groups' sizes sum to the kept rows)
}

}  // namespace

int fd_plan_keyspace(const fw_config& c, const char* what, KeySpace* ks, FoldedPart* part) {
    ks->hash_kind = c.key_hash;
    ks->max_p = c.max_parallelism;
    ks->maxp_div = make_udiv32((uint32_t)c.max_parallelism);
    ks->kg_start = (c.subtask_index * c.max_parallelism + c.parallelism - 1) / c.parallelism;
    const int kg_end = ((c.subtask_index + 1) * c.max_parallelism - 1) / c.parallelism;
    ks->n_kg = kg_end - ks->kg_start + 1;
    ks->pass_log2 = 0;
    // about 512 hinted entries per superbucket, at most 2048 superbuckets (one fold workgroup each)
    const int64_t hint = std::max<int64_t>(c.state_capacity, 1024);
    part->cap_rows = c.max_batch_rows;
    part->max_nch = (c.max_batch_rows + FD_TILE - 1) / FD_TILE;
    int64_t sbk = fd_next_pow2(((hint + 511) / 512 + ks->n_kg - 1) / ks->n_kg);
    while (sbk > 1 && ((int64_t)ks->n_kg * sbk > 2048 || (int64_t)ks->n_kg * sbk * part->max_nch > FD_MAX_HIST)) sbk >>= 1;
    if ((int64_t)ks->n_kg * sbk * part->max_nch > FD_MAX_HIST)
        return set_error(FW_E_INVALID, "%s: key groups per subtask x max_batch_rows too large for the partition table", what);
    ks->sb_per_kg_log2 = 0;
    while ((1ll << ks->sb_per_kg_log2) < sbk) ks->sb_per_kg_log2++;
    ks->n_sb = ks->n_kg << ks->sb_per_kg_log2;
    return FW_OK;
}

int fd_allocate(FoldedPart* part, const KeySpace& ks) {
    int rc;
    if ((rc = fd_dalloc(&part->hist, (size_t)ks.n_sb * part->max_nch))) return rc;
    if ((rc = fd_dalloc(&part->seg, (size_t)ks.n_sb + 1))) return rc;
    if ((rc = fd_dalloc(&part->s_sb, (size_t)part->cap_rows))) return rc;
    if ((rc = fd_dalloc(&part->s_row, (size_t)part->cap_rows))) return rc;
    if ((rc = fd_dalloc(&part->s_rank, (size_t)part->cap_rows))) return rc;
    return fd_dalloc(&part->perm, (size_t)part->cap_rows);
}

void fd_free(FoldedPart* part) {
    hipFree(part->hist);
    hipFree(part->seg);
    hipFree(part->s_sb);
    hipFree(part->s_row);
    hipFree(part->s_rank);
    hipFree(part->perm);
}

static int fd_partition_launch(const FoldedPart& part, const KeySpace& ks, Ctrl* ctrl, hipStream_t stream, int64_t n,
                               const int64_t* d_key, const int32_t* d_khash, const PartSegArgs* sg) {
    const int n_sb = ks.n_sb;
    const int32_t nch = (int32_t)((n + FD_TILE - 1) / FD_TILE);
    FD_TRY(hipMemsetAsync(part.hist, 0, (size_t)n_sb * nch * 4, stream));
    PartArgs pa{};
    pa.key = d_key;
    pa.khash = d_khash;
    pa.n = n;
    pa.n_chunks = nch;
    pa.ks = ks;
    pa.ctrl = ctrl;
    pa.hist = part.hist;
    pa.s_sb = part.s_sb;
    pa.s_row = part.s_row;
    pa.s_rank = part.s_rank;
    if (sg) hipLaunchKernelGGL(k_fd_part_seg, dim3(nch), dim3(FD_TILE), 0, stream, pa, *sg);
    else hipLaunchKernelGGL(k_fd_part, dim3(nch), dim3(FD_TILE), 0, stream, pa);
    hipLaunchKernelGGL(k_fd_scan, dim3(n_sb), dim3(256), 0, stream, part.hist, part.seg, nch);
    hipLaunchKernelGGL(k_fd_seg, dim3(1), dim3(FD_TILE), 0, stream, part.seg, (int32_t)n_sb);
    hipLaunchKernelGGL(k_fd_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, nch, part.hist, part.seg,
                       part.s_sb, part.s_row, part.s_rank, part.perm);
    return FW_OK;
}

int fd_partition(const FoldedPart& part, const KeySpace& ks, Ctrl* ctrl, hipStream_t stream, int64_t n, const int64_t* d_key,
                 const int32_t* d_khash) {
    return fd_partition_launch(part, ks, ctrl, stream, n, d_key, d_khash, nullptr);
}

int fd_partition_segments(const FoldedPart& part, const KeySpace& ks, Ctrl* ctrl, hipStream_t stream, int64_t n, const int64_t* d_key,
                          int32_t stride, const int32_t* d_khash, const int64_t* d_seg_counts, int64_t seg_len, int64_t row0) {
    const PartSegArgs sg{d_seg_counts, seg_len, row0, stride};
    return fd_partition_launch(part, ks, ctrl, stream, n, d_key, d_khash, &sg);
}

int fd_sb_range(const KeySpace& ks, int32_t key_group, int* sb0, int* sb1) {
    const int li = key_group - ks.kg_start;
    if (li < 0 || li >= ks.n_kg) return set_error(FW_E_INVALID, "key group %d is not owned by this subtask", key_group);
    *sb0 = li << ks.sb_per_kg_log2;
    *sb1 = (li + 1) << ks.sb_per_kg_log2;
    return FW_OK;
}

int fd_restore_sb(const KeySpace& ks, int64_t key, uint64_t where, int sb0, int sb1, int* sb) {
    const int L = ks.sb_per_kg_log2;
    const int kg = (int)(where >> 32);
    if (ks.hash_kind == KH_PRE) {
        // the recorded sub-bucket holds the low quotient bits of the snapshot's split; this handle uses the low L of them
        *sb = ((kg - ks.kg_start) << L) + (int)((uint32_t)where & (uint32_t)((1 << L) - 1));
    } else {
        uint32_t m;
        *sb = route_key(ks, key, 0, &m);
        if (*sb >= 0 && *sb < ks.n_sb && ks.kg_start + (*sb >> L) != kg)
            return set_error(FW_E_INVALID, "entry key does not belong to key group %d", kg);
    }
    if (*sb < sb0 || *sb >= sb1) return set_error(FW_E_INVALID, "snapshot entry of key group %d is not owned by this subtask", kg);
    return FW_OK;
}

int fd_restored_ctrl(const Ctrl* d_ctrl, bool key_group, int64_t n, int64_t watermark, Ctrl* c) {
    FD_TRY(hipMemcpy(c, d_ctrl, sizeof *c, hipMemcpyDeviceToHost));
    if (key_group) {
        c->live_entries += n;
    } else {
        c->live_entries = n;
        c->error = 0;
        c->out_count[0] = 0;
        c->cur = watermark;
    }
    return FW_OK;
}

}  // namespace fw
