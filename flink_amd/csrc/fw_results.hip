// fw_results.hip -- result delivery of libflinkwin (include/flinkwin.h): the result column sets, the
// compaction of the merge's output slabs and the five ways its rows reach the caller (fw_results with a host
// copy or device pointers, fw_results_async / fw_results_ready, fw_results_device,
// fw_results_device_segments), a count or session handle's rows, and the side channels read like results:
// first-element events, late records, a record count handle's gathered rows.  fw_api.hip plans, allocates,
// pushes and advances; what the two share is declared in fw_handle.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "fw_handle.h"

using namespace fw;

#define fail(...) fw::set_error(__VA_ARGS__)
#define HIP_TRY(expr) FD_TRY(expr)

// ---- column sets
int fw::cols_alloc_device(ResultCols* c, size_t rows, int n_val, bool ws) {
    int rc;
    if ((rc = fd_dalloc(&c->key, rows))) return rc;
    if (ws && (rc = fd_dalloc(&c->ws, rows))) return rc;
    if ((rc = fd_dalloc(&c->we, rows))) return rc;
    if ((rc = fd_dalloc(&c->null, rows))) return rc;
    for (int g = 0; g < n_val; g++)
        if ((rc = fd_dalloc(&c->val[g], rows))) return rc;
    return FW_OK;
}

int fw::cols_alloc_pinned(ResultCols* c, size_t rows, int n_val, unsigned flags) {
    HIP_TRY(hipHostMalloc((void**)&c->key, rows * 8, flags));
    HIP_TRY(hipHostMalloc((void**)&c->ws, rows * 8, flags));
    HIP_TRY(hipHostMalloc((void**)&c->we, rows * 8, flags));
    HIP_TRY(hipHostMalloc((void**)&c->null, rows * 4, flags));
    for (int g = 0; g < n_val; g++) HIP_TRY(hipHostMalloc((void**)&c->val[g], rows * 8, flags));
    return FW_OK;
}

void fw::cols_free(ResultCols* c, bool pinned) {
    auto drop = [pinned](void* p) { pinned ? (void)hipHostFree(p) : (void)hipFree(p); };
    drop(c->key);
    drop(c->ws);
    drop(c->we);
    drop(c->null);
    for (int g = 0; g < FW_MAX_AGGS; g++) drop(c->val[g]);
    *c = ResultCols{};
}

int fw::cols_copy_to_host(const ResultCols& dst, const ResultCols& src, int64_t n, int n_val, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(dst.key, src.key, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(dst.ws, src.ws, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(dst.we, src.we, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (src.null) HIP_TRY(hipMemcpyAsync(dst.null, src.null, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    for (int g = 0; g < n_val; g++) HIP_TRY(hipMemcpyAsync(dst.val[g], src.val[g], (size_t)n * 8, hipMemcpyDeviceToHost, s));
    return FW_OK;
}

namespace {

// out's columns from a set: n_val value columns and, where the rows carry one, the ordinal column
void set_result(fw_result* out, const ResultCols& c, int64_t n, int n_val, const uint64_t* ord) {
    out->n = n;
    out->key = c.key;
    out->window_start = c.ws;
    out->window_end = c.we;
    for (int g = 0; g < n_val; g++) out->values[g] = (int64_t*)c.val[g];
    out->first_ord = (int64_t*)ord;
    out->null_mask = c.null;
}

// a time-window handle's n_out result columns: with first ordinals planned the last one is value1's
// ordinal (fw_result.first_ord), not a value
void set_window_result(const fw_handle* h, fw_result* out, const ResultCols& c, int64_t n) {
    const int na = h->n_out;
    const int nv = h->ad.first_word >= 0 ? na - 1 : na;
    set_result(out, c, n, nv, nv < na ? c.val[nv] : nullptr);
}

// the compaction of the output slabs (and the overflow region) into dst
CompactArgs compact_args(fw_handle* h, const ResultCols& dst) {
    CompactArgs ca{};
    ca.ctrl = h->ctrl;
    ca.sb_out = h->sb_out;
    ca.off = h->coff;
    ca.n_sb = h->ks.n_sb;
    ca.n_aggs = h->n_out;
    ca.slab_cap = h->slab_cap;
    ca.out_key = h->out.key;
    ca.win = device_win(h);
    ca.local_out = h->cfg.agg_phase == FW_PHASE_LOCAL;
    ca.out_we = h->out.we;
    ca.out_null = h->out.null;
    for (int g = 0; g < h->n_out; g++) {
        ca.out_val[g] = h->out.val[g];
        ca.res_val[g] = dst.val[g];
    }
    ca.res_key = dst.key;
    ca.res_ws = dst.ws;
    ca.res_we = dst.we;
    ca.res_null = dst.null;
    ca.res_cap = h->out_cap;
    return ca;
}

// pinned, device-mapped result buffers of fw_results_async
int alloc_async_results(fw_handle* h) {
    if (h->ar_n[0]) return FW_OK;
    const size_t n = (size_t)h->out_cap;
    int rc;
    HIP_TRY(hipStreamCreateWithFlags(&h->d2h_stream, hipStreamNonBlocking));
    for (int b = 0; b < FW_AR_BUFS; b++) {
        // pinned host buffers: mapped for the kernel delivery, plain for the DMA
        if ((rc = cols_alloc_pinned(&h->ar[b], n, h->n_out, h->ar_kernel ? hipHostMallocMapped : hipHostMallocDefault))) return rc;
        HIP_TRY(hipHostMalloc((void**)&h->ar_n[b], 8, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipEventCreateWithFlags(&h->ar_ev[b], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ar_dma_ev[b], hipEventDisableTiming));
        if ((rc = cols_alloc_device(&h->ard[b], n, h->n_out, true))) return rc;
    }
    return FW_OK;
}

// queues the DMA of async result buffer b's n rows into its pinned host buffers on the D2H stream
int ar_enqueue_copy(fw_handle* h, int b, int64_t n) {
    int rc = cols_copy_to_host(h->ar[b], h->ard[b], n, h->n_out, h->d2h_stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ar_dma_ev[b], h->d2h_stream));
    return FW_OK;
}

}  // namespace

// Starts the DMA of the last fw_results_async's rows as soon as its compaction has finished, from
// the calls a pipelined caller makes between fw_results_async and fw_results_ready (the next batch's
// fw_commit / push, fw_advance): the copy then runs beside that batch's kernels and
// fw_results_ready finds it done.  Never blocks; any failure is left for fw_results_ready.
void fw::ar_kick(fw_handle* h) {
    if (h->ar_kernel || !h->d2h_stream) return;
    for (int i = 0; i < h->ar_qn; i++) {  // outstanding collections, oldest first
        const int b = h->ar_q[(h->ar_qhead + i) % FW_AR_BUFS];
        if (h->ar_empty[b] || h->ar_copied[b] || h->ar_inflight[b]) continue;
        if (hipEventQuery(h->ar_ev[b]) != hipSuccess) {  // compaction still queued: try at the next call
            (void)hipGetLastError();
            return;
        }
        const int64_t n = __atomic_load_n(h->ar_n[b], __ATOMIC_ACQUIRE);
        if (n <= 0 || n > h->out_cap) continue;
        if (ar_enqueue_copy(h, b, n) != FW_OK) {
            (void)hipGetLastError();
            return;
        }
        h->ar_inflight[b] = true;
    }
}

// a count or session handle's rows: one per fire, in the device's order; first_ord orders a count handle's as the reference emits
struct FoldedOut {
    ResultCols cols;  // [n_val] value columns (a SQL session handle: one per aggregate)
    int32_t n_val;
    uint64_t* ord;    // NULL: a session handle's rows carry no ordinal
    bool nulls;       // the null mask is written by the device (a SQL session handle); else zeros, and the host copy skips it
    int64_t out_cap;
};
static FoldedOut folded_out(fw_handle* h) {
    if (h->cw.on) {  // (a record handle: values[1] is the ordinal of the record each row is built from)
        const CountOp& c = h->cw;
        return {{c.out_key, c.out_ws, c.out_we, {c.out_val, (uint64_t*)c.out_rord}, c.out_null}, c.rec ? 2 : 1, (uint64_t*)c.out_ord, false,
                c.out_cap};
    }
    const SessionOp& s = h->sw;
    FoldedOut w{{s.out_key, s.out_ws, s.out_we, {}, s.out_null}, s.n_out, nullptr, s.d.sql != 0, s.out_cap};
    for (int g = 0; g < w.n_val; g++) w.cols.val[g] = s.out_val[g];
    return w;
}
static int cw_results(fw_handle* h, fw_result* out, int copy_to_host) {
    const FoldedOut w = folded_out(h);
    Ctrl c;
    int rc = read_ctrl(h, &c);
    if (rc) return rc;
    const int64_t n = (int64_t)c.out_count[0];
    if (n > w.out_cap)
        return fail(FW_E_CAPACITY, "%lld result rows exceed output_capacity %lld (read results more often)", (long long)n,
                    (long long)w.out_cap);
    memset(out, 0, sizeof *out);
    if (!copy_to_host) {
        set_result(out, w.cols, n, w.n_val, w.ord);
        return FW_OK;
    }
    ResultCols src = w.cols;  // what is copied: the ordinals travel as column n_val, a mask of zeros is not read
    int n_cols = w.n_val;
    if (w.ord) src.val[n_cols++] = w.ord;
    if (!w.nulls) src.null = nullptr;
    const ResultCols host = h->r.resize(n, n_cols);
    h->r.null.assign(n, 0u);
    if (n) {
        if ((rc = cols_copy_to_host(host, src, n, n_cols, h->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    set_result(out, host, n, w.n_val, w.ord ? host.val[w.n_val] : nullptr);
    return FW_OK;
}

extern "C" {

int fw_results(fw_handle* h, fw_result* out, int copy_to_host) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    if (h->cw.on || h->sw.on) return cw_results(h, out, copy_to_host);
    if (h->reset_pending) {  // consumed and nothing emitted since
        Ctrl c;
        int rc = read_ctrl(h, &c);
        if (rc) return rc;
        memset(out, 0, sizeof *out);
        return FW_OK;
    }
    HIP_TRY(launch_compact(compact_args(h, h->res), h->stream, h->timer));
    const int32_t krw = h->kr.stride_words - 1;  // image words per result row
    if (h->keyrow)  // each result row's key row, gathered from the table while its id is held
        HIP_TRY(launch_kr_result_rows(h->kr, h->res.key, h->coff + h->ks.n_sb + 1, h->out_cap, h->res_kr_len,
                                      h->res_kr_img, krw, h->stream));
    Ctrl c;
    int rc = read_ctrl(h, &c);
    if (rc) return rc;
    // (more rows than the result columns hold: the compaction raised ERR_OUTPUT, which failed read_ctrl)
    int64_t n = 0;  // the rows the compaction copied, <= out_cap
    HIP_TRY(hipMemcpy(&n, h->coff + h->ks.n_sb + 1, sizeof n, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    if (!copy_to_host) {
        set_window_result(h, out, h->res, n);
        if (h->keyrow) {
            out->key_row_len = h->res_kr_len;
            out->key_row_bytes = (uint8_t*)h->res_kr_img;
            out->key_row_stride = 8ll * krw;
        }
        return FW_OK;
    }
    const ResultCols host = h->r.resize(n, h->n_out);
    if (n && (rc = cols_copy_to_host(host, h->res, n, h->n_out, h->stream))) return rc;
    if (h->keyrow) {
        h->r_kr_len.resize(n);
        h->r_kr_img.resize((size_t)n * krw);
        if (n) {
            HIP_TRY(hipMemcpyAsync(h->r_kr_len.data(), h->res_kr_len, n * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(h->r_kr_img.data(), h->res_kr_img, (size_t)n * krw * 8, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    set_window_result(h, out, host, n);
    if (h->keyrow) {
        out->key_row_len = h->r_kr_len.data();
        out->key_row_bytes = (uint8_t*)h->r_kr_img.data();
        out->key_row_stride = 8ll * krw;
    }
    return FW_OK;
}

int fw_results_async(fw_handle* h) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    CW_REFUSE(h, "fw_results_async");
    if (h->keyrow) return fail(FW_E_INVALID, "key-row operators return their rows through fw_results");
    int rc = alloc_async_results(h);
    if (rc) return rc;
    if (h->ar_qn == FW_AR_BUFS)
        return fail(FW_E_STATE, "%d result collections outstanding: fw_results_ready first", FW_AR_BUFS);
    const int b = h->ar_cur;
    h->ar_cur = (b + 1) % FW_AR_BUFS;
    h->ar_q[(h->ar_qhead + h->ar_qn) % FW_AR_BUFS] = b;
    h->ar_qn++;
    h->ar_empty[b] = h->reset_pending;  // consumed and nothing emitted since
    h->ar_copied[b] = false;
    if (h->ar_inflight[b]) {  // an early DMA of this buffer's previous rows: the compaction waits for it
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ar_dma_ev[b], 0));
        h->ar_inflight[b] = false;
    }
    if (h->ar_empty[b]) return FW_OK;
    const ResultCols& src = h->ard[b];
    CompactArgs ca = compact_args(h, src);
    ca.host_n = mapped(h->ar_n[b]);
    if (!ca.host_n) return fail(FW_E_DEVICE, "mapped result count unavailable");
    HIP_TRY(launch_compact(ca, h->stream, h->timer));
    if (h->ar_kernel) {
        const ResultCols& dst = h->ar[b];
        CopyOutArgs co{};
        co.d_n = h->coff + h->ks.n_sb + 1;
        co.n_aggs = h->n_out;
        co.cap = h->out_cap;
        co.src_key = src.key;
        co.src_ws = src.ws;
        co.src_we = src.we;
        co.src_null = src.null;
        co.dst_key = mapped(dst.key);
        co.dst_ws = mapped(dst.ws);
        co.dst_we = mapped(dst.we);
        co.dst_null = mapped(dst.null);
        for (int g = 0; g < h->n_out; g++) {
            co.src_val[g] = src.val[g];
            co.dst_val[g] = mapped(dst.val[g]);
            if (!co.dst_val[g]) return fail(FW_E_DEVICE, "mapped result buffer unavailable");
        }
        if (!co.dst_key || !co.dst_ws || !co.dst_we || !co.dst_null) return fail(FW_E_DEVICE, "mapped result buffer unavailable");
        HIP_TRY(launch_copy_out(co, h->stream));
        h->ar_copied[b] = true;  // the rows are in host memory once ar_ev[b] has fired
    }
    HIP_TRY(hipEventRecord(h->ar_ev[b], h->stream));
    h->reset_pending = true;  // the rows are collected: the next merge launch starts the slabs afresh
    return FW_OK;
}

int fw_results_device_segments(fw_handle* h, fw_result_segments* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_results_device_segments");
    if (h->keyrow) return fail(FW_E_INVALID, "key-row operators return their rows through fw_results");
    memset(out, 0, sizeof *out);
    out->seg_cap = h->slab_cap;
    out->counts = h->sb_out;
    // (v10: no window_start column, it is derived from window_end (flinkwin.h))
    set_window_result(h, &out->cols, h->out, (int64_t)h->ks.n_sb * h->slab_cap + h->out_cap);
    // consumed and nothing emitted since: no segments (the counts are those of consumed rows)
    out->n_segments = h->reset_pending ? 0 : (int64_t)h->ks.n_sb + 1;
    h->reset_pending = true;  // consumed: the next merge launch starts the slabs afresh
    return FW_OK;
}

int fw_results_device(fw_handle* h, fw_result* out, int64_t** d_n) {
    if (!h || !out || !d_n) return fail(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_results_device");
    if (h->keyrow) return fail(FW_E_INVALID, "key-row operators return their rows through fw_results");
    memset(out, 0, sizeof *out);
    *d_n = h->coff + h->ks.n_sb + 1;
    if (h->reset_pending) {  // consumed and nothing emitted since: zero rows
        HIP_TRY(hipMemsetAsync(*d_n, 0, sizeof(int64_t), h->stream));
    } else {
        HIP_TRY(launch_compact(compact_args(h, h->res), h->stream, h->timer));
        h->reset_pending = true;
    }
    set_window_result(h, out, h->res, h->out_cap);
    return FW_OK;
}

int fw_results_ready(fw_handle* h, fw_result* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_results_ready");
    memset(out, 0, sizeof *out);
    if (h->ar_qn == 0) return fail(FW_E_STATE, "fw_results_ready without an outstanding fw_results_async");
    const int b = h->ar_q[h->ar_qhead];  // the oldest outstanding collection
    h->ar_qhead = (h->ar_qhead + 1) % FW_AR_BUFS;
    h->ar_qn--;
    if (h->ar_empty[b]) return FW_OK;
    HIP_TRY(hipEventSynchronize(h->ar_ev[b]));  // the compaction (long done: it ran a step ago)
    const int64_t n = __atomic_load_n(h->ar_n[b], __ATOMIC_ACQUIRE);
    if (n > h->out_cap)
        return fail(FW_E_CAPACITY, "%lld result rows exceed output_capacity %lld (read results more often)",
                    (long long)n, (long long)h->out_cap);
    if (n > 0 && !h->ar_copied[b]) {  // the rows by DMA on the D2H stream (no CU time, no operator-stream slot)
        if (!h->ar_inflight[b]) {  // not started early by ar_kick
            int rc = ar_enqueue_copy(h, b, n);
            if (rc) return rc;
            h->ar_inflight[b] = true;
        }
        HIP_TRY(hipEventSynchronize(h->ar_dma_ev[b]));
        h->ar_copied[b] = true;
    }
    set_window_result(h, out, h->ar[b], n);
    return FW_OK;
}

int fw_results_reset(fw_handle* h) {
    if (!h) return fail(FW_E_INVALID, "null handle");
    if (h->cw.on || h->sw.on) {  // stream-ordered: rows of pushes issued before the call are consumed, later ones kept
        HIP_TRY(hipMemsetAsync(&h->ctrl->out_count[0], 0, sizeof(uint64_t), h->stream));
        return FW_OK;
    }
    // no launch: the next merge launch starts every output slab and the overflow region afresh
    h->reset_pending = true;
    return FW_OK;
}

int fw_first_element_events(fw_handle* h, fw_ordinal_events* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    const bool rec = h->cw.on && h->cw.rec;  // a record count handle's events: the ordinals its ring slots hold
    if (!rec) {
        CW_REFUSE(h, "fw_first_element_events");
    }
    memset(out, 0, sizeof *out);
    const int64_t* ordev = rec ? h->cw.ordev : h->ordev;
    const int64_t ordev_cap = rec ? h->cw.ordev_cap : h->ordev_cap;
    if (!ordev_cap) return fail(FW_E_STATE, "the operator does not track first elements (ds_first_ordinals = 0)");
    Ctrl c;
    int rc = read_ctrl(h, &c);
    // (a record count handle: an overflow stays readable -- the events that fit, FW_ERRF_ORDEV in fw_get_stats;
    // fw_results keeps failing on the error bit)
    if (rc && !(rec && c.error == ERR_ORDEV)) return rc;
    const int64_t n = std::min<int64_t>(c.n_ordev, ordev_cap);
    std::vector<int64_t> raw((size_t)n);
    if (n) HIP_TRY(hipMemcpy(raw.data(), ordev, (size_t)n * 8, hipMemcpyDeviceToHost));
    const int64_t zero = 0;
    HIP_TRY(hipMemcpy(&h->ctrl->n_ordev, &zero, 8, hipMemcpyHostToDevice));
    h->ev_retain.clear();
    h->ev_release.clear();
    for (int64_t e : raw) {
        if (e & ORDEV_RELEASE) h->ev_release.push_back(e & ~ORDEV_RELEASE);
        else h->ev_retain.push_back(e);
    }
    out->n_retain = (int64_t)h->ev_retain.size();
    out->retain = h->ev_retain.data();
    out->n_release = (int64_t)h->ev_release.size();
    out->release = h->ev_release.data();
    return FW_OK;
}

// The late side output since the last call: up to side_cap rows of `stride` words at d_side, each (key, ts,
// push_seq << 32 | row, value words); value word s of a row belongs to value column col[s] (the columns
// the operator does not load stay 0: the row is named by push_seq, row).  Consumed.
static int late_rows(fw_handle* h, const int64_t* d_side, int64_t side_cap, int stride, int n_words, const int* col, fw_late_rows* out) {
    Ctrl c;
    int rc = read_ctrl(h, &c);
    if (rc) return rc;
    const int64_t n = std::min<int64_t>(c.n_side, side_cap);
    std::vector<int64_t> raw((size_t)n * stride);
    if (n) HIP_TRY(hipMemcpy(raw.data(), d_side, raw.size() * 8, hipMemcpyDeviceToHost));
    const int64_t zero = 0;
    HIP_TRY(hipMemcpy(&h->ctrl->n_side, &zero, 8, hipMemcpyHostToDevice));
    h->lr_key.resize(n);
    h->lr_ts.resize(n);
    h->lr_seq.resize(n);
    h->lr_row.resize(n);
    for (int v = 0; v < h->cfg.n_value_cols; v++) h->lr_val[v].assign(n, 0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t* p = raw.data() + (size_t)i * stride;
        h->lr_key[i] = p[0];
        h->lr_ts[i] = p[1];
        h->lr_seq[i] = (int64_t)((uint64_t)p[2] >> 32);
        h->lr_row[i] = p[2] & 0xffffffffll;
        for (int s = 0; s < n_words; s++) h->lr_val[col[s]][i] = p[3 + s];
    }
    out->n = n;
    out->key = h->lr_key.data();
    out->ts = h->lr_ts.data();
    out->push_seq = h->lr_seq.data();
    out->row = h->lr_row.data();
    for (int v = 0; v < h->cfg.n_value_cols; v++) out->values[v] = h->lr_val[v].data();
    return FW_OK;
}

int fw_late_records(fw_handle* h, fw_late_rows* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    if (h->sw.on) {  // a session handle: the aggregated field (a dynamic-gap handle's gap column stays 0)
        const SessionOp& w = h->sw;
        memset(out, 0, sizeof *out);
        if (!w.side_cap) return fail(FW_E_STATE, "the operator has no late side output (late_side_output = 0)");
        return late_rows(h, w.side, w.side_cap, SW_SIDE_WORDS, w.d.is_count ? 0 : 1, &w.val_col, out);
    }
    CW_REFUSE(h, "fw_late_records");
    memset(out, 0, sizeof *out);
    if (!h->side_cap) return fail(FW_E_STATE, "the operator has no late side output (late_side_output = 0)");
    return late_rows(h, h->side, h->side_cap, SOW, h->nv, h->slot_col, out);  // the loaded value slots
}

int fw_count_record_rows(fw_handle* h, const int64_t* d_rows, int32_t row_words, int64_t n_rows, fw_record_rows* out) {
    if (!h || !out) return fail(FW_E_INVALID, "null argument");
    CW_ONLY_RECORD_EXCHANGE(h, "fw_count_record_rows");
    memset(out, 0, sizeof *out);
    CountOp& w = h->cw;
    const int32_t F = h->cfg.n_value_cols;
    int rc = check_row_words(h, row_words, "fw_count_record_rows");
    if (rc) return rc;
    if (n_rows < 0 || n_rows >= (1ll << 32) || (n_rows > 0 && !d_rows)) return fail(FW_E_INVALID, "fw_count_record_rows: bad rows");
    if (w.push_seq == 0) return fail(FW_E_STATE, "fw_count_record_rows without a push");
    rc = cw_record_rows(&w, d_rows, row_words, n_rows, F);
    if (rc) return rc;
    Ctrl c;
    memset(&c, 0, sizeof c);
    rc = read_ctrl(h, &c);  // the one host wait: behind the push and the gather
    if (rc && c.error != ERR_ORDEV) return rc;  // (an event overflow stays readable, as in fw_first_element_events)
    const int64_t n_ev = std::min<int64_t>(c.n_ordev, w.ordev_cap);
    const int64_t n_res = std::min<int64_t>((int64_t)c.out_count[0], w.out_cap);
    h->rr_ord.resize((size_t)n_ev);
    h->rr_rord.resize((size_t)n_res);
    if (n_ev) HIP_TRY(hipMemcpy(h->rr_ord.data(), w.ordev, (size_t)n_ev * 8, hipMemcpyDeviceToHost));
    if (n_res) HIP_TRY(hipMemcpy(h->rr_rord.data(), w.out_rord, (size_t)n_res * 8, hipMemcpyDeviceToHost));
    const uint64_t seq = (uint64_t)(w.push_seq - 1);
    h->rr_is_retain.assign((size_t)n_ev, 0);
    h->rr_from_push.assign((size_t)n_res, 0);
    for (int64_t i = 0; i < n_ev; i++) {  // nothing is consumed before every named row is known to lie in the buffer
        const int64_t e = h->rr_ord[i];
        if (e & ORDEV_RELEASE) continue;
        h->rr_is_retain[i] = 1;
        if (((uint64_t)e >> 32) != seq)
            return fail(FW_E_INVALID, "fw_count_record_rows: a retain event names push %lld, not the last push %lld (call it after every push)",
                        (long long)((uint64_t)e >> 32), (long long)seq);
        if ((e & 0xffffffffll) >= n_rows)
            return fail(FW_E_INVALID, "fw_count_record_rows: a retain event names row %lld of the push, n_rows is %lld",
                        (long long)(e & 0xffffffffll), (long long)n_rows);
    }
    for (int64_t i = 0; i < n_res; i++) {
        const uint64_t o = (uint64_t)h->rr_rord[i];
        if ((o >> 32) != seq) continue;
        h->rr_from_push[i] = 1;
        if ((int64_t)(o & 0xffffffffull) >= n_rows)
            return fail(FW_E_INVALID, "fw_count_record_rows: a result names row %lld of the push, n_rows is %lld",
                        (long long)(o & 0xffffffffull), (long long)n_rows);
    }
    h->rr_ev_words.resize((size_t)n_ev * F);
    h->rr_res_words.resize((size_t)n_res * F);
    if (n_ev) HIP_TRY(hipMemcpy(h->rr_ev_words.data(), w.g_ev, (size_t)n_ev * F * 8, hipMemcpyDeviceToHost));
    if (n_res) HIP_TRY(hipMemcpy(h->rr_res_words.data(), w.g_res, (size_t)n_res * F * 8, hipMemcpyDeviceToHost));
    const int64_t zero = 0;
    HIP_TRY(hipMemcpy(&h->ctrl->n_ordev, &zero, 8, hipMemcpyHostToDevice));
    for (int64_t i = 0; i < n_ev; i++) {
        h->rr_ord[i] &= ~ORDEV_RELEASE;
        if (!h->rr_is_retain[i]) memset(h->rr_ev_words.data() + (size_t)i * F, 0, (size_t)F * 8);
    }
    for (int64_t i = 0; i < n_res; i++)
        if (!h->rr_from_push[i]) memset(h->rr_res_words.data() + (size_t)i * F, 0, (size_t)F * 8);
    out->n_fields = F;
    out->n_ev = n_ev;
    out->ev_ord = h->rr_ord.data();
    out->ev_is_retain = h->rr_is_retain.data();
    out->ev_words = h->rr_ev_words.data();
    out->n_res = n_res;
    out->res_words = h->rr_res_words.data();
    out->res_from_push = h->rr_from_push.data();
    return FW_OK;
}

}  // extern "C"
