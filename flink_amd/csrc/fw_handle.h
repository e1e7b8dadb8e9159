// fw_handle.h -- the operator handle behind the C-ABI (include/flinkwin.h), private to the library:
// fw_api.hip creates, drives and destroys it, fw_results.hip delivers its rows, fw_checkpoint.hip
// collects its time-window state and installs restored state.  Also the few helpers these host files
// share and the entry points' refusal macros.  Host translation units only.
#pragma once
#include <vector>

#include "fw_count.h"
#include "fw_session.h"
#include "fw_internal.h"

namespace fw {

// One set of result columns: pointers only, no ownership.  val[] holds the handle's n_out result columns.
struct ResultCols {
    int64_t* key = nullptr;
    int64_t* ws = nullptr;
    int64_t* we = nullptr;
    uint64_t* val[FW_MAX_AGGS] = {};
    uint32_t* null = nullptr;
};

// the host copies fw_results returns
struct ResultVecs {
    std::vector<int64_t> key, ws, we;
    std::vector<uint64_t> val[FW_MAX_AGGS];
    std::vector<uint32_t> null;
    ResultCols resize(int64_t n, int n_val) {  // n rows of n_val value columns, as a column set
        key.resize(n);
        ws.resize(n);
        we.resize(n);
        null.resize(n);
        ResultCols c{key.data(), ws.data(), we.data(), {}, null.data()};
        for (int g = 0; g < n_val; g++) {
            val[g].resize(n);
            c.val[g] = val[g].data();
        }
        return c;
    }
};

}  // namespace fw

struct fw_handle {
    fw_config cfg;
    fw::CountOp cw;  // FW_WIN_COUNT / FW_WIN_COUNT_RECORD (cw.rec): the count-window state (cw.on); the time-window members below stay unused
    fw::SessionOp sw;  // FW_WIN_SESSION: the session-window state (sw.on), likewise
    hipStream_t stream = nullptr;
    fw::WinDesc win{};
    fw::KeySpace ks{};
    fw::WordDesc wd{};
    fw::AggDesc ad{};
    int nv = 0;
    int slot_col[fw::MAX_KCOLS] = {};
    int nw_t = 1;  // template word count (layout stride)
    int pwe = 4;   // words per state entry: key, slice (HOP block: block start), flags, accumulator words
    int n_out = 1; // result value columns (aggregates; LOCAL phase: accumulator fields)
    int64_t cap_rows = 0;     // rows per partial-buffer slot (= max rows per push piece)
    int64_t chunk_rows = 0;   // rows per ingest chunk (IG_BLOCK * ig_rpt(nw_t))
    int64_t max_nch = 0;      // ingest chunks per push piece
    int cap_e = 1024;
    bool always_flush = false;

    fw::Ctrl* ctrl = nullptr;
    uint64_t* parts = nullptr;
    int32_t narrow = 0;          // compact partial rows (IngestArgs::narrow)
    int32_t pack = 0;            // PF_PACK run rows (IngestArgs::pack)
    int64_t* slot_base = nullptr;  // [FW_MAX_PENDING] rank base of each pending push
    uint8_t* ranks = nullptr;      // [FW_MAX_PENDING][cap_rows] rank bytes of compact rows
    int64_t cell_cols = 0;       // cell_pad(max_nch): cells per superbucket per slot
    uint32_t* cells = nullptr;   // [FW_MAX_PENDING][cell_cols / 16][n_sb][16] (cell_index)
    int32_t* slot_nch = nullptr;  // [FW_MAX_PENDING]
    // runs (IngestArgs::runs): superbucket-contiguous partial rows; run_rows == 0: off
    int64_t run_rows = 0;
    int32_t sub_cap = 0;
    uint64_t* runs = nullptr;
    uint8_t* run_ranks = nullptr;
    uint32_t* run_fill = nullptr;
    uint32_t* run_ovf = nullptr;
    int32_t* slot_fmt = nullptr;
    int64_t* treq = nullptr;
    int64_t treq_cap = 0;
    uint64_t* lfire = nullptr;   // DataStream late-fire rows
    int64_t lfire_cap = 0;
    int64_t* side = nullptr;     // DataStream late side-output rows
    int64_t side_cap = 0;
    int64_t* ordev = nullptr;    // DataStream first-element retain / release events
    int64_t ordev_cap = 0;
    std::vector<int64_t> ev_retain, ev_release;  // fw_first_element_events copies
    std::vector<int64_t> rr_ord, rr_rord, rr_ev_words, rr_res_words;  // fw_count_record_rows copies (rr_rord: the result rows' values[1])
    std::vector<uint8_t> rr_is_retain, rr_from_push;
    int32_t push_seq = 0;        // fw_commit / fw_push_device calls (side-output row ids)
    std::vector<int64_t> tz_utc, tz_off, tz_bound;  // shift-zone table (host copy)
    int64_t* d_tz = nullptr;     // device copy: [utc | off | bound]
    std::vector<int64_t> lr_key, lr_ts, lr_seq, lr_row, lr_val[FW_MAX_COLS];  // fw_late_records copies
    uint64_t* state = nullptr;
    int32_t* state_count = nullptr;
    int64_t* sb_min_timer = nullptr;
    uint8_t* sb_nar = nullptr;  // HOP block state: superbucket written in the narrow layout
    int hb_narrow = 2;           // narrowest HOP block layout level (FW_HB_NARROW=0/1: development A/B)
    fw::ResultCols out;        // where the merge writes its rows: a slab per superbucket, then the overflow region (out.ws stays null)
    int64_t out_cap = 0;       // result rows between resets (= overflow region rows)
    int64_t slab_cap = 0;      // output slab rows per superbucket
    int32_t* sb_out = nullptr;
    uint32_t* sb_fired = nullptr;
    int64_t* chunk_stats = nullptr;
    fw::Tickets* tickets = nullptr;  // last-workgroup election counters of k_ingest / k_merge_fire
    int64_t* coff = nullptr;   // compaction offsets [n_sb + 2]
    fw::ResultCols res;        // the compacted rows (fw_results, fw_results_device)

    // host-staged ingest (FW_STAGE_BUFS pinned column sets)
    int64_t stage_cap = 0;
    int stage_cur = 0;
    int64_t* h_key[fw::FW_STAGE_BUFS] = {};
    int64_t* h_ts[fw::FW_STAGE_BUFS] = {};
    int32_t* h_kh[fw::FW_STAGE_BUFS] = {};
    int64_t* h_val[fw::FW_STAGE_BUFS][FW_MAX_COLS] = {};
    uint8_t* h_nul[fw::FW_STAGE_BUFS][FW_MAX_COLS] = {};
    hipEvent_t stage_ev[fw::FW_STAGE_BUFS] = {};   // H2D from host buffer b done (copy stream)
    // device staging, one set per host set: batch b+1 crosses PCIe on the copy stream while batch b
    // is ingested on the operator stream
    hipStream_t cstream = nullptr;
    hipEvent_t dstage_free[fw::FW_STAGE_BUFS] = {};  // the ingest that read device buffer b has run (operator stream)
    int64_t* d_key[fw::FW_STAGE_BUFS] = {};
    int64_t* d_ts[fw::FW_STAGE_BUFS] = {};
    int32_t* d_kh[fw::FW_STAGE_BUFS] = {};
    int64_t* d_val[fw::FW_STAGE_BUFS][FW_MAX_COLS] = {};
    uint8_t* d_nul[fw::FW_STAGE_BUFS][FW_MAX_COLS] = {};
    // fw_commit_delta32: the 32-bit delta columns of staging set b, FW_PACK_COLS slices of pack_stride
    uint32_t* d_pack[fw::FW_STAGE_BUFS] = {};
    int64_t pack_stride = 0;
    int64_t reserved = -1;

    // asynchronous result delivery (fw_results_async / fw_results_ready): rows compacted on the
    // device into one of FW_AR_BUFS device buffers (ard), then moved into pinned host buffers
    // (ar); only the row count goes through mapped memory.  Up to FW_AR_BUFS collections are
    // outstanding; fw_results_ready returns the oldest (ar_q, a FIFO of buffer indices)
    fw::ResultCols ard[fw::FW_AR_BUFS];
    hipStream_t d2h_stream = nullptr;
    fw::ResultCols ar[fw::FW_AR_BUFS];
    int64_t* ar_n[fw::FW_AR_BUFS] = {};          // row count (written by the compaction kernel)
    hipEvent_t ar_ev[fw::FW_AR_BUFS] = {};
    hipEvent_t ar_dma_ev[fw::FW_AR_BUFS] = {};   // the DMA of buffer b's rows (started early by ar_kick)
    bool ar_copied[fw::FW_AR_BUFS] = {};         // buffer b's rows are (or are queued to be) in host memory
    bool ar_inflight[fw::FW_AR_BUFS] = {};       // buffer b's DMA is queued (ar_kick), fw_results_ready waits for it
    // async result delivery: CU stores of the compacted rows into mapped pinned host memory (1, the
    // default), or DMA on the D2H stream (FW_AR_KERNEL=0).  Measured round 5 (CFG2 end to end):
    // the DMA queues behind the next batch's H2D on the copy engine, so fw_results_ready waited
    // 2.2 ms per step (1.18 G ev/s); the kernel stores run beside that H2D: 1.1 ms (1.64 G ev/s)
    int ar_kernel = 1;
    int ar_cur = 0;                 // buffer of the next fw_results_async
    int ar_q[fw::FW_AR_BUFS] = {};      // outstanding collections, oldest first
    int ar_qhead = 0, ar_qn = 0;
    bool ar_empty[fw::FW_AR_BUFS] = {}; // that call had nothing to collect

    // FW_KEYHASH_KEYROW: the key-row intern table, per-push intern output, key-row staging
    bool keyrow = false;
    fw::KeyRowTable kr{};
    int64_t kr_scratch_n = 0;
    int64_t* d_kid = nullptr;       // interned ids of the push being ingested
    int32_t* d_khash = nullptr;     // their hashCodes
    int64_t* h_kro[fw::FW_STAGE_BUFS] = {};         // pinned staging: key row offsets / bytes (fw_reserve)
    uint8_t* h_krb[fw::FW_STAGE_BUFS] = {};
    int64_t krb_cap = 0;            // staging bytes per batch
    int64_t* d_kro[fw::FW_STAGE_BUFS] = {};
    uint8_t* d_krb[fw::FW_STAGE_BUFS] = {};
    int32_t* res_kr_len = nullptr;  // result key rows (fw_results)
    uint64_t* res_kr_img = nullptr;
    std::vector<int32_t> r_kr_len;
    std::vector<uint64_t> r_kr_img;

    fw::ResultVecs r;  // host copies of results

    int64_t pushes_ub = 0;  // upper bound of device pending_pushes
    // pending-push mirror: host-mapped word written by each merge launch (MergeArgs::host_mirror)
    volatile unsigned long long* mirror = nullptr;
    unsigned long long* d_mirror = nullptr;
    uint64_t merge_seq = 0;         // merge launches so far
    uint64_t pushes_total = 0;      // ingest launches so far
    uint64_t pushes_at_merge[64] = {};  // pushes_total when merge launch (seq % 64) was issued
    bool reset_pending = false;  // fw_results_reset called: the next merge launch empties the results
    int64_t host_cur = INT64_MIN;
    // the device's currentProgress / nextTriggerProgress as the launched merges leave them (mirrored
    // on the host from the watermarks it launched; merge_finalize applies the same rule), so fw_advance
    // can tell a watermark that crosses no slice end -- the merge launch would change nothing -- and
    // skip it (FW_SKIP_IDLE=0: launch every advance)
    int64_t dev_cur = INT64_MIN;
    int64_t dev_ntp = INT64_MIN;
    bool skip_idle = true;
    fw::KTimer* timer = nullptr;  // non-null while fw_set_profiling is on
    int ablate = 0;           // FW_ABLATE (development timing builds only; results are wrong)
    int fold_always = 0;      // FW_FOLD=1 (development A/B): no adaptive fold skip
    // k_ingest_pack (fw_ingest_pack.h): FW_IG_PACK 0 never, 1 (default) by fw_host_ig_pack_choice (the
    // last completed push left the LDS fold skipped and valid PF_PACK fields, a flush epoch has been
    // opened, no fold measurement is due), 2 on every push of an eligible handle (tests)
    int ig_pack_mode = 1;
    // k_ingest_pack's geometry (fw_internal.h).  FW_IGP_GEOM=0/1 fixes it (A/B, tests); otherwise (-1) each
    // launch takes the 256 x 16 geometry when that makes the whole push resident and 512 x 8 does not
    // (more chunks than igp_res[0], at most igp_res[1]: workgroups per CU x CUs), else 512 x 8, which
    // is faster at every other size
    int igp_geom = -1;
    int igp_last = 0;             // geometry of the last k_ingest_pack launch
    int64_t igp_res[2] = {0, 0};  // chunks resident at once per geometry
    uint64_t ig_since_fold = 0;      // pushes since the last one on which k_ingest folded (that one included)
    uint64_t ig_merges = 0;          // merge launches since the control block was initialised
    bool mg_tag = false;      // planned: the merge launches its GF_TAG variant (tag path for PF_PACK flushes)
    bool ig_pack_ok = false;  // planned: the handle's pushes are ones k_ingest_pack serves
    // ingest mirror: host-mapped word written after each ingest launch (Tickets::ig_mirror)
    volatile unsigned long long* ig_mirror = nullptr;
    unsigned long long* d_ig_mirror = nullptr;
    uint64_t ig_pushes = 0;          // ingest launches since the control block was initialised (Ctrl::push_count)
    int64_t ig_pack_launches = 0;    // of all launches, the ones k_ingest_pack took
    int fill_pct = 75;        // superbucket LDS fill target (FW_FILL_PCT: development A/B)
    unsigned long long* stamps = nullptr;  // [N_STAMPS] merge phase cycles (FW_ABLATE & AB_STAMPS)
    unsigned long long* kt_dev = nullptr;  // [FW_KT_N][KT_WORDS] in-kernel launch timing
    int kt_device = 0;                     // fw_set_profiling(FW_PROF_DEVICE) is on
};

namespace fw {

// fw_api.hip.  The control block, read behind everything queued on the handle's stream; a device
// error bit set in it is FW_E_CAPACITY
int read_ctrl(fw_handle* h, Ctrl* out);
// folds every pending push into the state (prepareSnapshotPreBarrier -> windowBuffer.flush())
int force_flush(fw_handle* h);
// interns n key-row images (device) into the table: d_kid / d_khash hold their ids and hashCodes
int kr_intern(fw_handle* h, int64_t n, const int64_t* d_off, const uint8_t* d_bytes);
// the window description the kernels get: the shift-zone table pointers are the device copy's
WinDesc device_win(const fw_handle* h);
// a packed row is (key, ts or an unread word, the value columns).  `name`: the entry's name for the record
// entries' wording, null for the plain one
int check_row_words(const fw_handle* h, int32_t row_words, const char* name);

// fw_results.hip.  Column sets: `rows` rows of n_val value columns on the device (ws: with a window_start
// column) or pinned (hipHostMalloc flags); freeing takes every pointer of the set; the copy queues n rows
// of src into dst (host memory) on a stream
int cols_alloc_device(ResultCols* c, size_t rows, int n_val, bool ws);
int cols_alloc_pinned(ResultCols* c, size_t rows, int n_val, unsigned flags);
void cols_free(ResultCols* c, bool pinned);
int cols_copy_to_host(const ResultCols& dst, const ResultCols& src, int64_t n, int n_val, hipStream_t s);
// starts the DMA of a finished fw_results_async early, from the calls made before fw_results_ready; never blocks
void ar_kick(fw_handle* h);

template <typename T>
T* mapped(T* host) {
    void* d = nullptr;
    return hipHostGetDevicePointer(&d, (void*)host, 0) == hipSuccess ? (T*)d : nullptr;
}

}  // namespace fw

// entry points a count handle (FW_WIN_COUNT) or a session handle (FW_WIN_SESSION) does not have
#define CW_REFUSE(h, name)                                                                \
    if ((h)->cw.on) return fw::set_error(FW_E_INVALID, name ": not for count windows");   \
    if ((h)->sw.on) return fw::set_error(FW_E_INVALID, name ": not for session windows")
// The push entry points behind the N > 1 keyBy exchange (fw_push_device_segments,
// fw_push_device_packed_segments; fw_advance_device likewise): a session handle has them iff its
// configuration has parallelism > 1 -- only such a handle has an exchange in front of it.  One of
// parallelism 1 refuses them as ever, and so does every count handle.
// A record count handle (FW_WIN_COUNT_RECORD) has no key-group checkpoint -- a restored key group's
// records would have to be re-numbered under fresh ordinals -- and an exchange entry of its own
// (fw_push_device_count_record_packed_segments): the count handle's two segment pushes stay refused.
#define CW_REFUSE_RECORD(h, name)                                                                                       \
    if ((h)->cw.on && (h)->cw.rec)                                                                                      \
        return fw::set_error(FW_E_INVALID, name ": not for record count windows (FW_WIN_COUNT_RECORD: retained records are not re-numbered)")
// The record count handle's own exchange entries (fw_push_device_count_record_packed_segments,
// fw_count_record_rows): the count handle's two segment pushes keep refusing it.
#define CW_ONLY_RECORD_EXCHANGE(h, name)                                                                                   \
    if ((h)->sw.on) return fw::set_error(FW_E_INVALID, name ": not for session windows (record count windows only)");      \
    if (!(h)->cw.on) return fw::set_error(FW_E_INVALID, name ": not for time windows (record count windows only)");        \
    if (!(h)->cw.rec)                                                                                                      \
        return fw::set_error(FW_E_INVALID, name ": not for count windows (FW_WIN_COUNT: fw_push_device_count_packed_segments)"); \
    if ((h)->cfg.parallelism <= 1)                                                                                         \
        return fw::set_error(FW_E_INVALID, name ": a record count handle of parallelism 1 has no keyBy exchange in front of it")
#define CW_REFUSE_EXCHANGE(h, name)                                                       \
    if ((h)->cw.on) return fw::set_error(FW_E_INVALID, name ": not for count windows");   \
    if ((h)->sw.on && (h)->cfg.parallelism <= 1) return fw::set_error(FW_E_INVALID, name ": not for session windows")
