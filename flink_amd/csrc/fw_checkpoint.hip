// fw_checkpoint.hip -- the time-window path's checkpoint entry points (include/flinkwin.h) and the
// steps of a checkpoint that touch the device.  An export is collect -> encode, a restore decode ->
// install: kg_collect / snap_collect gather a handle's state into the in-memory form of
// fw_ckpt_format.h, whose codecs write and read the four formats on the host alone, and kg_install /
// snap_install put a decoded state into a handle.  A blob the decoder refuses never reaches install,
// so it leaves the handle as it was.  (The count and session paths keep their own blobs: cw_snapshot,
// sw_snapshot.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "fw_ckpt_format.h"
#include "fw_handle.h"

using namespace fw;

namespace {

// Fingerprint of everything that gives the stored words their meaning: API, phase, window kind,
// size, slice interval, offset, key hashing, maxParallelism and the accumulator word layout (op,
// value column, NULL gate per word).  A blob is only restored into an operator with the same one.
uint64_t semantics_fingerprint(const fw_handle* h) {
    uint64_t x = 0xcbf29ce484222325ull;
    auto mix = [&](int64_t v) {
        for (int b = 0; b < 8; b++) {
            x ^= (uint64_t)((v >> (8 * b)) & 0xff);
            x *= 0x100000001b3ull;
        }
    };
    const fw_config& c = h->cfg;
    mix(c.api);
    mix(c.agg_phase);
    mix(h->win.kind);
    mix(h->win.size);
    mix(h->win.interval);
    mix(h->win.offset);
    mix(h->cfg.key_hash);
    mix(h->ks.max_p);
    mix(c.allowed_lateness_ms);
    mix(c.tz_use_dst);
    for (size_t i = 0; i < h->tz_utc.size(); i++) {
        mix(h->tz_utc[i]);
        mix(h->tz_off[i]);
    }
    mix(h->wd.nw);
    for (int w = 0; w < h->wd.nw; w++) {
        mix(h->wd.op[w]);
        mix(h->slot_col[h->wd.col[w]]);
        mix(h->wd.gate[w]);
    }
    return x;
}

CkLayout layout_of(const fw_handle* h) {
    return CkLayout{h->ks.n_sb,  h->cap_e,     h->pwe,          h->wd.nw,  h->nw_t,         h->ks.sb_per_kg_log2,
                    h->ks.kg_start, h->ks.n_kg, h->cfg.key_hash, h->keyrow, h->kr.cap_ids,   (int32_t)h->kr.max_len,
                    h->win.size, h->win.interval, semantics_fingerprint(h)};
}

CkPlan plan_of(const fw_handle* h) { return CkPlan{h->cfg, h->win, h->wd, h->ad, h->ks, h->nw_t, h->pwe, h->keyrow}; }

// the first n entries of superbucket sb, in the wide layout (key, slice, flags, words) whatever the
// layout the last write-back chose (HOP block state may be narrow, hb_narrow_words)
int state_rows_to_host(const fw_handle* h, size_t sb, int64_t n, uint64_t* out) {
    const int pwe = h->pwe;
    const uint64_t* src = h->state + sb * h->cap_e * pwe;
    uint8_t nar = 0;
    if (h->win.hopb) FD_TRY(hipMemcpy(&nar, h->sb_nar + sb, 1, hipMemcpyDeviceToHost));
    if (!nar) {
        FD_TRY(hipMemcpy(out, src, (size_t)n * pwe * 8, hipMemcpyDeviceToHost));
        return FW_OK;
    }
    const int nw = h->nw_t, pwn = hb_narrow_words(nw, nar), sbytes = hb_slot_bytes(nar);
    uint64_t none[MAX_WORDS];
    acc_identity(h->wd, nw, none);
    std::vector<uint64_t> tmp((size_t)n * pwn);
    FD_TRY(hipMemcpy(tmp.data(), src, tmp.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {
        const uint8_t* q = (const uint8_t*)(tmp.data() + (size_t)i * pwn);
        uint64_t* e = out + (size_t)i * pwe;
        uint32_t bi;
        uint16_t fl;
        memcpy(&e[0], q, 8);
        memcpy(&bi, q + 8, 4);  // block index: block start = index * hb_span + offset
        memcpy(&fl, q + 12, 2);
        e[1] = (uint64_t)wadd((int64_t)bi * h->win.hb_span, h->win.offset);
        e[2] = fl;
        const uint32_t mask = (uint32_t)fl >> HB_MASK_SHIFT;
        for (int s = 0; s < HB_R; s++)
            for (int x = 0; x < nw; x++) {
                const uint8_t* f = q + HB_HDR_BYTES + sbytes * (s * nw + x);
                int64_t v;
                if (sbytes == 4) {
                    int32_t t;
                    memcpy(&t, f, 4);
                    v = t;
                } else {
                    int16_t t;
                    memcpy(&t, f, 2);
                    v = t;
                }
                e[3 + s * nw + x] = ((mask >> s) & 1u) ? (uint64_t)v : none[x];
            }
    }
    return FW_OK;
}

// earliest watermark-visible time of an entry's timers, as a window end (is_fired(x, W) <=> due):
// the maxTimestamp timer at its window end, a DataStream cleanup timer at cleanupTime + 1
int64_t entry_timer_end(const fw_handle* h, int64_t slice, uint64_t flags) {
    if (h->win.hopb) {  // block entry: no window of it is due before its oldest slice with data
        const uint32_t mask = (uint32_t)flags >> 8;
        for (int i = 0; i < HB_R; i++)
            if ((mask >> i) & 1u) return wadd(slice, (int64_t)(i + 1) * h->win.interval);
        return INT64_MAX;
    }
    int64_t m = (flags & F_TIMER) ? slice : INT64_MAX;
    if (h->win.ds && (flags & F_CLEAN)) m = std::min(m, wadd(ds_cleanup_time(h->win, slice), 1));
    return m;
}

// ---- collect: flush, the control block, the counts, the entries, their key rows

// the entries of the n_sb superbuckets from sb0 on: their counts, then the entries in that order
int rows_collect(fw_handle* h, size_t sb0, int n_sb, std::vector<int32_t>* cnt, std::vector<uint64_t>* ent) {
    cnt->resize((size_t)n_sb);
    FD_TRY(hipMemcpy(cnt->data(), h->state_count + sb0, sizeof(int32_t) * n_sb, hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (int32_t c : *cnt) total += c;
    ent->resize((size_t)total * h->pwe);
    uint64_t* e = ent->data();
    for (int q = 0; q < n_sb; q++) {
        if (!(*cnt)[q]) continue;
        if (const int rc = state_rows_to_host(h, sb0 + q, (*cnt)[q], e)) return rc;
        e += (size_t)(*cnt)[q] * h->pwe;
    }
    return FW_OK;
}

// the key row of every id the entries use, from the arena (c: the control block just read)
int kr_collect(fw_handle* h, const Ctrl& c, const std::vector<uint64_t>& ent, KeyRows* out) {
    *out = KeyRows{};
    if (!h->keyrow) return FW_OK;
    std::vector<int64_t> ids;
    ids.reserve(ent.size() / h->pwe);
    for (size_t i = 0; i < ent.size(); i += (size_t)h->pwe) ids.push_back((int64_t)ent[i]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    if (ids.empty()) return FW_OK;
    if (ids.front() < 0 || ids.back() >= c.kr_next_id) return set_error(FW_E_STATE, "state entry with an unknown key row id");
    const int64_t sw = h->kr.stride_words;
    std::vector<uint64_t> rows((size_t)(ids.back() + 1) * sw);
    FD_TRY(hipMemcpy(rows.data(), h->kr.arena, rows.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t id : ids) {
        const uint64_t* r = rows.data() + (size_t)id * sw;  // [hash << 32 | length, image words]
        out->add(id, (uint32_t)(r[0] >> 32), r + 1, (int64_t)((uint32_t)r[0] & ~7u));
    }
    return FW_OK;
}

int kg_collect(fw_handle* h, int32_t key_group, KgState* out) {
    const KeySpace& ks = h->ks;
    int rc = force_flush(h);  // prepareSnapshotPreBarrier -> windowBuffer.flush()
    if (rc) return rc;
    Ctrl c;
    if ((rc = read_ctrl(h, &c))) return rc;
    const int L = ks.sb_per_kg_log2, pwe = h->pwe;
    std::vector<int32_t> cnt;
    if ((rc = rows_collect(h, (size_t)(key_group - ks.kg_start) << L, 1 << L, &cnt, &out->ent))) return rc;
    uint64_t* e = out->ent.data();
    for (int q = 0; q < (1 << L); q++)  // the sub-bucket an entry came from, beside its flags
        for (int i = 0; i < cnt[q]; i++, e += pwe) e[2] = (uint32_t)e[2] | ((uint64_t)q << 32);
    out->key_group = key_group;
    out->sb_log2 = L;
    out->cur = std::max(c.cur, h->host_cur);
    out->push_seq = (int64_t)h->push_seq;
    return kr_collect(h, c, out->ent, &out->kr);
}

int snap_collect(fw_handle* h, SnapState* out) {
    int rc = force_flush(h);  // prepareSnapshotPreBarrier -> windowBuffer.flush()
    if (rc) return rc;
    Ctrl c;
    if ((rc = read_ctrl(h, &c))) return rc;
    if ((rc = rows_collect(h, 0, h->ks.n_sb, &out->cnt, &out->ent))) return rc;
    out->cur = std::max(c.cur, h->host_cur);
    out->late_dropped = (int64_t)c.late_dropped;
    out->fired = 0;
    out->push_seq = (int64_t)h->push_seq;
    return kr_collect(h, c, out->ent, &out->kr);
}

// ---- install

// interns a decoded state's key rows: (the blob's id, this handle's id) sorted by the former, and
// the hash that routes each (BinaryRowData.hashCode), in that order
int kr_install(fw_handle* h, const KeyRows& kr, std::vector<std::pair<int64_t, int64_t>>* map, std::vector<int32_t>* hashes) {
    map->clear();
    hashes->clear();
    const int64_t nk = (int64_t)kr.id.size();
    if (nk == 0) return FW_OK;
    int64_t* d_off = nullptr;
    uint8_t* d_bytes = nullptr;
    int rc;
    if ((rc = fd_dalloc(&d_off, kr.off.size()))) return rc;
    if ((rc = fd_dalloc(&d_bytes, std::max<size_t>(kr.img.size() * 8, 8)))) { hipFree(d_off); return rc; }
    FD_TRY(hipMemcpy(d_off, kr.off.data(), kr.off.size() * 8, hipMemcpyHostToDevice));
    FD_TRY(hipMemcpy(d_bytes, kr.img.data(), kr.img.size() * 8, hipMemcpyHostToDevice));
    rc = kr_intern(h, nk, d_off, d_bytes);
    std::vector<int64_t> ids((size_t)nk);
    std::vector<int32_t> hs((size_t)nk);
    if (!rc) {
        FD_TRY(hipMemcpyAsync(ids.data(), h->d_kid, nk * 8, hipMemcpyDeviceToHost, h->stream));
        FD_TRY(hipMemcpyAsync(hs.data(), h->d_khash, nk * 4, hipMemcpyDeviceToHost, h->stream));
        Ctrl c;
        rc = read_ctrl(h, &c);  // syncs; a full table is a device error
    }
    hipFree(d_off);
    hipFree(d_bytes);
    if (rc) return rc;
    std::vector<size_t> order((size_t)nk);
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::make_pair(kr.id[a], ids[a]) < std::make_pair(kr.id[b], ids[b]); });
    for (size_t k : order) {
        map->emplace_back(kr.id[k], ids[k]);
        hashes->push_back(hs[k]);
    }
    return FW_OK;
}

int64_t kr_lookup(const std::vector<std::pair<int64_t, int64_t>>& map, int64_t old, size_t* pos) {
    auto it = std::lower_bound(map.begin(), map.end(), std::make_pair(old, INT64_MIN));
    if (it == map.end() || it->first != old) return -1;
    *pos = (size_t)(it - map.begin());
    return it->second;
}

// adds a key group's state to the handle's (s passed kg_decode, or comes from a converter)
int kg_install(fw_handle* h, const KgState& s) {
    const KeySpace& ks = h->ks;
    const int pwe = h->pwe, L = ks.sb_per_kg_log2;
    const int li = s.key_group - ks.kg_start;
    if (ks.hash_kind == KH_PRE && !h->keyrow && L > s.sb_log2)
        return set_error(FW_E_INVALID, "precomputed-hash keys cannot be split finer than the snapshot's sub-buckets");
    const int nsub = 1 << L;
    std::vector<int32_t> cnt(nsub);
    FD_TRY(hipStreamSynchronize(h->stream));
    FD_TRY(hipMemcpy(cnt.data(), h->state_count + ((size_t)li << L), sizeof(int32_t) * nsub, hipMemcpyDeviceToHost));
    for (int q = 0; q < nsub; q++)
        if (cnt[q] != 0)  // restored twice, or restored after records of this key group arrived
            return set_error(FW_E_STATE, "key group %d already holds state in this subtask", s.key_group);
    // key rows: this handle's ids, and the hash that routes each (BinaryRowData.hashCode)
    std::vector<std::pair<int64_t, int64_t>> map;
    std::vector<int32_t> hashes;
    int rc;
    if (h->keyrow && (rc = kr_install(h, s.kr, &map, &hashes))) return rc;
    // target superbucket of every entry
    std::vector<std::vector<uint64_t>> per(nsub);
    for (size_t i = 0; i < s.ent.size(); i += (size_t)pwe) {
        const uint64_t* e = s.ent.data() + i;
        int64_t key = (int64_t)e[0];
        int sb;
        if (h->keyrow) {
            size_t pos = 0;
            key = kr_lookup(map, key, &pos);
            if (key < 0) return set_error(FW_E_INVALID, "key-group snapshot entry without its key row");
            uint32_t m;
            sb = route_key(ks, key, hashes[pos], &m);
            if ((sb >> L) != li) return set_error(FW_E_INVALID, "entry key does not belong to key group %d", s.key_group);
        } else if (ks.hash_kind == KH_PRE) {
            sb = (li << L) + (int)((e[2] >> 32) & (uint64_t)(nsub - 1));
        } else {
            uint32_t m;
            sb = route_key(ks, key, 0, &m);
            if ((sb >> L) != li) return set_error(FW_E_INVALID, "entry key does not belong to key group %d", s.key_group);
        }
        auto& v = per[sb - (li << L)];
        v.insert(v.end(), e, e + pwe);
        v[v.size() - pwe] = (uint64_t)key;
        v[v.size() - pwe + 2] = (uint32_t)e[2];  // flags without the source sub-bucket
    }
    std::vector<int64_t> mins(nsub);
    FD_TRY(hipMemcpy(mins.data(), h->sb_min_timer + ((size_t)li << L), sizeof(int64_t) * nsub, hipMemcpyDeviceToHost));
    for (int q = 0; q < nsub; q++)
        if (cnt[q] + (int64_t)(per[q].size() / pwe) > h->cap_e)
            return set_error(FW_E_CAPACITY, "restored key group %d exceeds the state table (%lld entries per superbucket)",
                             s.key_group, (long long)h->cap_e);
    int64_t added = 0;
    for (int q = 0; q < nsub; q++) {
        const int64_t n = (int64_t)(per[q].size() / pwe);
        if (!n) continue;
        const size_t sb = ((size_t)li << L) + q;
        FD_TRY(hipMemcpy(h->state + (sb * h->cap_e + cnt[q]) * pwe, per[q].data(), (size_t)n * pwe * 8,
                         hipMemcpyHostToDevice));
        FD_TRY(hipMemset(h->sb_nar + sb, 0, 1));  // (the superbucket held no entries: cnt[q] == 0)
        for (int64_t i = 0; i < n; i++)
            mins[q] = std::min(mins[q], entry_timer_end(h, (int64_t)per[q][(size_t)i * pwe + 1], per[q][(size_t)i * pwe + 2]));
        cnt[q] += (int32_t)n;
        added += n;
    }
    FD_TRY(hipMemcpy(h->state_count + ((size_t)li << L), cnt.data(), sizeof(int32_t) * nsub, hipMemcpyHostToDevice));
    FD_TRY(hipMemcpy(h->sb_min_timer + ((size_t)li << L), mins.data(), sizeof(int64_t) * nsub, hipMemcpyHostToDevice));
    Ctrl c;
    if ((rc = read_ctrl(h, &c))) return rc;
    c.live_entries += added;
    c.ntp = INT64_MIN;  // next trigger recomputed at the next advance
    h->dev_ntp = INT64_MIN;
    FD_TRY(hipMemcpy(h->ctrl, &c, sizeof c, hipMemcpyHostToDevice));
    h->push_seq = std::max<int64_t>(h->push_seq, s.push_seq);
    h->reset_pending = true;  // as snap_install: uncollected rows of before the restore are dropped
    return FW_OK;
}

// replaces the handle's state by s (which passed snap_decode); s's entries take this handle's key ids
int snap_install(fw_handle* h, SnapState& s) {
    const int nsb = h->ks.n_sb, pwe = h->pwe;
    std::vector<uint64_t>& ent = s.ent;
    int rc;
    if (h->keyrow) {  // this handle's ids for the blob's key rows
        // Everything that holds an id of before the restore goes with it (state, pending pushes, timer
        // requests, uncollected rows): the table starts empty.  A handle whose table was full restores
        // like a fresh one, and a device error of before the restore does not fail the interning.
        FD_TRY(hipStreamSynchronize(h->stream));
        Ctrl k;
        FD_TRY(hipMemcpy(&k, h->ctrl, sizeof k, hipMemcpyDeviceToHost));
        k.kr_next_id = k.kr_free_count = k.kr_free_cursor = 0;
        k.error = 0;
        FD_TRY(hipMemcpy(h->ctrl, &k, sizeof k, hipMemcpyHostToDevice));
        FD_TRY(hipMemsetAsync(h->kr.slots, 0, sizeof(uint32_t) * h->kr.n_slots, h->stream));
        std::vector<std::pair<int64_t, int64_t>> map;
        std::vector<int32_t> hashes;
        if ((rc = kr_install(h, s.kr, &map, &hashes))) return rc;
        for (size_t i = 0; i < ent.size(); i += (size_t)pwe) {
            size_t pos;
            const int64_t id = kr_lookup(map, (int64_t)ent[i], &pos);
            if (id < 0) return set_error(FW_E_INVALID, "snapshot entry without its key row");
            ent[i] = (uint64_t)id;
        }
    }
    FD_TRY(hipStreamSynchronize(h->stream));
    std::vector<int64_t> mins(nsb, INT64_MAX);
    const uint64_t* e = ent.data();
    for (int sb = 0; sb < nsb; sb++) {
        const int32_t n = s.cnt[sb];
        if (!n) continue;
        for (int i = 0; i < n; i++)
            mins[sb] = std::min(mins[sb], entry_timer_end(h, (int64_t)e[(size_t)i * pwe + 1], e[(size_t)i * pwe + 2]));
        FD_TRY(hipMemcpy(h->state + (size_t)sb * h->cap_e * pwe, e, (size_t)n * pwe * 8, hipMemcpyHostToDevice));
        e += (size_t)n * pwe;
    }
    FD_TRY(hipMemcpy(h->state_count, s.cnt.data(), 4ll * nsb, hipMemcpyHostToDevice));
    FD_TRY(hipMemset(h->sb_nar, 0, (size_t)nsb));  // restored entries are in the wide layout
    FD_TRY(hipMemcpy(h->sb_min_timer, mins.data(), 8ll * nsb, hipMemcpyHostToDevice));
    Ctrl c;
    FD_TRY(hipMemcpy(&c, h->ctrl, sizeof c, hipMemcpyDeviceToHost));  // the key-row allocator survives
    const Ctrl keep = c;
    FD_TRY(launch_init_ctrl(h->ctrl, h->stream));
    h->ig_pushes = 0;  // Ctrl::push_count starts over: so does the host's copy, and the ingest mirror
    h->ig_since_fold = 0;
    h->ig_merges = 0;  // (no PF_PACK fields until a push has measured them and a flush has opened an epoch)
    if (h->ig_mirror) *h->ig_mirror = ~0ull;
    // the restore drops the pending pushes: with runs, their fill counters, overflow flags and formats
    // go too (as allocate() starts them), or the next push would add onto the dropped push's fills and
    // the next flush would fold its stale rows
    if (h->run_rows) {
        const size_t n_isb = (size_t)(h->ks.n_sb >> h->ks.pass_log2);
        FD_TRY(hipMemsetAsync(h->run_fill, 0, sizeof(uint32_t) * FW_MAX_PENDING * RUN_X * n_isb, h->stream));
        FD_TRY(hipMemsetAsync(h->run_ovf, 0, sizeof(uint32_t) * FW_MAX_PENDING * n_isb, h->stream));
        FD_TRY(hipMemsetAsync(h->slot_fmt, 0, sizeof(int32_t) * FW_MAX_PENDING, h->stream));
    }
    FD_TRY(hipStreamSynchronize(h->stream));
    FD_TRY(hipMemcpy(&c, h->ctrl, sizeof c, hipMemcpyDeviceToHost));
    // SQL: union-list watermark state (WindowAggOperator.initializeState :183-206).  DataStream:
    // the WindowOperator keeps no watermark state, its timer service restarts at Long.MIN_VALUE
    // (InternalTimerServiceImpl.java:72) until the next watermark arrives.
    c.cur = h->cfg.api == FW_API_SQL ? s.cur : INT64_MIN;
    c.ntp = INT64_MIN;
    c.late_dropped = (uint64_t)s.late_dropped;
    c.fired = (uint64_t)s.fired;
    c.live_entries = (int64_t)(ent.size() / (size_t)pwe);
    c.kr_next_id = keep.kr_next_id;
    c.kr_free_count = keep.kr_free_count;
    c.kr_free_cursor = keep.kr_free_cursor;
    c.kr_epoch = keep.kr_epoch;
    c.kr_collections = keep.kr_collections;
    FD_TRY(hipMemcpy(h->ctrl, &c, sizeof c, hipMemcpyHostToDevice));
    h->pushes_ub = 0;
    h->host_cur = c.cur;
    h->dev_cur = c.cur;
    h->dev_ntp = INT64_MIN;
    h->push_seq = std::max<int64_t>(h->push_seq, s.push_seq);
    // rows emitted before the restore and not collected go with the rest (a restored operator starts
    // with none): out_count went with the control block, the next merge launch starts the slabs afresh
    h->reset_pending = true;
    return FW_OK;
}

}  // namespace

extern "C" {

int fw_snapshot(fw_handle* h, void* buf, int64_t capacity, int64_t* size) {
    if (!h || !size) return set_error(FW_E_INVALID, "null argument");
    if (h->cw.on) {
        h->cw.watermark = h->host_cur;
        return cw_snapshot(&h->cw, -1, buf, capacity, size);
    }
    if (h->sw.on) {
        int rc_wm;
        if (h->sw.wm_dev && (rc_wm = sw_read_watermark(&h->sw, &h->host_cur))) return rc_wm;
        return sw_snapshot(&h->sw, h->host_cur, -1, buf, capacity, size);
    }
    SnapState s;
    if (const int rc = snap_collect(h, &s)) return rc;
    return snap_encode(layout_of(h), s, buf, capacity, size);
}

int fw_restore(fw_handle* h, const void* buf, int64_t size) {
    if (!h || !buf) return set_error(FW_E_INVALID, "null argument");
    if (h->cw.on) {
        const int rc = cw_restore(&h->cw, false, buf, size);
        if (!rc) h->host_cur = h->cw.watermark;
        return rc;
    }
    if (h->sw.on) return sw_restore(&h->sw, false, buf, size, &h->host_cur);
    SnapState s;  // the blob is checked before the handle changes: a blob that fails here leaves it as it was
    if (const int rc = snap_decode(layout_of(h), buf, size, &s)) return rc;
    return snap_install(h, s);
}

int fw_snapshot_key_group(fw_handle* h, int32_t key_group, void* buf, int64_t capacity, int64_t* size) {
    if (!h || !size) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE_RECORD(h, "fw_snapshot_key_group");
    if (h->cw.on) {
        if (key_group < 0) return set_error(FW_E_INVALID, "key group %d is not owned by this subtask", key_group);
        h->cw.watermark = h->host_cur;
        return cw_snapshot(&h->cw, key_group, buf, capacity, size);
    }
    if (h->sw.on) {
        if (key_group < 0) return set_error(FW_E_INVALID, "key group %d is not owned by this subtask", key_group);
        int rc_wm;
        if (h->sw.wm_dev && (rc_wm = sw_read_watermark(&h->sw, &h->host_cur))) return rc_wm;
        return sw_snapshot(&h->sw, h->host_cur, key_group, buf, capacity, size);
    }
    const CkLayout L = layout_of(h);
    KgState s;
    int rc;
    if ((rc = ck_owned(L, key_group)) || (rc = kg_collect(h, key_group, &s))) return rc;
    return kg_encode(L, s, buf, capacity, size);
}

int fw_restore_key_group(fw_handle* h, const void* buf, int64_t size) {
    if (!h || !buf) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE_RECORD(h, "fw_restore_key_group");
    if (h->cw.on) return cw_restore(&h->cw, true, buf, size);
    if (h->sw.on) {
        // (lateness: the blob's watermark must be the handle's, which is Ctrl::cur once advanced from the device)
        int rc_wm = 0;
        if (h->sw.late && h->sw.wm_dev && (rc_wm = sw_read_watermark(&h->sw, &h->host_cur))) return rc_wm;
        return sw_restore(&h->sw, true, buf, size, &h->host_cur);
    }
    KgState s;
    if (const int rc = kg_decode(layout_of(h), buf, size, &s)) return rc;
    return kg_install(h, s);
}

int fw_snapshot_key_group_heap(fw_handle* h, int32_t key_group, const fw_heap_state_ids* ids, void* buf,
                               int64_t capacity, int64_t* size) {
    if (!h || !size) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_snapshot_key_group_heap");
    const CkPlan p = plan_of(h);
    KgState s;
    int rc;
    if ((rc = heap_check(p, ids)) || (rc = ck_owned(layout_of(h), key_group)) || (rc = kg_collect(h, key_group, &s))) return rc;
    std::vector<uint8_t> bytes;
    heap_encode(p, ids, s, &bytes);
    return ck_emit({{bytes.data(), bytes.size()}}, buf, capacity, size);
}

int fw_restore_key_group_heap(fw_handle* h, const void* buf, int64_t size, const fw_heap_state_ids* ids) {
    if (!h || !buf || size < 0) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_restore_key_group_heap");
    const CkPlan p = plan_of(h);
    KgState s;
    Ctrl c;
    int rc;
    if ((rc = heap_check(p, ids)) || (rc = heap_decode(p, ids, buf, size, &s)) || (rc = read_ctrl(h, &c)) ||
        (rc = ck_owned(layout_of(h), s.key_group)))
        return rc;
    s.push_seq = (int64_t)h->push_seq;
    return kg_install(h, s);
}

int fw_ds_snapshot_key_group(fw_handle* h, int32_t key_group, fw_ds_window* out, int64_t capacity, int64_t* n) {
    if (!h || !n) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_ds_snapshot_key_group");
    const CkPlan p = plan_of(h);
    KgState s;
    int rc;
    if ((rc = ds_state_check(p)) || (rc = ck_owned(layout_of(h), key_group)) || (rc = kg_collect(h, key_group, &s))) return rc;  // flushes
    return ds_encode(p, s, out, capacity, n);
}

int fw_ds_restore_key_group(fw_handle* h, int32_t key_group, const fw_ds_window* in, int64_t n, int64_t next_push_seq) {
    if (!h || (n > 0 && !in) || n < 0) return set_error(FW_E_INVALID, "null argument");
    CW_REFUSE(h, "fw_ds_restore_key_group");
    const CkPlan p = plan_of(h);
    KgState s;
    Ctrl c;
    int rc;
    if ((rc = ds_state_check(p)) || (rc = ck_owned(layout_of(h), key_group)) || (rc = ds_decode(p, key_group, in, n, next_push_seq, &s)) ||
        (rc = read_ctrl(h, &c)))
        return rc;
    return kg_install(h, s);
}

}  // extern "C"
