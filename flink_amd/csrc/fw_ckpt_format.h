// fw_ckpt_format.h -- the time-window path's checkpoint formats, on the host alone: no HIP call and
// no handle, so the readers of the one artefact that outlives a process run under a sanitizer without
// a device (ckpt_san_driver.hip).
//
// A checkpoint moves in three steps (fw_checkpoint.hip): collect gathers a handle's state into the
// in-memory form (KgState: one key group, SnapState: the whole handle), a codec of this header turns
// that form into bytes or back, and install puts a decoded state into a handle.  Four formats:
//   the whole-handle blob      snap_encode / snap_decode
//   the key-group blob         kg_encode / kg_decode
//   the heap backend's bytes   heap_encode / heap_decode   (one key group)
//   the DataStream window list ds_encode / ds_decode       (one key group)
// A decoder checks its input against the restoring operator's CkLayout and fills its output only when
// every check has passed: whatever needs no device is refused here, before the handle changes.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

#include "fw_folded.h"

namespace fw {

// The integers a blob is checked against, and the ones its header repeats.
struct CkLayout {
    int32_t n_sb, cap_e, pwe, nw, nw_t, sb_per_kg_log2;
    int32_t kg_start, n_kg;
    int32_t hash_kind;  // fw_config.key_hash
    bool keyrow;
    int64_t kr_cap_ids;
    int32_t kr_max_len;
    int64_t win_size, win_interval;
    uint64_t semantics;  // the fingerprint of everything that gives the stored words their meaning
};

// ---- key rows in a blob (FW_KEYHASH_KEYROW): the entries carry table ids, which mean nothing to
// another handle, so a blob also holds the key row of every id its entries use:
//   [n_keys] then per key [id, hash << 32 | length, image words...]  (uint64 words)
// and a restore interns the images into its own table and rewrites the entries' keys.
struct KeyRows {
    std::vector<int64_t> id;         // the writer's table ids
    std::vector<uint32_t> hash;      // their hashCodes
    std::vector<int64_t> off{0};     // image k is bytes [off[k], off[k + 1]) of img
    std::vector<uint64_t> img;
    void add(int64_t key_id, uint32_t hash_code, const void* image, int64_t len) {
        id.push_back(key_id);
        hash.push_back(hash_code);
        img.resize(img.size() + (size_t)len / 8);
        if (len) memcpy(img.data() + off.back() / 8, image, (size_t)len);
        off.push_back(off.back() + len);
    }
};

// one key group's state
struct KgState {
    int32_t key_group = 0;
    int32_t sb_log2 = 0;  // the writer's sub-buckets per key group (log2)
    int64_t cur = INT64_MIN, push_seq = 0;
    std::vector<uint64_t> ent;  // pwe words per entry; the source sub-bucket in the high half of the flags word
    KeyRows kr;
};

// the whole handle's state
struct SnapState {
    int64_t cur = INT64_MIN, late_dropped = 0, fired = 0, push_seq = 0;
    std::vector<int32_t> cnt;   // entries per superbucket
    std::vector<uint64_t> ent;  // superbucket 0's entries, superbucket 1's, ...
    KeyRows kr;
};

// ---- snapshot: [header][state_count[n_sb]][entries of sb 0][entries of sb 1]... [key rows]
struct SnapHeader {
    uint64_t magic;
    int32_t version, n_sb, cap_e, pwe;
    int64_t cur, late_dropped, fired, live;
    uint64_t semantics;
    int64_t push_seq;  // arrival ordinals continue after the restore (W_FIRST words stay ordered)
};
static const uint64_t SNAP_MAGIC = 0x464c4b57494e3033ull;  // "FLKWIN03"

// ---- key-group-partitioned checkpoint (rescaling): [header][entries][key rows] ---------
// The heap backend writes keyed state per key group (HeapSnapshotStrategy.java:97 ->
// AbstractStateTableSnapshot.writeStateInKeyGroup :112) and a rescaled job hands every new
// subtask the key groups of its computeKeyGroupRangeForOperatorIndex range.  The blob of one key
// group is therefore independent of this build's superbucket split: entries carry the sub-bucket
// they came from, and a restoring handle re-routes every key with the same route_key the
// ingest kernel runs (only a precomputed-hash key cannot be re-hashed; it keeps its sub-bucket
// bits, which works for any target split not finer than the source's).
struct KgHeader {
    uint64_t magic;
    int32_t version, key_group, pwe, nw, sb_log2, hash_kind;
    int64_t win_size, win_interval, cur, n;
    uint64_t semantics;
    int64_t push_seq;  // arrival ordinals of the restoring handle continue after every restored blob's
};
static const uint64_t KG_MAGIC = 0x464c4b574b473033ull;  // "FLKWKG03"
constexpr int32_t CK_VERSION = 3;

// accumulator words holding no row: the identities of the planned words, 0 in the layout's padding
inline void acc_identity(const WordDesc& wd, int nw_t, uint64_t* out) {
    for (int w = 0; w < nw_t; w++) out[w] = w < wd.nw ? word_identity(wd.op[w]) : 0;
}

inline int ck_owned(const CkLayout& L, int32_t key_group) {
    if (key_group < L.kg_start || key_group >= L.kg_start + L.n_kg)
        return set_error(FW_E_INVALID, "key group %d is not owned by this subtask", key_group);
    return FW_OK;
}

// The tail of every export: *size = the bytes of the pieces; without a buffer that is all (the size
// query), else the pieces are copied out if they fit.
struct CkPiece {
    const void* p;
    size_t n;
};
inline int ck_emit(std::initializer_list<CkPiece> pieces, void* buf, int64_t capacity, int64_t* size) {
    int64_t need = 0;
    for (const CkPiece& q : pieces) need += (int64_t)q.n;
    *size = need;
    if (!buf) return FW_OK;
    if (capacity < need) return set_error(FW_E_INVALID, "snapshot buffer too small (%lld < %lld)", (long long)capacity, (long long)need);
    char* at = (char*)buf;
    for (const CkPiece& q : pieces) {
        if (q.n) memcpy(at, q.p, q.n);
        at += q.n;
    }
    return FW_OK;
}

inline void kr_encode(const KeyRows& kr, std::vector<uint64_t>* sec) {
    sec->assign(1, (uint64_t)kr.id.size());
    for (size_t k = 0; k < kr.id.size(); k++) {
        const int64_t len = kr.off[k + 1] - kr.off[k];
        sec->push_back((uint64_t)kr.id[k]);
        sec->push_back((uint64_t)kr.hash[k] << 32 | (uint64_t)len);
        sec->insert(sec->end(), kr.img.begin() + kr.off[k] / 8, kr.img.begin() + kr.off[k + 1] / 8);
    }
}

// a blob's key-row section: the ids it names, their hashes and images
inline int kr_parse(const uint64_t* sec, int64_t avail_words, KeyRows* out) {
    *out = KeyRows{};
    if (avail_words < 1) return set_error(FW_E_INVALID, "key-row section truncated");
    const int64_t nk = (int64_t)sec[0];
    int64_t p = 1;
    for (int64_t k = 0; k < nk; k++) {
        if (p + 2 > avail_words) return set_error(FW_E_INVALID, "key-row section truncated");
        const int64_t len = (int64_t)(uint32_t)sec[p + 1];
        if ((len & 7) || p + 2 + len / 8 > avail_words) return set_error(FW_E_INVALID, "key-row section truncated");
        out->add((int64_t)sec[p], (uint32_t)(sec[p + 1] >> 32), sec + p + 2, len);
        p += 2 + len / 8;
    }
    return FW_OK;
}

// The key-row section behind a blob's entries, checked against the restoring table: whole words, no
// more rows than the table holds, every length one the table takes, and a row for every entry's key.
// `what` names the blob in the messages.
inline int kr_decode(const CkLayout& L, const char* what, const char* sec_bytes, int64_t n_bytes, const std::vector<uint64_t>& ent,
                     KeyRows* out) {
    if (n_bytes & 7) return set_error(FW_E_INVALID, "key-row section is not whole words (%lld bytes)", (long long)n_bytes);
    std::vector<uint64_t> sec((size_t)(n_bytes / 8));
    if (n_bytes) memcpy(sec.data(), sec_bytes, (size_t)n_bytes);
    if (const int rc = kr_parse(sec.data(), (int64_t)sec.size(), out)) return rc;
    if ((int64_t)out->id.size() > L.kr_cap_ids)
        return set_error(FW_E_CAPACITY, "%s holds %lld key rows, the table %lld", what, (long long)out->id.size(), (long long)L.kr_cap_ids);
    for (size_t k = 0; k + 1 < out->off.size(); k++)
        if (out->off[k + 1] - out->off[k] < 8 || out->off[k + 1] - out->off[k] > L.kr_max_len)
            return set_error(FW_E_INVALID, "%s key row of %lld bytes (key_row_max_bytes %d)", what, (long long)(out->off[k + 1] - out->off[k]),
                             (int)L.kr_max_len);
    std::vector<int64_t> ids = out->id;
    std::sort(ids.begin(), ids.end());
    for (size_t i = 0; i < ent.size(); i += (size_t)L.pwe)
        if (!std::binary_search(ids.begin(), ids.end(), (int64_t)ent[i])) return set_error(FW_E_INVALID, "%s entry without its key row", what);
    return FW_OK;
}

// ---- the key-group blob
inline int kg_encode(const CkLayout& L, const KgState& s, void* buf, int64_t capacity, int64_t* size) {
    const KgHeader hd{KG_MAGIC,     CK_VERSION,     s.key_group, L.pwe,
                      L.nw,         s.sb_log2,      L.hash_kind, L.win_size,
                      L.win_interval, s.cur,        (int64_t)(s.ent.size() / (size_t)L.pwe), L.semantics,
                      s.push_seq};
    std::vector<uint64_t> krs;
    if (L.keyrow) kr_encode(s.kr, &krs);
    return ck_emit({{&hd, sizeof hd}, {s.ent.data(), s.ent.size() * 8}, {krs.data(), krs.size() * 8}}, buf, capacity, size);
}

// *out = the blob's key group, of the operator L describes and owned by its subtask; *out is left as
// it was when the blob is refused
inline int kg_decode(const CkLayout& L, const void* buf, int64_t size, KgState* out) {
    KgHeader hd;
    if (size < (int64_t)sizeof hd) return set_error(FW_E_INVALID, "key-group snapshot truncated");
    memcpy(&hd, buf, sizeof hd);
    if (hd.magic != KG_MAGIC || hd.version != CK_VERSION) return set_error(FW_E_INVALID, "not a key-group snapshot");
    if (hd.pwe != L.pwe || hd.nw != L.nw || hd.hash_kind != L.hash_kind || hd.win_size != L.win_size ||
        hd.win_interval != L.win_interval || hd.semantics != L.semantics)
        return set_error(FW_E_INVALID, "key-group snapshot of a different operator configuration");
    if (hd.n < 0) return set_error(FW_E_INVALID, "key-group snapshot with %lld entries", (long long)hd.n);
    const int64_t ent_bytes = (int64_t)L.pwe * 8;
    if (hd.n > (size - (int64_t)sizeof hd) / ent_bytes) return set_error(FW_E_INVALID, "key-group snapshot truncated");
    const int64_t ent_end = (int64_t)sizeof hd + hd.n * ent_bytes;
    if (const int rc = ck_owned(L, hd.key_group)) return rc;
    KgState s;
    s.key_group = hd.key_group;
    s.sb_log2 = hd.sb_log2;
    s.cur = hd.cur;
    s.push_seq = hd.push_seq;
    s.ent.resize((size_t)hd.n * (size_t)L.pwe);
    if (hd.n) memcpy(s.ent.data(), (const char*)buf + sizeof hd, s.ent.size() * 8);
    if (L.keyrow)
        if (const int rc = kr_decode(L, "key-group snapshot", (const char*)buf + ent_end, size - ent_end, s.ent, &s.kr)) return rc;
    *out = std::move(s);
    return FW_OK;
}

// ---- the whole-handle blob
inline int snap_encode(const CkLayout& L, const SnapState& s, void* buf, int64_t capacity, int64_t* size) {
    const SnapHeader hd{SNAP_MAGIC, CK_VERSION,     L.n_sb,  L.cap_e, L.pwe, s.cur, s.late_dropped,
                        s.fired,    (int64_t)(s.ent.size() / (size_t)L.pwe), L.semantics, s.push_seq};
    std::vector<uint64_t> krs;
    if (L.keyrow) kr_encode(s.kr, &krs);
    return ck_emit({{&hd, sizeof hd}, {s.cnt.data(), s.cnt.size() * 4}, {s.ent.data(), s.ent.size() * 8}, {krs.data(), krs.size() * 8}}, buf,
                   capacity, size);
}

// *out = the blob's state, of a handle with L's layout: every count inside the table, the counts
// adding up to the entries; *out is left as it was when the blob is refused
inline int snap_decode(const CkLayout& L, const void* buf, int64_t size, SnapState* out) {
    SnapHeader hd;
    if (size < (int64_t)sizeof hd) return set_error(FW_E_INVALID, "snapshot truncated");
    memcpy(&hd, buf, sizeof hd);
    if (hd.magic != SNAP_MAGIC || hd.version != CK_VERSION || hd.n_sb != L.n_sb || hd.pwe != L.pwe || hd.cap_e != L.cap_e ||
        hd.semantics != L.semantics)
        return set_error(FW_E_INVALID, "snapshot layout does not match this operator configuration");
    if (hd.live < 0) return set_error(FW_E_INVALID, "snapshot with %lld entries", (long long)hd.live);
    const int64_t ent_bytes = (int64_t)L.pwe * 8, cnt_end = (int64_t)sizeof hd + 4ll * L.n_sb;
    if (size < cnt_end || hd.live > (size - cnt_end) / ent_bytes) return set_error(FW_E_INVALID, "snapshot truncated");
    const int64_t ent_end = cnt_end + hd.live * ent_bytes;
    SnapState s;
    s.cur = hd.cur;
    s.late_dropped = hd.late_dropped;
    s.fired = hd.fired;
    s.push_seq = hd.push_seq;
    s.cnt.resize((size_t)L.n_sb);
    memcpy(s.cnt.data(), (const char*)buf + sizeof hd, 4 * s.cnt.size());
    int64_t total = 0;
    for (int32_t c : s.cnt) {
        if (c < 0 || c > L.cap_e) return set_error(FW_E_INVALID, "snapshot superbucket of %d entries (the table holds %d)", c, L.cap_e);
        total += c;
    }
    if (total != hd.live)
        return set_error(FW_E_INVALID, "snapshot superbuckets hold %lld entries, its header says %lld", (long long)total, (long long)hd.live);
    s.ent.resize((size_t)hd.live * (size_t)L.pwe);
    if (hd.live) memcpy(s.ent.data(), (const char*)buf + cnt_end, s.ent.size() * 8);
    if (L.keyrow)
        if (const int rc = kr_decode(L, "snapshot", (const char*)buf + ent_end, size - ent_end, s.ent, &s.kr)) return rc;
    *out = std::move(s);
    return FW_OK;
}

// ---- what the heap and DataStream converters need of an operator's plan
struct CkPlan {
    const fw_config& cfg;
    const WinDesc& win;
    const WordDesc& wd;
    const AggDesc& ad;
    const KeySpace& ks;
    int nw_t, pwe;
    bool keyrow;
};

// ---- heap keyed-state backend key-group format ------------------------------------------
// The bytes the heap backend writes for one key group of a window-aggregate operator
// (HeapSnapshotStrategy.java:161-172): writeInt(keyGroup), then per registered state
// writeShort(stateId) and that state's key-group writer --
//   window-aggs ValueState (CopyOnWriteStateMapSnapshot.writeState :127-149):
//       writeInt(n), then per entry namespace (LongSerializer: 8 B big-endian sliceEnd),
//       key (BinaryRowData: writeInt(len) + bytes), accumulator (RowDataSerializer -> BinaryRowData)
//   event / processing window-timers queues (KeyGroupPartitioner.java:241-254 with
//       TimerSerializer.serialize :147-152): writeInt(n), then per timer
//       writeLong(flipSignBit(ts)), key, namespace
// The accumulator row holds every aggregate's buffer fields in order (COUNT(*) / COUNT: count
// BIGINT; SUM / MIN / MAX: value of the aggregate's type, NULL-able; AVG: sum BIGINT|DOUBLE, count
// BIGINT), the LOCAL phase's output fields.  A timer's timestamp is
// toEpochMillsForTimer(window - 1) (SlicingWindowTimerServiceImpl.java:43-46).
constexpr int HEAP_MAX_FIELDS = 2 * FW_MAX_AGGS;

struct HeapWriter {
    std::vector<uint8_t> b;
    void u8(uint8_t v) { b.push_back(v); }
    void be32(uint32_t v) { for (int i = 3; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i))); }
    void be16(uint16_t v) { b.push_back((uint8_t)(v >> 8)); b.push_back((uint8_t)v); }
    void be64(uint64_t v) { for (int i = 7; i >= 0; i--) b.push_back((uint8_t)(v >> (8 * i))); }
    void bytes(const uint8_t* p, size_t n) { b.insert(b.end(), p, p + n); }
};

struct HeapReader {
    const uint8_t* p;
    size_t n, at = 0;
    bool bad = false;
    bool need(size_t k) { if (at + k > n) bad = true; return !bad; }
    uint32_t be32() { if (!need(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; i++) v = v << 8 | p[at++]; return v; }
    uint16_t be16() { if (!need(2)) return 0; uint16_t v = (uint16_t)(p[at] << 8 | p[at + 1]); at += 2; return v; }
    uint64_t be64() { if (!need(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; i++) v = v << 8 | p[at++]; return v; }
    const uint8_t* take(size_t k) { if (!need(k)) return nullptr; const uint8_t* q = p + at; at += k; return q; }
};

// the accumulator row's field types (FW_T_*), in order
inline int heap_fields(const AggDesc& ad, int32_t* type) {
    int j = 0;
    for (int g = 0; g < ad.n; g++) {
        const int k = ad.kind[g], t = ad.type[g];
        if (k == FW_AGG_COUNT_STAR || k == FW_AGG_COUNT) type[j++] = FW_T_I64;
        else if (k == FW_AGG_AVG) { type[j++] = t == FW_T_F64 ? FW_T_F64 : FW_T_I64; type[j++] = FW_T_I64; }
        else type[j++] = t;
    }
    return j;
}

inline int heap_bitset_bytes(int arity) { return ((arity + 63 + 8) / 64) * 8; }  // BinaryRowData.calculateBitSetWidthInBytes

// accumulator words -> buffer field values + NULL mask (emit_partial, restated on the host)
inline void heap_words_to_fields(const AggDesc& ad, const uint64_t* acc, uint64_t* v, uint32_t* nm) {
    *nm = 0;
    int j = 0;
    for (int g = 0; g < ad.n; g++) {
        const int kind = ad.kind[g], type = ad.type[g];
        const uint64_t w0 = acc[ad.w0[g]];
        const bool no_rows = ad.nn[g] >= 0 && acc[ad.nn[g]] == 0;
        uint64_t x = w0;
        bool isnull = false;
        if (kind == FW_AGG_SUM) {
            x = type == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)w0 : w0;
            isnull = no_rows;
        } else if (kind == FW_AGG_MIN || kind == FW_AGG_MAX) {
            if (ad.qf[g] >= 0) {  // q_result (fw_kernel_common.h)
                const uint64_t f = acc[ad.qf[g]];
                isnull = f == Q_EMPTY;
                if (isnull) x = 0;
                else if ((uint32_t)f) x = (f << 32) | (acc[ad.qn[g]] & 0xFFFFFFFFull);
                else if ((int64_t)w0 != 0) x = dkey_inv((int64_t)w0);
                else x = acc[ad.qz[g]] != Q_EMPTY ? ((acc[ad.qz[g]] & 1ull) << 63) : 0ull;
            } else {
                x = type == FW_T_F64 ? dkey_inv((int64_t)w0) : w0;
                isnull = no_rows;
            }
        } else if (kind == FW_AGG_AVG) {
            v[j++] = w0;
            x = acc[ad.w1[g]];
        }
        if (isnull) *nm |= 1u << j;
        v[j++] = isnull ? 0ull : x;
    }
}

// buffer field values -> accumulator words (the inverse; a hidden non-NULL count word becomes 1,
// its only observable property being != 0, and a MIN/MAX(DOUBLE) group is one element of ordinal 0)
inline void heap_fields_to_words(const CkPlan& p, const uint64_t* v, uint32_t nm, uint64_t* acc) {
    const AggDesc& ad = p.ad;
    acc_identity(p.wd, p.nw_t, acc);
    bool set[MAX_WORDS] = {};
    int j = 0;
    for (int g = 0; g < ad.n; g++) {
        const int kind = ad.kind[g], type = ad.type[g];
        const int w0 = ad.w0[g];
        if (kind == FW_AGG_COUNT_STAR || kind == FW_AGG_COUNT) {
            acc[w0] = v[j++];
            set[w0] = true;
            continue;
        }
        if (kind == FW_AGG_AVG) {
            acc[w0] = v[j++];
            acc[ad.w1[g]] = v[j++];
            set[w0] = set[ad.w1[g]] = true;
            continue;
        }
        const bool isnull = (nm >> j) & 1u;
        const uint64_t x = v[j++];
        if (isnull) continue;  // identity words
        if (ad.qf[g] >= 0) {  // merge_q_groups' re-encoding
            const bool nan = f64_isnan(x);
            acc[ad.qf[g]] = nan ? (x >> 32) : 0ull;
            if (nan) acc[ad.qn[g]] = x & 0xFFFFFFFFull;
            if (f64_iszero(x)) acc[ad.qz[g]] = x >> 63;
            if (!nan) acc[w0] = f64_iszero(x) ? 0ull : (uint64_t)dkey(x);
            continue;
        }
        if ((kind == FW_AGG_MIN || kind == FW_AGG_MAX) && type == FW_T_F64) acc[w0] = (uint64_t)dkey(x);
        else if (type == FW_T_I32) acc[w0] = (uint64_t)(int64_t)(int32_t)(uint32_t)x;
        else acc[w0] = x;
        set[w0] = true;
    }
    for (int g = 0; g < ad.n; g++) {  // hidden non-NULL counts of SUM / MIN / MAX
        const int nn = ad.nn[g];
        if (nn < 0 || set[nn]) continue;
        int jj = 0;  // field index of aggregate g
        for (int q = 0; q < g; q++) jj += ad.kind[q] == FW_AGG_AVG ? 2 : 1;
        if (!((nm >> jj) & 1u)) acc[nn] = 1;
    }
}

inline void heap_write_row(HeapWriter& w, const AggDesc& ad, const uint64_t* v, uint32_t nm) {
    int32_t type[HEAP_MAX_FIELDS];
    const int n = heap_fields(ad, type);
    const int bs = heap_bitset_bytes(n);
    w.be32((uint32_t)(bs + 8 * n));
    std::vector<uint8_t> row((size_t)(bs + 8 * n), 0);  // header byte 0 = RowKind.INSERT
    for (int j = 0; j < n; j++) {
        if ((nm >> j) & 1u) {
            row[(size_t)(j + 8) / 8] |= (uint8_t)(1u << ((j + 8) % 8));
            continue;
        }
        const uint64_t x = type[j] == FW_T_I32 ? (uint32_t)v[j] : v[j];
        memcpy(row.data() + bs + 8 * j, &x, 8);  // little-endian slot; an INT in its low 4 bytes
    }
    w.bytes(row.data(), row.size());
}

inline bool heap_read_row(HeapReader& r, const AggDesc& ad, uint64_t* v, uint32_t* nm) {
    int32_t type[HEAP_MAX_FIELDS];
    const int n = heap_fields(ad, type);
    const int bs = heap_bitset_bytes(n);
    const uint32_t len = r.be32();
    if (r.bad || len != (uint32_t)(bs + 8 * n)) return false;
    const uint8_t* p = r.take(len);
    if (!p) return false;
    *nm = 0;
    for (int j = 0; j < n; j++) {
        if ((p[(j + 8) / 8] >> ((j + 8) % 8)) & 1u) { *nm |= 1u << j; v[j] = 0; continue; }
        uint64_t x;
        memcpy(&x, p + bs + 8 * j, 8);
        v[j] = type[j] == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)x : x;
    }
    return true;
}

// the key's BinaryRowData image: BINROW_BIGINT / BINROW_INT keys are the one-field row the key
// projection writes (8 B header, the value slot); key rows carry their interned image
inline int heap_key_kind(const CkPlan& p) {
    if (p.keyrow) return FW_KEYHASH_KEYROW;
    const int k = p.cfg.key_hash;
    return k == FW_KEYHASH_BINROW_BIGINT || k == FW_KEYHASH_BINROW_INT ? k : -1;
}

inline int heap_check(const CkPlan& p, const fw_heap_state_ids* ids) {
    if (!ids) return set_error(FW_E_INVALID, "null state ids");
    if (p.cfg.api != FW_API_SQL || p.cfg.agg_phase == FW_PHASE_LOCAL)
        return set_error(FW_E_INVALID, "the heap key-group format is the SQL window-aggregate operator's keyed state");
    if (heap_key_kind(p) < 0)
        return set_error(FW_E_INVALID, "the heap key-group format needs SQL key rows (BINROW_BIGINT, BINROW_INT or KEYROW keys)");
    if (ids->window_state == ids->event_timers || ids->window_state == ids->processing_timers ||
        ids->event_timers == ids->processing_timers)
        return set_error(FW_E_INVALID, "state ids must differ");
    return FW_OK;
}

// one key group's state -> the heap backend's bytes
inline void heap_encode(const CkPlan& p, const fw_heap_state_ids* ids, const KgState& st, std::vector<uint8_t>* out) {
    const int pwe = p.pwe, nw = p.nw_t;
    const int64_t n = (int64_t)(st.ent.size() / (size_t)pwe);
    const uint64_t* ent = st.ent.data();
    // key images
    std::unordered_map<int64_t, std::pair<const uint8_t*, uint32_t>> img;
    for (size_t k = 0; k < st.kr.id.size(); k++)
        img[st.kr.id[k]] = {(const uint8_t*)(st.kr.img.data() + st.kr.off[k] / 8), (uint32_t)(st.kr.off[k + 1] - st.kr.off[k])};
    const int kk = heap_key_kind(p);
    auto write_key = [&](HeapWriter& w, int64_t key) {
        if (kk == FW_KEYHASH_KEYROW) {
            const auto& im = img.at(key);
            w.be32(im.second);
            w.bytes(im.first, im.second);
            return;
        }
        uint8_t row[16] = {};
        const uint64_t x = kk == FW_KEYHASH_BINROW_INT ? (uint32_t)key : (uint64_t)key;
        memcpy(row + 8, &x, 8);
        w.be32(16);
        w.bytes(row, 16);
    };
    struct St { int64_t key, ns; const uint64_t* acc; };
    std::vector<St> states;
    std::vector<std::pair<int64_t, int64_t>> timers;  // (key, window)
    const WinDesc& win = p.win;
    if (win.hopb) {
        // block entries -> one (key, sliceEnd) state per slot with data.  Timers: the reference holds
        // one per unfired slice end with data (AggCombiner.combine step 5) and one at the first
        // unfired window end whose window holds data (the nextTriggerWindow chain, or a late
        // record's registration).  A chain timer at an EMPTY window (its predecessor's only data
        // was in the slice that window expired) is not derivable from the expired state; it fires
        // without output, and is the one timer the export leaves out.
        std::unordered_map<int64_t, std::vector<int64_t>> ends;  // key -> slice ends with data
        for (int64_t i = 0; i < n; i++) {
            const uint64_t* e = ent + (size_t)i * pwe;
            const uint32_t mask = (uint32_t)e[2] >> HB_MASK_SHIFT;
            for (int s = 0; s < HB_R; s++)
                if ((mask >> s) & 1u) {
                    const int64_t se = wadd((int64_t)e[1], (int64_t)(s + 1) * win.interval);
                    states.push_back({(int64_t)e[0], se, e + 3 + s * nw});
                    ends[(int64_t)e[0]].push_back(se);
                }
        }
        for (auto& kv : ends) {
            auto& v = kv.second;
            std::sort(v.begin(), v.end());
            for (int64_t se : v)
                if (!win_fired(win, se, st.cur)) timers.push_back({kv.first, se});
            if (win_fired(win, v.front(), st.cur)) {  // some data slice fired: the chain's next window
                int64_t e1 = v.front();
                while (win_fired(win, e1, st.cur)) e1 = wadd(e1, win.interval);
                const int64_t lo = wsub(e1, win.size);  // window (e1 - size, e1] holds data?
                const bool data = std::any_of(v.begin(), v.end(), [&](int64_t se) { return se > lo && se <= e1; });
                if (data && !std::binary_search(v.begin(), v.end(), e1)) timers.push_back({kv.first, e1});
            }
        }
    } else {
        for (int64_t i = 0; i < n; i++) {
            const uint64_t* e = ent + (size_t)i * pwe;
            if (e[2] & F_ACC) states.push_back({(int64_t)e[0], (int64_t)e[1], e + 3});
            if (e[2] & F_TIMER) timers.push_back({(int64_t)e[0], (int64_t)e[1]});
        }
    }
    std::sort(timers.begin(), timers.end(), [&](const std::pair<int64_t, int64_t>& a, const std::pair<int64_t, int64_t>& b) {
        return a.second != b.second ? a.second < b.second : a.first < b.first;
    });
    HeapWriter w;
    w.be32((uint32_t)st.key_group);
    int16_t sorted[3] = {ids->window_state, ids->event_timers, ids->processing_timers};
    std::sort(sorted, sorted + 3);
    for (int16_t sid : sorted) {
        w.be16((uint16_t)sid);
        if (sid == ids->window_state) {
            w.be32((uint32_t)states.size());
            uint64_t v[HEAP_MAX_FIELDS];
            uint32_t nm;
            for (const St& s : states) {
                w.be64((uint64_t)s.ns);
                write_key(w, s.key);
                heap_words_to_fields(p.ad, s.acc, v, &nm);
                heap_write_row(w, p.ad, v, nm);
            }
        } else if (sid == ids->event_timers) {
            w.be32((uint32_t)timers.size());
            for (const auto& t : timers) {
                const int64_t ts = tz_epoch_for_timer(win.tz, wsub(t.second, 1));
                w.be64((uint64_t)ts ^ (1ull << 63));  // MathUtils.flipSignBit
                write_key(w, t.first);
                w.be64((uint64_t)t.second);
            }
        } else {
            w.be32(0);  // event-time operator: no processing-time timers
        }
    }
    *out = std::move(w.b);
}

// the heap backend's bytes -> one key group's state (key rows numbered in order of appearance)
inline int heap_decode(const CkPlan& p, const fw_heap_state_ids* ids, const void* buf, int64_t size, KgState* out) {
    HeapReader r{(const uint8_t*)buf, (size_t)size};
    const int32_t kg = (int32_t)r.be32();
    const int kk = heap_key_kind(p);
    // keys: BIGINT / INT values, or key-row images numbered in order of appearance
    KeyRows images;
    std::map<std::vector<uint8_t>, int64_t> image_id;
    auto read_key = [&](int64_t* key) -> bool {
        const uint32_t len = r.be32();
        if (r.bad || len > (1u << 24)) return false;
        const uint8_t* q = r.take(len);
        if (!q) return false;
        if (kk == FW_KEYHASH_KEYROW) {
            if (len % 8) return false;
            std::vector<uint8_t> im(q, q + len);
            auto it = image_id.find(im);
            if (it == image_id.end()) {
                it = image_id.emplace(im, (int64_t)images.id.size()).first;
                images.add(it->second, 0, q, len);
            }
            *key = it->second;
            return true;
        }
        if (len != 16) return false;
        for (int i = 0; i < 8; i++)
            if (q[i]) return false;  // RowKind INSERT, key field not NULL
        uint64_t x;
        memcpy(&x, q + 8, 8);
        *key = kk == FW_KEYHASH_BINROW_INT ? (int64_t)(int32_t)(uint32_t)x : (int64_t)x;
        return kk == FW_KEYHASH_BINROW_BIGINT || (x >> 32) == 0;
    };
    struct Acc { uint64_t v[HEAP_MAX_FIELDS]; uint32_t nm; };
    std::map<std::pair<int64_t, int64_t>, std::pair<int, int>> ent;  // (key, ns) -> (state index or -1, timer)
    std::vector<Acc> accs;
    bool seen[3] = {};
    while (!r.bad && r.at < r.n) {
        const int16_t sid = (int16_t)r.be16();
        const uint32_t n = r.be32();
        if (r.bad) break;
        if (sid == ids->window_state && !seen[0]) {
            seen[0] = true;
            for (uint32_t i = 0; i < n && !r.bad; i++) {
                const int64_t ns = (int64_t)r.be64();
                int64_t key;
                Acc a;
                if (!read_key(&key) || !heap_read_row(r, p.ad, a.v, &a.nm)) { r.bad = true; break; }
                auto& slot = ent.emplace(std::make_pair(key, ns), std::make_pair(-1, 0)).first->second;
                if (slot.first >= 0) return set_error(FW_E_INVALID, "duplicate window state (key, namespace) in key group %d", kg);
                slot.first = (int)accs.size();
                accs.push_back(a);
            }
        } else if (sid == ids->event_timers && !seen[1]) {
            seen[1] = true;
            for (uint32_t i = 0; i < n && !r.bad; i++) {
                const int64_t ts = (int64_t)(r.be64() ^ (1ull << 63));
                int64_t key;
                if (!read_key(&key)) { r.bad = true; break; }
                const int64_t ns = (int64_t)r.be64();
                if (ts != tz_epoch_for_timer(p.win.tz, wsub(ns, 1)))
                    return set_error(FW_E_INVALID, "timer %lld of window %lld is not the window's end timer", (long long)ts, (long long)ns);
                ent.emplace(std::make_pair(key, ns), std::make_pair(-1, 0)).first->second.second = 1;
            }
        } else if (sid == ids->processing_timers && !seen[2]) {
            seen[2] = true;
            if (n != 0) return set_error(FW_E_INVALID, "processing-time timers in an event-time window operator");
        } else {
            return set_error(FW_E_INVALID, "unexpected state id %d in key group %d", (int)sid, kg);
        }
    }
    if (r.bad) return set_error(FW_E_INVALID, "heap key-group data truncated or malformed");
    const int pwe = p.pwe, nw = p.nw_t;
    const WinDesc& win = p.win;
    std::vector<uint64_t> words;
    if (win.hopb) {  // (key, sliceEnd) states -> blocks; timers are arithmetic there
        std::map<std::pair<int64_t, int64_t>, size_t> blk;  // (key, block start) -> word offset
        for (const auto& kv : ent) {
            if (kv.second.first < 0) continue;  // a timer without state fires without output
            const int64_t key = kv.first.first, se = kv.first.second;
            const int64_t bs = window_start(wsub(se, 1), win.offset, win.hb_span_div);
            const int slot = (int)((se - bs) / win.interval) - 1;
            if (slot < 0 || slot >= HB_R || wadd(bs, (int64_t)(slot + 1) * win.interval) != se)
                return set_error(FW_E_INVALID, "namespace %lld is not a slice end of this window", (long long)se);
            auto it = blk.find({key, bs});
            if (it == blk.end()) {
                it = blk.emplace(std::make_pair(key, bs), words.size()).first;
                words.resize(words.size() + pwe, 0);
                uint64_t* e = words.data() + it->second;
                e[0] = (uint64_t)key;
                e[1] = (uint64_t)bs;
                for (int s = 0; s < HB_R; s++) acc_identity(p.wd, nw, e + 3 + s * nw);
            }
            uint64_t* e = words.data() + it->second;
            e[2] |= (uint64_t)(1u << slot) << HB_MASK_SHIFT;
            const Acc& a = accs[(size_t)kv.second.first];
            heap_fields_to_words(p, a.v, a.nm, e + 3 + slot * nw);
        }
    } else {
        for (const auto& kv : ent) {
            const size_t at = words.size();
            words.resize(at + pwe, 0);
            uint64_t* e = words.data() + at;
            e[0] = (uint64_t)kv.first.first;
            e[1] = (uint64_t)kv.first.second;
            e[2] = (kv.second.first >= 0 ? F_ACC : 0u) | (kv.second.second ? F_TIMER : 0u);
            if (kv.second.first >= 0) heap_fields_to_words(p, accs[(size_t)kv.second.first].v, accs[(size_t)kv.second.first].nm, e + 3);
            else acc_identity(p.wd, nw, e + 3);
        }
    }
    out->key_group = kg;
    out->sb_log2 = p.ks.sb_per_kg_log2;
    out->ent = std::move(words);
    out->kr = std::move(images);
    return FW_OK;
}

// ---- DataStream WindowOperator key-group state ---------------------------------------------
// A heap-backend savepoint of the DataStream WindowOperator holds, per key group, the
// "window-contents" reducing state (WindowOperatorBuilder.java:81: namespace TimeWindow, value the
// reduced record) and the "window-timers" queues (WindowOperator.java:232).  The value is the user's
// record type -- value1 with the aggregated field set, whose bytes only the operator shim can write
// -- so the heap bytes are assembled there (flink_amd/datastream/heap_state.py); this pair moves
// the device side as one fw_ds_window per (key, window) holding state or a timer.
inline int ds_state_check(const CkPlan& p) {
    if (p.cfg.api != FW_API_DATASTREAM)
        return set_error(FW_E_INVALID, "DataStream key-group windows are the DataStream WindowOperator's state");
    // LONG / INT keys are re-routed from the key itself; precomputed-hash keys (interned String keys)
    // from the hash the shim passes with each restored window (fw_ds_window.key_hash)
    if (p.cfg.key_hash != FW_KEYHASH_LONG && p.cfg.key_hash != FW_KEYHASH_INT && p.cfg.key_hash != FW_KEYHASH_PRECOMPUTED)
        return set_error(FW_E_INVALID, "DataStream key-group windows need LONG, INT or precomputed-hash keys");
    if (p.ad.n != 1) return set_error(FW_E_INVALID, "DataStream key-group windows hold one aggregated field");
    return FW_OK;
}

// the field value of a window from its words (emit_row's DataStream branch, restated on the host)
inline uint64_t ds_value_of(const AggDesc& ad, const uint64_t* acc) {
    const uint64_t w0 = acc[ad.w0[0]];
    switch (ad.kind[0]) {
        case FW_AGG_SUM: return ad.type[0] == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)w0 : w0;
        case FW_AGG_MIN:
        case FW_AGG_MAX:
        case FW_AGG_MINBY:
        case FW_AGG_MAXBY: {
            uint64_t v = ad.type[0] == FW_T_F64 ? dkey_inv((int64_t)w0) : w0;
            if (ad.dn_hi[0] >= 0 && f64_isnan(v)) v = (acc[ad.dn_hi[0]] << 32) | (acc[ad.dn_lo[0]] & 0xFFFFFFFFull);
            return v;
        }
        default: return w0;  // counts
    }
}

// the words of a window state holding `value` whose first element has ordinal `first` (the state
// after one element of that value, in its written-back form: NaN bits at ordinal 0)
inline void ds_words_of(const CkPlan& p, uint64_t value, int64_t first, uint64_t* acc) {
    const AggDesc& ad = p.ad;
    acc_identity(p.wd, p.nw_t, acc);
    const int w0 = ad.w0[0];
    const bool f = ad.type[0] == FW_T_F64;
    switch (ad.kind[0]) {
        case FW_AGG_SUM: acc[w0] = ad.type[0] == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)value : value; break;
        case FW_AGG_MIN:
        case FW_AGG_MAX:
            acc[w0] = f ? (uint64_t)dkey(value) : ad.type[0] == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)value : value;
            if (ad.dn_hi[0] >= 0 && f64_isnan(value)) {
                acc[ad.dn_hi[0]] = value >> 32;
                acc[ad.dn_lo[0]] = value & 0xFFFFFFFFull;
            }
            break;
        case FW_AGG_MINBY:
        case FW_AGG_MAXBY:
            acc[w0] = f ? (uint64_t)dkey(f64_isnan(value) ? 0x7FF8000000000000ull : value)
                        : ad.type[0] == FW_T_I32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)value : value;
            acc[ad.by_prev] = (uint64_t)first;  // the restored element is retained
            break;
        default: acc[w0] = value; break;
    }
    // hidden counts (the sliding window's COUNT(*), a non-NULL count): only != 0 is observable
    if (ad.count_star_word >= 0 && ad.count_star_word != w0) acc[ad.count_star_word] = 1;
    if (ad.nn[0] >= 0 && ad.nn[0] != w0) acc[ad.nn[0]] = 1;
    if (ad.first_word >= 0) acc[ad.first_word] = (uint64_t)first;
}

// one key group's state -> its windows: *n = how many, the first min(*n, capacity) of them in out
inline int ds_encode(const CkPlan& p, const KgState& st, fw_ds_window* out, int64_t capacity, int64_t* n) {
    int64_t m = 0;
    for (size_t i = 0; i < st.ent.size(); i += (size_t)p.pwe) {
        const uint64_t* e = st.ent.data() + i;
        const uint32_t f = (uint32_t)e[2];
        const int32_t fl = ((f & F_ACC) ? FW_DSW_CONTENTS : 0) | ((f & F_TIMER) ? FW_DSW_TRIGGER : 0) |
                           ((f & F_CLEAN) ? FW_DSW_CLEANUP : 0);
        if (!fl) continue;
        if (out && m < capacity) {
            fw_ds_window& w = out[m];
            w.key = (int64_t)e[0];
            w.window_end = (int64_t)e[1];
            w.value = (f & F_ACC) ? (int64_t)ds_value_of(p.ad, e + 3) : 0;
            w.first_ord = (f & F_ACC) && p.ad.first_word >= 0 ? (int64_t)e[3 + p.ad.first_word] : -1;
            w.flags = fl;
            w.key_hash = 0;
        }
        m++;
    }
    *n = m;
    if (out && capacity < m) return set_error(FW_E_INVALID, "window buffer too small (%lld < %lld)", (long long)capacity, (long long)m);
    return FW_OK;
}

// n windows of key group `key_group` -> its state
inline int ds_decode(const CkPlan& p, int32_t key_group, const fw_ds_window* in, int64_t n, int64_t next_push_seq, KgState* out) {
    const WinDesc& win = p.win;
    const int pwe = p.pwe;
    std::vector<uint64_t> ent;
    ent.reserve((size_t)n * pwe);
    for (int64_t i = 0; i < n; i++) {
        const fw_ds_window& w = in[i];
        if (w.flags & ~(FW_DSW_CONTENTS | FW_DSW_TRIGGER | FW_DSW_CLEANUP) || !w.flags)
            return set_error(FW_E_INVALID, "window %lld: bad flags %d", (long long)i, w.flags);
        // a window of this assigner: start = end - size on the slide grid (SlidingEventTimeWindows
        // .assignWindows :77-90; tumbling: slide = size)
        const int64_t st = wsub(w.window_end, win.size);
        if (window_start(st, win.offset, win.slide_div) != st)
            return set_error(FW_E_INVALID, "window [%lld, %lld) is not a window of this assigner", (long long)st, (long long)w.window_end);
        if ((w.flags & FW_DSW_CLEANUP) && ds_cleanup_time(win, w.window_end) == INT64_MAX)
            return set_error(FW_E_INVALID, "window %lld has no cleanup time but a cleanup timer", (long long)w.window_end);
        // precomputed-hash keys (a shim's interned String keys): the window's superbucket comes from
        // the key's hash, routed as the ingest routes the key's records; the sub-bucket rides in the
        // high half of the flags word like a key-group blob's (kg_install)
        uint64_t sub = 0;
        if (p.ks.hash_kind == KH_PRE && !p.keyrow) {
            uint32_t m;
            const int sb = route_key(p.ks, w.key, w.key_hash, &m);
            if ((sb >> p.ks.sb_per_kg_log2) != key_group - p.ks.kg_start)
                return set_error(FW_E_INVALID, "window %lld: key hash %d is not in key group %d", (long long)i, w.key_hash, key_group);
            sub = (uint64_t)(sb & ((1 << p.ks.sb_per_kg_log2) - 1));
        }
        const size_t at = ent.size();
        ent.resize(at + pwe, 0);
        uint64_t* e = ent.data() + at;
        e[0] = (uint64_t)w.key;
        e[1] = (uint64_t)w.window_end;
        e[2] = ((w.flags & FW_DSW_CONTENTS) ? F_ACC : 0u) | ((w.flags & FW_DSW_TRIGGER) ? F_TIMER : 0u) |
               ((w.flags & FW_DSW_CLEANUP) ? F_CLEAN : 0u) | (sub << 32);
        if (w.flags & FW_DSW_CONTENTS) {
            if (p.ad.first_word >= 0 && (w.first_ord < 0 || (w.first_ord >> 32) >= next_push_seq))
                return set_error(FW_E_INVALID, "window %lld: first element ordinal not below push %lld", (long long)i,
                                 (long long)next_push_seq);
            ds_words_of(p, (uint64_t)w.value, w.first_ord, e + 3);
        } else {
            acc_identity(p.wd, p.nw_t, e + 3);
        }
    }
    out->key_group = key_group;
    out->sb_log2 = p.ks.sb_per_kg_log2;
    out->push_seq = std::max<int64_t>(next_push_seq, 0);
    out->ent = std::move(ent);
    out->kr = KeyRows{};
    return FW_OK;
}

}  // namespace fw
