// ckpt_san_driver.hip -- the checkpoint codecs of fw_ckpt_format.h under AddressSanitizer + UBSan, on
// the host alone (`make san`; no HIP call, no device).  For the key-group blob and the whole-handle blob
// of three small hand-built states it checks that encode -> decode -> encode gives the same bytes, that
// every proper prefix of a blob is refused, and that each single-field corruption a damaged savepoint
// could carry is refused with the output state untouched.  A sanitizer report aborts the program, so a
// clean exit with the last line "ok" is the assertion.
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

#include "fw_ckpt_format.h"

using namespace fw;

static std::string g_err;
int fw::set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

static int g_checks = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        g_checks++;                                   \
        if (!(cond)) {                                \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);             \
            fprintf(stderr, " (last error: %s)\n", g_err.c_str()); \
            exit(1);                                  \
        }                                             \
    } while (0)

typedef std::vector<uint8_t> Bytes;

template <typename T>
static void poke(Bytes& b, size_t at, T v) {
    CHECK(at + sizeof v <= b.size(), "poke past the blob");
    memcpy(b.data() + at, &v, sizeof v);
}

// One state in both forms, with its layout.  The key-group form holds the entries of key group 1
// (superbuckets 2 and 3 of 4), the whole-handle form the same entries under their superbuckets.
struct Case {
    const char* name;
    CkLayout L;
    KgState kg;
    SnapState snap;
};

static const int64_t SENTINEL = -7777;

static uint64_t flags_from(uint32_t flags, int sub) { return (uint64_t)flags | ((uint64_t)sub << 32); }

// n entries of pwe words: key, slice, flags, then words counting up
static Case make_case(const char* name, int pwe, int nw, int nw_t, bool keyrow, const std::vector<int64_t>& keys,
                      const std::vector<int>& subs, uint32_t flags) {
    Case c{name, CkLayout{}, KgState{}, SnapState{}};
    c.L = CkLayout{4, 4, pwe, nw, nw_t, 1, 0, 2, keyrow ? FW_KEYHASH_KEYROW : FW_KEYHASH_BINROW_BIGINT, keyrow, 8, 32, 1000, 250,
                   0x1234567887654321ull};
    c.kg.key_group = 1;
    c.kg.sb_log2 = 1;
    c.kg.cur = 4999;
    c.kg.push_seq = 12;
    c.snap.cur = 4999;
    c.snap.late_dropped = 3;
    c.snap.push_seq = 12;
    c.snap.cnt.assign(4, 0);
    for (size_t i = 0; i < keys.size(); i++) {
        std::vector<uint64_t> e((size_t)pwe);
        e[0] = (uint64_t)keys[i];
        e[1] = (uint64_t)(5000 + 250 * (int64_t)i);
        e[2] = flags;
        for (int w = 3; w < pwe; w++) e[(size_t)w] = 100 * (i + 1) + (uint64_t)w;
        c.snap.ent.insert(c.snap.ent.end(), e.begin(), e.end());
        c.snap.cnt[(size_t)(2 + subs[i])]++;
        e[2] = flags_from(flags, subs[i]);
        c.kg.ent.insert(c.kg.ent.end(), e.begin(), e.end());
    }
    if (keyrow) {
        const uint64_t row16[2] = {0, 41}, row24[3] = {0, 42, 0x6162636465666768ull};
        for (KeyRows* kr : {&c.kg.kr, &c.snap.kr}) {
            kr->add(5, 0x9e3779b9u, row16, 16);
            kr->add(7, 0x85ebca6bu, row24, 24);
        }
    }
    return c;
}

// the codec pair of one blob kind over one case: encode the case's state, decode into a state whose
// marker must survive every refusal, encode what a decode gave
struct Codec {
    const char* kind;
    std::function<int(void*, int64_t, int64_t*)> encode;
    std::function<int(const CkLayout&, const Bytes&, int64_t)> decode;  // (layout, blob, size): rc, marker checked on refusal
    std::function<int(void*, int64_t, int64_t*)> reencode;              // of the last successful decode
    size_t hdr, ent_at;  // header bytes; where the entries start
};

static Bytes encode_all(const std::function<int(void*, int64_t, int64_t*)>& enc) {
    int64_t size = -1;
    CHECK(enc(nullptr, 0, &size) == FW_OK && size > 0, "size query");
    Bytes b((size_t)size);
    int64_t again = -1;
    CHECK(enc(b.data(), size - 1, &again) == FW_E_INVALID && again == size, "a buffer one byte short is refused");
    CHECK(enc(b.data(), size, &again) == FW_OK && again == size, "encode");
    return b;
}

static void run(const Case& c, const Codec& k) {
    const Bytes blob = encode_all(k.encode);
    // encode -> decode -> encode
    CHECK(k.decode(c.L, blob, (int64_t)blob.size()) == FW_OK, "%s %s: decode of a valid blob", c.name, k.kind);
    CHECK(encode_all(k.reencode) == blob, "%s %s: encode -> decode -> encode differs", c.name, k.kind);
    // every proper prefix
    for (size_t n = 0; n < blob.size(); n++) {
        Bytes cut(blob.begin(), blob.begin() + (long)n);  // its own allocation: a read past n is a report
        cut.shrink_to_fit();
        CHECK(k.decode(c.L, cut, (int64_t)n) != FW_OK, "%s %s: prefix of %zu bytes accepted", c.name, k.kind, n);
    }
    auto refused = [&](const char* what, const Bytes& b, int code = 0) {
        const int rc = k.decode(c.L, b, (int64_t)b.size());
        CHECK(rc != FW_OK && (!code || rc == code), "%s %s: %s gave %d", c.name, k.kind, what, rc);
    };
    Bytes b;
    const bool whole = k.hdr == sizeof(SnapHeader);
    const size_t n_at = whole ? offsetof(SnapHeader, live) : offsetof(KgHeader, n);
    b = blob, poke<int64_t>(b, n_at, -1), refused("n = -1", b);
    b = blob, poke<int64_t>(b, n_at, (int64_t)1 << 61), refused("n = 2^61", b);
    b = blob, poke<uint64_t>(b, 0, SNAP_MAGIC ^ KG_MAGIC ^ (whole ? SNAP_MAGIC : KG_MAGIC)), refused("the other blob's magic", b);
    b = blob, poke<uint64_t>(b, 0, 0), refused("magic 0", b);
    b = blob, poke<int32_t>(b, 8, CK_VERSION + 1), refused("wrong version", b);
    b = blob, poke<int32_t>(b, 8, CK_VERSION - 1), refused("old version", b);
    b = blob, poke<uint64_t>(b, whole ? offsetof(SnapHeader, semantics) : offsetof(KgHeader, semantics), c.L.semantics + 1),
    refused("wrong fingerprint", b);
    if (whole) {
        const size_t cnt_at = sizeof(SnapHeader);  // counts: 0, 0, then the two superbuckets with entries
        b = blob, poke<int32_t>(b, cnt_at + 8, c.L.cap_e + 1), refused("a count above cap_e", b);
        b = blob, poke<int32_t>(b, cnt_at + 8, 0x7fffffff), refused("a count of INT32_MAX", b);
        b = blob, poke<int32_t>(b, cnt_at + 8, -1), refused("a negative count", b);
        b = blob, poke<int32_t>(b, cnt_at + 0, -1), poke<int32_t>(b, cnt_at + 4, 1), refused("a negative count the sum hides", b);
        b = blob, poke<int32_t>(b, cnt_at + 0, 1), refused("counts above live", b);
        b = blob, poke<int32_t>(b, cnt_at + 8, 0), refused("counts below live", b);
    }
    if (!c.L.keyrow) return;
    const size_t n_ent = c.kg.ent.size() / (size_t)c.L.pwe;
    const size_t sec = k.ent_at + n_ent * (size_t)c.L.pwe * 8;  // [n][id, hash << 32 | length, image]...
    const uint64_t len_word = (uint64_t)0x9e3779b9u << 32;
    b = blob, b.insert(b.end(), 4, 0), refused("a size that is no multiple of 8 past the entries", b);
    b = blob, poke<uint64_t>(b, sec + 16, len_word | 12), refused("a key-row length of 12", b);
    b = blob, poke<uint64_t>(b, sec + 16, len_word | 0), refused("a key-row length of 0", b);
    b = blob, poke<uint64_t>(b, sec + 16, len_word | (uint64_t)(c.L.kr_max_len + 1)), refused("a key-row length of max_len + 1", b);
    b = blob, poke<uint64_t>(b, sec + 16, len_word | (uint64_t)(c.L.kr_max_len + 8)), b.insert(b.end(), 64, 0),
    refused("a key-row length of max_len + 8, with the bytes for it", b);
    b = blob, poke<uint64_t>(b, sec, (uint64_t)c.L.kr_cap_ids + 1), refused("a key-row count above cap_ids", b);
    b = blob, poke<uint64_t>(b, sec, (uint64_t)1 << 40), refused("a key-row count of 2^40", b);
    b = blob, poke<uint64_t>(b, sec, ~0ull), refused("a key-row count of -1", b);
    b = blob, poke<uint64_t>(b, k.ent_at, 99), refused("an entry whose key id is missing from the section", b);
    b = blob, poke<uint64_t>(b, sec + 8, 99), refused("a section that renames an entry's key id", b);
    CkLayout small = c.L;  // two rows in a blob for a table of one
    small.kr_cap_ids = 1;
    CHECK(k.decode(small, blob, (int64_t)blob.size()) == FW_E_CAPACITY, "%s %s: more key rows than the table holds", c.name, k.kind);
}

static void run_case(const Case& c) {
    KgState kg_out;
    SnapState snap_out;
    Codec kg{"key-group blob",
             [&](void* buf, int64_t cap, int64_t* size) { return kg_encode(c.L, c.kg, buf, cap, size); },
             [&](const CkLayout& L, const Bytes& b, int64_t n) {
                 kg_out = KgState{};
                 kg_out.cur = SENTINEL;
                 const int rc = kg_decode(L, b.data(), n, &kg_out);
                 if (rc) CHECK(kg_out.cur == SENTINEL && kg_out.ent.empty() && kg_out.kr.id.empty(), "a refused blob changed the state");
                 return rc;
             },
             [&](void* buf, int64_t cap, int64_t* size) { return kg_encode(c.L, kg_out, buf, cap, size); },
             sizeof(KgHeader), sizeof(KgHeader)};
    Codec snap{"whole-handle blob",
               [&](void* buf, int64_t cap, int64_t* size) { return snap_encode(c.L, c.snap, buf, cap, size); },
               [&](const CkLayout& L, const Bytes& b, int64_t n) {
                   snap_out = SnapState{};
                   snap_out.cur = SENTINEL;
                   const int rc = snap_decode(L, b.data(), n, &snap_out);
                   if (rc) CHECK(snap_out.cur == SENTINEL && snap_out.ent.empty() && snap_out.cnt.empty(), "a refused blob changed the state");
                   return rc;
               },
               [&](void* buf, int64_t cap, int64_t* size) { return snap_encode(c.L, snap_out, buf, cap, size); },
               sizeof(SnapHeader), sizeof(SnapHeader) + 4 * 4};
    run(c, kg);
    run(c, snap);
    // a key group of another subtask
    KgState other = c.kg;
    other.key_group = 2;
    int64_t size = 0;
    CHECK(kg_encode(c.L, other, nullptr, 0, &size) == FW_OK, "size query");
    Bytes b((size_t)size);
    CHECK(kg_encode(c.L, other, b.data(), size, &size) == FW_OK, "encode");
    CHECK(kg.decode(c.L, b, size) == FW_E_INVALID, "%s: a key group the subtask does not own", c.name);
    printf("%s %d\n", c.name, g_checks);
}

int main() {
    // one word per entry, three entries over the key group's two sub-buckets
    run_case(make_case("one_word", 4, 1, 1, false, {11, 12, 13}, {0, 0, 1}, F_ACC | F_TIMER));
    // HOP block entries: the block's HB_R slices of nw_t words behind key, block start, flags
    run_case(make_case("hop_block", 3 + HB_R * 2, 2, 2, false, {21, 22}, {1, 0}, 0x5u << HB_MASK_SHIFT));
    // key rows: entries keyed by table ids 5 (16 bytes) and 7 (24 bytes)
    run_case(make_case("key_rows", 4, 1, 1, true, {5, 7, 5}, {0, 1, 1}, F_ACC | F_TIMER));
    uint64_t none[MAX_WORDS];
    WordDesc wd{};
    wd.nw = 1;
    wd.op[0] = 0;
    acc_identity(wd, 2, none);
    CHECK(none[0] == word_identity(0) && none[1] == 0, "acc_identity");
    printf("ok\n");
    return 0;
}
