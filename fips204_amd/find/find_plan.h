// The pure arithmetic of libmldsa_find.so (include/mldsa_find.h): the walk over one Extensions SEQUENCE for the two key identifiers, the
// rule by which a range of a row may be followed, the keyed hash, the key comparison, the slot count and the scratch layout.  No HIP
// here: every function is constexpr and takes bytes through a fetch functor f(pos) -> byte, so the kernels of find.hip call these very
// functions on the blob and tests/cpp/find_plan_main.cpp compiles the file alone, under the sanitizers, on heap blocks of exactly the
// bytes it may read.  The DER reader and the range check are those of ../x509/x509_plan.h and ../rec/rec_plan.h, included and not
// copied.
//
// walk_ids fetches no position at or behind the `end` it was given; its one loop is bounded by MAX_EXTS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../x509/x509_plan.h"

namespace mldsa_find {

using mldsa_rec::in_range;
using mldsa_x509::NO_ISSUER;
using mldsa_x509::read_tlv;
using mldsa_x509::Tlv;

// the codes and caps of include/mldsa_find.h (find.hip asserts the equality)
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_ALG = 3, ST_SIG = 4, ST_EXT = 26;
constexpr int R_FOUND = 0, R_NONE = 1, R_CERT = 2, R_SPACE = 3;
constexpr uint32_t MAX_EXTS = 32, MAX_KEYID = 64, PROBE_MAX = 256, OVERFLOW_MAX = 1024;
constexpr uint64_t MAX_CERTS = 1u << 28;
constexpr uint32_t KIND_ANY = 1, KIND_SKI = 2, KIND_NOSKI = 3;
constexpr uint64_t EMPTY_TAG = ~0ull;          // a slot nobody has claimed; no hash takes this value (finish_hash)
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;      // slot_of: the entry's probe ran out
constexpr uint32_t NO_ENTRY = 0xFFFFFFFEu;     // slot_of: the certificate is no candidate
constexpr uint32_t CRL_NONE = 0xFFFFFFFFu;

// the row layouts (find.hip asserts them against the structs of the header)
constexpr size_t ID_BYTES = 24, ID_AKI_OFF = 8, ID_SKI_LEN = 16, ID_AKI_LEN = 17, ID_STATUS = 18;
constexpr size_t KEY_BYTES = 32;  // one Key (below), as the table keeps it for every entry
constexpr size_t RESULT_BYTES = 12, RESULT_CANDIDATES = 4, RESULT_STATUS = 8, TOTALS_BYTES = 16;

// ---- the table's size and the scratch -----------------------------------------------------------------------------------------------------
// (static: the host side calls these out of line, and a copy with external linkage would be a weak dynamic symbol of the library)
static constexpr size_t table_slots(size_t n) {
    if (n > MAX_CERTS) return 0;
    size_t s = 64;
    while (s < 4 * n) s <<= 1;
    return s;
}

static constexpr size_t round256(size_t x) { return (x + 255) / 256 * 256; }

struct Layout {
    size_t tags = 0, owners = 0, counts = 0, slot_of = 0, keys = 0, overflow = 0, ca_crl = 0, total = 0;
};

static constexpr Layout layout(size_t n) {
    Layout L;
    const size_t s = table_slots(n);
    if (n > MAX_CERTS) return L;
    L.tags = 0;
    L.owners = L.tags + round256(8 * s);
    L.counts = L.owners + round256(4 * s);
    L.slot_of = L.counts + round256(4 * s);
    L.keys = L.slot_of + round256(8 * n);
    L.overflow = L.keys + round256(2 * KEY_BYTES * n);
    L.ca_crl = L.overflow + round256(4 * OVERFLOW_MAX);
    L.total = L.ca_crl + round256(4 * n);
    return L;
}

static constexpr size_t scratch_bytes(size_t n) { return layout(n).total; }

// ---- which ranges are followed ------------------------------------------------------------------------------------------------------------
// [off, off + len) lies inside [outer_off, outer_off + outer_len); the caller vouches for the outer range lying in the blob
constexpr bool inside(uint64_t off, uint64_t len, uint64_t outer_off, uint64_t outer_len) {
    return off >= outer_off && in_range(off - outer_off, len, outer_len);
}

// the population of the table: the certificates whose key mldsa_x509_link will lend
constexpr bool candidate_row(int fields_status, uint32_t key_set, int id_status) {
    return (fields_status == ST_OK || fields_status == ST_ALG || fields_status == ST_SIG) && key_set != 0 && id_status == ST_OK;
}

constexpr bool seeker_row(int fields_status, uint32_t sig_set, int id_status) { return fields_status == ST_OK && sig_set != 0 && id_status == ST_OK; }

// ---- the identifiers ----------------------------------------------------------------------------------------------------------------------
// What walk_ids finds, positions as the functor's.  Every status but ST_OK leaves the rest 0.
struct Ids {
    uint32_t ski_off = 0, ski_len = 0, aki_off = 0, aki_len = 0;
    int status = ST_DER;
};

// The content of one Extensions SEQUENCE, [pos, end): the rules of the header.
template <class Fetch>
constexpr Ids walk_ids(const Fetch& f, uint32_t pos, uint32_t end) {
    const Ids der;
    Ids ext;
    ext.status = ST_EXT;
    uint32_t ski_at = 0, ski_end = 0, aki_at = 0, aki_end = 0, q = pos;
    bool bad_ext = false;
    for (uint32_t k = 0; k < MAX_EXTS && q < end; ++k) {  // MAX_EXTS rounds at most, whatever the data says
        const Tlv x = read_tlv(f, q, end);
        if (!x.ok || x.tag != 0x30) return der;
        const uint32_t xend = x.at + x.len;
        const Tlv oid = read_tlv(f, x.at, xend);
        if (!oid.ok || oid.tag != 0x06) return der;
        Tlv v = read_tlv(f, oid.at + oid.len, xend);
        if (v.ok && v.tag == 0x01) v = read_tlv(f, v.at + v.len, xend);
        if (!v.ok || v.tag != 0x04 || v.at + v.len != xend) return der;
        const bool id_ce = oid.len == 3 && f(oid.at) == 0x55 && f(oid.at + 1) == 0x1D;
        const uint32_t arc = id_ce ? f(oid.at + 2) : 0;
        if (arc == 0x0E) {
            if (ski_end != 0) bad_ext = true;  // twice
            else ski_at = v.at, ski_end = xend;
        } else if (arc == 0x23) {
            if (aki_end != 0) bad_ext = true;
            else aki_at = v.at, aki_end = xend;
        }
        q = xend;
    }
    if (q != end || bad_ext) return ext;  // more than MAX_EXTS extensions
    Ids out;
    if (ski_end != 0) {
        const Tlv s = read_tlv(f, ski_at, ski_end);
        if (!s.ok || s.tag != 0x04 || s.at + s.len != ski_end || s.len < 1 || s.len > MAX_KEYID) return ext;
        out.ski_off = s.at;
        out.ski_len = s.len;
    }
    if (aki_end != 0) {
        const Tlv seq = read_tlv(f, aki_at, aki_end);
        if (!seq.ok || seq.tag != 0x30 || seq.at + seq.len != aki_end) return ext;
        uint32_t p = seq.at;
        for (uint32_t m = 0; m < 3; ++m) {
            if (p >= aki_end) break;
            const Tlv t = read_tlv(f, p, aki_end);
            if (!t.ok) return ext;
            if (t.tag != (m == 0 ? 0x80u : m == 1 ? 0xA1u : 0x82u)) continue;  // absent: the next member may stand here
            if (m == 0) {
                if (t.len < 1 || t.len > MAX_KEYID) return ext;
                out.aki_off = t.at;
                out.aki_len = t.len;
            }
            p = t.at + t.len;
        }
        if (p != aki_end) return ext;
    }
    out.status = ST_OK;
    return out;
}

// ---- the key ------------------------------------------------------------------------------------------------------------------------------
// One key of the table or of a lookup: offsets are absolute blob offsets, and whoever made the Key vouches for both ranges.
struct Key {
    uint64_t name_off = 0, id_off = 0;
    uint32_t name_len = 0, id_len = 0, kind = 0, set = 0;
};
static_assert(sizeof(Key) == KEY_BYTES, "a Key of the table is 32 bytes");

// what two keys must agree in before a byte is compared
constexpr bool same_shape(const Key& a, const Key& b) {
    return a.kind == b.kind && a.set == b.set && a.name_len == b.name_len && a.id_len == b.id_len;
}

// byte idx of the two keys' Name (idx < name_len) or identifier (name_len <= idx < name_len + id_len): their difference
template <class Fetch>
constexpr uint32_t key_byte_diff(const Fetch& f, const Key& a, const Key& b, uint64_t idx) {
    if (idx < a.name_len) return (uint32_t)(f(a.name_off + idx) ^ f(b.name_off + idx));
    const uint64_t k = idx - a.name_len;
    return k < a.id_len ? (uint32_t)(f(a.id_off + k) ^ f(b.id_off + k)) : 0;
}

// the whole comparison, as one lane would make it
template <class Fetch>
constexpr bool keys_equal(const Fetch& f, const Key& a, const Key& b) {
    if (!same_shape(a, b)) return false;
    uint32_t diff = 0;
    for (uint64_t idx = 0; idx < (uint64_t)a.name_len + a.id_len; ++idx) diff |= key_byte_diff(f, a, b, idx);
    return diff == 0;
}

// ---- the hash -----------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// What byte `byte` at index idx of a key (key_byte_diff's numbering) adds to the sum: a 64-bit word drawn from the first seed word at
// (idx, byte).  The sum runs over the bytes in any order, so the lanes of a wave add their bytes and the partial sums are reduced.
constexpr uint64_t byte_term(uint64_t s0, uint64_t idx, uint32_t byte) { return mix64(s0 + ((idx << 8 | byte) + 1) * 0x9E3779B97F4A7C15ull); }

// the sum, kind, set and lengths to the tag, under the second seed word; hash_bits 1 ... 64; never EMPTY_TAG
constexpr uint64_t finish_hash(uint64_t sum, const Key& k, uint64_t s1, int hash_bits) {
    const uint64_t shape = (uint64_t)k.kind | (uint64_t)k.set << 8 | (uint64_t)k.id_len << 24 | (uint64_t)k.name_len << 32;
    uint64_t h = mix64(sum + mix64(s1 ^ shape) + s1);
    if (hash_bits < 64) h &= ((uint64_t)1 << hash_bits) - 1;
    return h == EMPTY_TAG ? EMPTY_TAG - 1 : h;
}

// the whole hash, as one lane would make it
template <class Fetch>
constexpr uint64_t key_hash(const Fetch& f, const Key& k, uint64_t s0, uint64_t s1, int hash_bits) {
    uint64_t sum = 0;
    for (uint64_t idx = 0; idx < k.name_len; ++idx) sum += byte_term(s0, idx, f(k.name_off + idx));
    for (uint64_t j = 0; j < k.id_len; ++j) sum += byte_term(s0, (uint64_t)k.name_len + j, f(k.id_off + j));
    return finish_hash(sum, k, s1, hash_bits);
}

// ---- the answer ---------------------------------------------------------------------------------------------------------------------------
// One lookup's part of an answer: the lowest matching candidate and how many there are, or `space`.
struct Match {
    uint32_t lowest = NO_ISSUER, count = 0;
    bool space = false;
};

// the answer of a seeker from its one or two lookups (b: count 0 where only one was made)
constexpr Match join(const Match& a, const Match& b) {
    Match m;
    m.space = a.space || b.space;
    if (m.space) return m;
    m.count = a.count + b.count;
    m.lowest = a.lowest < b.lowest ? a.lowest : b.lowest;
    return m;
}

constexpr int result_status(bool seeker, const Match& m) { return !seeker ? R_CERT : m.space ? R_SPACE : m.count != 0 ? R_FOUND : R_NONE; }

}  // namespace mldsa_find
