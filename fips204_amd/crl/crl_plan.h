// The pure arithmetic of libmldsa_crl.so (include/mldsa_crl.h): the walk over one CertificateList (RFC 5280 5.1), the rule of one revoked
// entry, the serial of a certificate, the placement of the entry table, the hash of a serial, the link rule that ties a CRL to its
// issuer and the order of the lookup's answers.  No HIP here: every function is constexpr and takes bytes through a fetch functor
// f(pos) -> byte pos, so the kernels of crl.hip call these very functions on the blob (or on a window of it held in LDS) and
// tests/cpp/crl_plan_main.cpp compiles the file alone, under the sanitizers, on heap blocks of exactly len bytes.  The DER reader, the
// OID test and the Name comparison are those of ../x509/x509_plan.h, the range check and the signature lengths those of
// ../rec/rec_plan.h: included, not copied.
//
// Positions are relative to the CRL's first byte and 32 bits wide, as its length is.  No function fetches a position at or behind the
// `end` it was given, and every `end` is at most len.  walk_crl is a fixed sequence of at most 12 read_tlv steps, walk_entry of at most
// 4 and cert_serial of at most 3: no loop in them runs to a count taken from the data.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../x509/x509_plan.h"

namespace mldsa_crl {

using mldsa_rec::class_of_set;
using mldsa_rec::in_range;
using mldsa_rec::sig_len;
using mldsa_x509::name_byte_diff;
using mldsa_x509::names_differ;
using mldsa_x509::OID_LEN;
using mldsa_x509::oid_set;
using mldsa_x509::read_tlv;
using mldsa_x509::same_alg;
using mldsa_x509::Tlv;

// the status codes, the flag and the caps of include/mldsa_crl.h (crl.hip asserts the equality); 0 ... 6 are include/mldsa_x509.h's
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_ALG = 3, ST_SIG = 4, ST_ISSUER = 5, ST_NAME = 6;
constexpr int ST_VERSION = 19, ST_ENTRY = 20, ST_SPACE = 21;
constexpr uint32_t FLAG_CHECK_NAMES = 1;
constexpr uint32_t SERIAL_MAX = 20;   // content bytes of a userCertificate INTEGER
constexpr uint32_t ENTRY_MIN = 20;    // the smallest legal entry: 30 12 | 02 01 xx | 17 0D and 13 bytes of UTCTime
constexpr uint32_t TIME_MIN = 13;     // content bytes of the shortest Time RFC 5280 allows (YYMMDDHHMMSSZ)
constexpr size_t SCAN_BLOCK = 256;    // MLDSA_CRL_SCAN_BLOCK
constexpr size_t MAX_CRLS = (size_t)1 << 30, MAX_ENTRIES = (size_t)1 << 30, MAX_CERTS = (size_t)1 << 30;
constexpr uint32_t CRL_NONE = 0xFFFFFFFFu;
// the answers of the lookup, in the order of their rules (answer() below)
constexpr int REV_GOOD = 0, REV_REVOKED = 1, REV_NO_CRL = 2, REV_CRL_INDEX = 3, REV_CRL_REFUSED = 4, REV_CERT = 5, REV_SCOPE = 6;

constexpr bool is_time(uint32_t tag) { return tag == 0x17 || tag == 0x18; }

// ---- the serial -------------------------------------------------------------------------------------------------------------------------
// An INTEGER's content of 1 ... SERIAL_MAX bytes at [at, at + len) in DER's shortest form: a leading 00 only before a byte >= 0x80, a
// leading FF only before a byte < 0x80.  The caller vouches for the range.
template <class Fetch>
constexpr bool serial_ok(const Fetch& f, uint32_t at, uint32_t len) {
    if (len == 0 || len > SERIAL_MAX) return false;
    if (len >= 2) {
        const uint32_t b0 = f(at), b1 = f(at + 1);
        if ((b0 == 0x00 && b1 < 0x80) || (b0 == 0xFF && b1 >= 0x80)) return false;
    }
    return true;
}

// A serial as the table holds it: its content bytes as they stand in the DER (sign byte included), zero-padded to SERIAL_MAX, in five
// little-endian words, and its length.  len = 0: none.
struct Serial {
    uint32_t w[5] = {0, 0, 0, 0, 0};
    uint32_t len = 0;
};

template <class Fetch>
constexpr uint32_t serial_word(const Fetch& f, uint32_t at, uint32_t len, uint32_t k) {
    uint32_t v = 0;
    if (4 * k + 0 < len) v |= (uint32_t)f(at + 4 * k + 0);
    if (4 * k + 1 < len) v |= (uint32_t)f(at + 4 * k + 1) << 8;
    if (4 * k + 2 < len) v |= (uint32_t)f(at + 4 * k + 2) << 16;
    if (4 * k + 3 < len) v |= (uint32_t)f(at + 4 * k + 3) << 24;
    return v;
}

// the serial at [at, at + len), 1 <= len <= SERIAL_MAX (serial_ok passed)
template <class Fetch>
constexpr Serial load_serial(const Fetch& f, uint32_t at, uint32_t len) {
    Serial s;
    s.w[0] = serial_word(f, at, len, 0);
    s.w[1] = serial_word(f, at, len, 1);
    s.w[2] = serial_word(f, at, len, 2);
    s.w[3] = serial_word(f, at, len, 3);
    s.w[4] = serial_word(f, at, len, 4);
    s.len = len;
    return s;
}

// ---- the hash ---------------------------------------------------------------------------------------------------------------------------
// The home slot of (crl, serial) is hash_serial(...) & (table_slots - 1).  A fixed mix: multiply by the golden ratio's odd neighbour and
// fold the high bits down, word after word, then murmur3's finalizer.  Nothing secret is hashed and nobody is served by a collision
// but the one who wrote the CRL, whose lookups then probe longer: the probe loop is bounded by the table's size either way.
constexpr uint32_t hash_step(uint32_t h, uint32_t v) {
    h = (h ^ v) * 0x9E3779B1u;
    return h ^ (h >> 15);
}

constexpr uint32_t hash_serial(uint32_t crl, const Serial& s) {
    uint32_t h = 0x811C9DC5u;
    h = hash_step(h, crl);
    h = hash_step(h, s.len);
    h = hash_step(h, s.w[0]);
    h = hash_step(h, s.w[1]);
    h = hash_step(h, s.w[2]);
    h = hash_step(h, s.w[3]);
    h = hash_step(h, s.w[4]);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// ---- the placement ----------------------------------------------------------------------------------------------------------------------
// slots a revokedCertificates content of `bytes` bytes can need: no legal entry is shorter than ENTRY_MIN
constexpr uint64_t entries_bound(uint64_t bytes) { return bytes / ENTRY_MIN; }

// slots of the lookup table over max_entries entry rows: the power of two >= 2 max_entries, at least 64; 0 past MAX_ENTRIES
constexpr uint64_t table_slots(uint64_t max_entries) {
    if (max_entries > MAX_ENTRIES) return 0;
    uint64_t t = 64;
    while (t < 2 * max_entries) t <<= 1;
    return t;
}

constexpr size_t n_blocks(size_t n) { return mldsa_rec::scan_blocks(n, SCAN_BLOCK); }
// the working memory of the placement: one 64-bit sum per workgroup of the scan, rounded up to 256 bytes; 0 past MAX_CRLS
constexpr size_t scratch_bytes(size_t n_crls) { return n_crls > MAX_CRLS ? 0 : mldsa_rec::place_sums_bytes(n_crls, SCAN_BLOCK, 1); }

// CRL i, whose header walk was accepted, has its slots at [first, first + bound) where they lie inside the table; else ST_SPACE
constexpr int place_status(uint64_t first, uint64_t bound, uint64_t max_entries) { return first + bound > max_entries ? ST_SPACE : ST_OK; }

// ---- the walk of the header -------------------------------------------------------------------------------------------------------------
// What the walk finds, relative to the CRL.  A status of ST_DER leaves everything else 0.  sig_off and sig_set are nonzero only where
// the status is ST_OK.  next_off = 0: no nextUpdate; has_revoked / has_ext tell an absent field from an empty one.
struct CrlWalk {
    uint32_t tbs_off = 0, tbs_len = 0, sig_off = 0, issuer_off = 0, issuer_len = 0, this_off = 0, next_off = 0;
    uint32_t revoked_off = 0, revoked_len = 0, ext_off = 0, ext_len = 0;
    uint32_t sig_set = 0;
    bool has_revoked = false, has_ext = false;
    int status = ST_DER;
};

// The CRL's len bytes (2 <= len: the caller's range check).  Structure first, everywhere on the path, then the rules in the order ALG,
// SIG, VERSION, ENTRY (the empty list): the first rule broken is the status.
template <class Fetch>
constexpr CrlWalk walk_crl(const Fetch& f, uint32_t len) {
    const CrlWalk der;  // what every structural refusal returns
    // 1. CertificateList ::= SEQUENCE, filling [0, len) exactly
    const Tlv list = read_tlv(f, 0, len);
    if (!list.ok || list.tag != 0x30 || list.at + list.len != len) return der;
    // 2. tbsCertList, signatureAlgorithm, signatureValue, ending at the list's end
    const Tlv tbs = read_tlv(f, list.at, len);
    if (!tbs.ok || tbs.tag != 0x30) return der;
    const Tlv alg = read_tlv(f, tbs.at + tbs.len, len);
    if (!alg.ok || alg.tag != 0x30) return der;
    const Tlv sig = read_tlv(f, alg.at + alg.len, len);
    if (!sig.ok || sig.tag != 0x03 || sig.at + sig.len != len) return der;
    // 3. inside the TBS: version (optional), signature, issuer, thisUpdate, nextUpdate (optional), revokedCertificates (optional),
    //    [0] crlExtensions (optional), ending at the TBS's end
    const uint32_t tend = tbs.at + tbs.len;
    Tlv t = read_tlv(f, tbs.at, tend);
    if (!t.ok) return der;
    const bool has_version = t.tag == 0x02;
    const Tlv version = t;
    if (has_version) t = read_tlv(f, t.at + t.len, tend);
    if (!t.ok || t.tag != 0x30) return der;
    const Tlv inner = t;
    const Tlv issuer = read_tlv(f, inner.at + inner.len, tend);
    if (!issuer.ok || issuer.tag != 0x30) return der;
    const Tlv this_update = read_tlv(f, issuer.at + issuer.len, tend);
    if (!this_update.ok || !is_time(this_update.tag)) return der;
    CrlWalk w;
    w.this_off = issuer.at + issuer.len;
    uint32_t pos = this_update.at + this_update.len;
    // the three optional fields: each is read only where bytes are left, and taken only where its tag stands
    bool have = pos < tend;
    if (have) {
        t = read_tlv(f, pos, tend);
        if (!t.ok) return der;
    }
    if (have && is_time(t.tag)) {
        w.next_off = pos;
        pos = t.at + t.len;
        have = pos < tend;
        if (have) {
            t = read_tlv(f, pos, tend);
            if (!t.ok) return der;
        }
    }
    if (have && t.tag == 0x30) {
        w.has_revoked = true;
        w.revoked_off = t.at;
        w.revoked_len = t.len;
        pos = t.at + t.len;
        have = pos < tend;
        if (have) {
            t = read_tlv(f, pos, tend);
            if (!t.ok) return der;
        }
    }
    if (have && t.tag == 0xA0) {
        const Tlv ext = read_tlv(f, t.at, t.at + t.len);
        if (!ext.ok || ext.tag != 0x30 || ext.at + ext.len != t.at + t.len) return der;
        w.has_ext = true;
        w.ext_off = ext.at;
        w.ext_len = ext.len;
        pos = t.at + t.len;
    }
    if (pos != tend) return der;  // a tag that belongs nowhere, or bytes behind the last field

    w.tbs_off = list.at;
    w.tbs_len = tend - list.at;
    w.issuer_off = inner.at + inner.len;
    w.issuer_len = issuer.at + issuer.len - w.issuer_off;
    // ALG: the outer algorithm, and the inner one byte for byte the same TLV (the outer one is 30 0B and OID_LEN bytes by now)
    const uint32_t sset = alg.len == OID_LEN ? oid_set(f, alg.at) : 0;
    const bool same = sset != 0 && inner.len == OID_LEN && same_alg(f, inner.at, alg.at);
    w.status = ST_ALG;
    if (!same) return w;
    w.status = ST_SIG;
    if (sig.len != 1 + sig_len(class_of_set(sset)) || f(sig.at) != 0) return w;
    // VERSION: 02 01 01 where there is one; extensions belong to version 2 alone
    w.status = ST_VERSION;
    if (has_version && (version.len != 1 || f(version.at) != 1)) return w;
    if (w.has_ext && !has_version) return w;
    // ENTRY: revokedCertificates is absent where nobody is revoked, never empty
    w.status = ST_ENTRY;
    if (w.has_revoked && w.revoked_len == 0) return w;
    w.status = ST_OK;
    w.sig_set = sset;
    w.sig_off = sig.at + 1;
    return w;
}

// ---- one revoked entry ------------------------------------------------------------------------------------------------------------------
struct Entry {
    bool ok = false;
    uint32_t next = 0;        // the position behind the entry
    uint32_t serial_at = 0;   // first content byte of userCertificate
    uint32_t serial_len = 0;  // 1 ... SERIAL_MAX
};

// The entry at pos inside the list that ends at `end`: SEQUENCE { userCertificate INTEGER (serial_ok), revocationDate Time of at
// least TIME_MIN bytes, crlEntryExtensions SEQUENCE OPTIONAL }, ending exactly at its own end.  Times and extensions are not read.
template <class Fetch>
constexpr Entry walk_entry(const Fetch& f, uint32_t pos, uint32_t end) {
    Entry e;
    const Tlv seq = read_tlv(f, pos, end);
    if (!seq.ok || seq.tag != 0x30) return e;
    const uint32_t eend = seq.at + seq.len;
    const Tlv serial = read_tlv(f, seq.at, eend);
    if (!serial.ok || serial.tag != 0x02 || !serial_ok(f, serial.at, serial.len)) return e;
    const Tlv date = read_tlv(f, serial.at + serial.len, eend);
    if (!date.ok || !is_time(date.tag) || date.len < TIME_MIN) return e;
    uint32_t behind = date.at + date.len;
    if (behind < eend) {
        const Tlv ext = read_tlv(f, behind, eend);
        if (!ext.ok || ext.tag != 0x30) return e;
        behind = ext.at + ext.len;
    }
    if (behind != eend) return e;
    e.ok = true;
    e.next = eend;
    e.serial_at = serial.at;
    e.serial_len = serial.len;
    return e;
}

// The hop from one entry's header to the next: the position behind the TLV at pos, or 0 where no TLV can be read there (a position
// behind a TLV is at least 2).  The hop reads headers only; what they frame is walk_entry's to judge.
template <class Fetch>
constexpr uint32_t hop(const Fetch& f, uint32_t pos, uint32_t end) {
    const Tlv t = read_tlv(f, pos, end);
    return t.ok ? t.at + t.len : 0;
}

// ---- the window -------------------------------------------------------------------------------------------------------------------------
// k_crl_entries keeps WINDOW bytes of the CRL in LDS, loaded in aligned 16-byte chunks.  Frame coordinates: 0 is the CRL's address
// rounded down to 16, so CRL position p lies at mis + p, mis = address & 15.  The window that serves position pos begins at
// ws = (mis + pos) rounded down to 16; of its chunks only those that lie wholly inside the CRL, [mis, mis + len), are loaded: the
// loaded part is [lo, hi), possibly empty (lo >= hi).  A position outside it is fetched from the blob.
constexpr uint32_t WINDOW = 1024;
struct Window {
    uint64_t ws = 0, lo = 0, hi = 0;
};

constexpr Window window_at(uint32_t mis, uint32_t len, uint32_t pos) {
    Window w;
    w.ws = ((uint64_t)mis + pos) & ~(uint64_t)15;
    w.lo = w.ws >= mis ? w.ws : w.ws + 16;
    const uint64_t last = ((uint64_t)mis + len) & ~(uint64_t)15;
    w.hi = w.ws + WINDOW < last ? w.ws + WINDOW : last;
    return w;
}

// chunk k (0 ... WINDOW / 16 - 1) of the window is loaded
constexpr bool window_chunk(const Window& w, uint32_t k) { return w.ws + 16 * k >= w.lo && w.ws + 16 * k + 16 <= w.hi; }
// frame coordinate q lies in the loaded part
constexpr bool window_holds(const Window& w, uint64_t q) { return q >= w.lo && q < w.hi; }

// ---- the serial of a certificate --------------------------------------------------------------------------------------------------------
// f fetches from the TBSCertificate TLV of tbs_len bytes: its header, an optional [0] version, then serialNumber by serial_ok.
template <class Fetch>
constexpr Serial cert_serial(const Fetch& f, uint32_t tbs_len) {
    const Serial none;
    const Tlv tbs = read_tlv(f, 0, tbs_len);
    if (!tbs.ok || tbs.tag != 0x30) return none;
    const uint32_t tend = tbs.at + tbs.len;
    Tlv t = read_tlv(f, tbs.at, tend);
    if (t.ok && t.tag == 0xA0) t = read_tlv(f, t.at + t.len, tend);
    if (!t.ok || t.tag != 0x02 || !serial_ok(f, t.at, t.len)) return none;
    return load_serial(f, t.at, t.len);
}

// ---- the link rule ----------------------------------------------------------------------------------------------------------------------
// The status of CRL i after walk, placement and entries (own_status, own_sig_set) and before the Names are compared: the certificate's
// rule without its "no issuer" case.  A CRL always names an issuer: 0xFFFFFFFF is an index like any other and, with n_certs at most
// 2^30, out of range.
constexpr int link_status(int own_status, uint32_t own_sig_set, uint32_t issuer, uint64_t n_certs, int issuer_status, uint32_t issuer_key_set) {
    return mldsa_x509::signer_status(own_status, own_sig_set, issuer, n_certs, issuer_status, issuer_key_set);
}

// ---- the lookup's answer ----------------------------------------------------------------------------------------------------------------
// The rules in their order; every argument behind the first that decides is ignored (pass anything).
constexpr int answer(bool has_crl, bool crl_in_range, bool crl_accepted, bool cert_ok, bool same_issuer, bool listed) {
    if (!has_crl) return REV_NO_CRL;
    if (!crl_in_range) return REV_CRL_INDEX;
    if (!crl_accepted) return REV_CRL_REFUSED;
    if (!cert_ok) return REV_CERT;
    if (!same_issuer) return REV_SCOPE;
    return listed ? REV_REVOKED : REV_GOOD;
}

}  // namespace mldsa_crl
