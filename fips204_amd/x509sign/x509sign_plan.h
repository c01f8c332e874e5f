// The pure arithmetic of libmldsa_x509sign.so (include/mldsa_x509sign.h): the refusal rules of an untrusted issuing request, the strict
// walk over one DER TBSCertificate and the frame that turns it into a Certificate.  No HIP here: every function is constexpr and takes
// the TBS's bytes through a fetch functor f(pos) -> byte pos of the TBS, 0 <= pos < len, so the kernels of x509sign.hip call these very
// functions on the blob and tests/cpp/x509sign_plan_main.cpp compiles the file alone, under the sanitizers, on a heap block of exactly
// len bytes.  The TLV reader and the OID test are those of ../x509/x509_plan.h, the range check, the lengths and the classes those of
// ../rec/rec_plan.h: included and not copied.
//
// The frame is fixed once the set is known:
//     30 82 hh ll | TBS | 30 0B 06 09 60 86 48 01 65 03 04 03 {11|12|13} | 03 82 hh ll 00 | SIG_LEN bytes
// HEADER_LEN = 4 bytes in front of the TBS, TRAILER_LEN = 18 behind it, then the hole.  The outer length is always the two-byte long
// form: the content is never below 2438 bytes, and a TBS that would push it above 65535 is refused (ST_LONG).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../rec/rec_plan.h"
#include "../x509/x509_plan.h"

namespace mldsa_x509sign {

using mldsa_rec::class_of_set;
using mldsa_rec::CLASS_44;
using mldsa_rec::CLASS_65;
using mldsa_rec::CLASS_87;
using mldsa_rec::CLASS_REFUSED;
using mldsa_rec::in_range;
using mldsa_rec::sig_len;
using mldsa_x509::oid_set;
using mldsa_x509::OID_LEN;
using mldsa_x509::read_tlv;
using mldsa_x509::Tlv;

// the status codes and the flag of include/mldsa_x509sign.h (x509sign.hip asserts the equality); 1 ... 3 are mldsa_x509.h's
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_ALG = 3, ST_ENTRY = 8, ST_KEY = 9, ST_LONG = 10, ST_SPACE = 11;
constexpr uint32_t FLAG_RND = 1;  // MLDSA_X509SIGN_RND: the request's 32 bytes of randomness lie at rnd_off
constexpr uint32_t RND_LEN = 32;
constexpr uint32_t HEADER_LEN = 4, TRAILER_LEN = 18, FRAME_LEN = HEADER_LEN + TRAILER_LEN;
constexpr size_t CHECK_BLOCK = 256;  // MLDSA_X509SIGN_SCAN_BLOCK: requests per workgroup of the check and apply passes

// ---- the frame --------------------------------------------------------------------------------------------------------------------------
// the longest TBS of class c: the Certificate's content, tbs_len + TRAILER_LEN + SIG_LEN, still fits two length bytes
constexpr uint32_t max_tbs_len(int c) { return 65535 - TRAILER_LEN - sig_len(c); }

// bytes of the finished certificate
constexpr uint32_t cert_len(int c, uint32_t tbs_len) { return tbs_len + FRAME_LEN + sig_len(c); }

// byte j < HEADER_LEN of the certificate: SEQUENCE, two length bytes of everything behind the header
constexpr uint32_t header_byte(uint32_t j, uint32_t total) {
    const uint32_t content = total - HEADER_LEN;
    return j == 0 ? 0x30 : j == 1 ? 0x82 : j == 2 ? (content >> 8) & 0xFF : content & 0xFF;
}

// byte j < TRAILER_LEN behind the TBS: the AlgorithmIdentifier of class c (13 bytes), then the BIT STRING's header and its unused-bits
// byte (5 bytes); the BIT STRING holds 1 + SIG_LEN bytes
constexpr uint32_t trailer_byte(uint32_t j, int c) {
    const uint32_t bits = 1 + sig_len(c);
    switch (j) {
        case 0: return 0x30;
        case 1: return 0x0B;
        case 2: return 0x06;
        case 3: return 0x09;
        case 4: return 0x60;
        case 5: return 0x86;
        case 6: return 0x48;
        case 7: return 0x01;
        case 8: return 0x65;
        case 9: return 0x03;
        case 10: return 0x04;
        case 11: return 0x03;
        case 12: return 0x11 + (uint32_t)c;
        case 13: return 0x03;
        case 14: return 0x82;
        case 15: return bits >> 8;
        case 16: return bits & 0xFF;
        default: return 0x00;
    }
}

// ---- the rules in front of the walk -------------------------------------------------------------------------------------------------------
// ENTRY, KEY, RANGE, LONG in the header's order; ST_OK where the TBS may be walked.  n_keys: the rows of the three key tables in class
// order; a set with no keys is not served, so every key of it is out of range.  Nothing of the blob is read.
constexpr int entry_status(uint64_t off, uint64_t rnd_off, uint32_t len, uint32_t key, uint32_t set, uint32_t flags, uint32_t reserved,
                           uint64_t blob_len, uint64_t n_keys_44, uint64_t n_keys_65, uint64_t n_keys_87) {
    const int c = class_of_set(set);
    if (c == CLASS_REFUSED || (flags & ~FLAG_RND) != 0 || reserved != 0) return ST_ENTRY;
    const uint64_t n_keys = c == CLASS_44 ? n_keys_44 : c == CLASS_65 ? n_keys_65 : n_keys_87;
    if (key >= n_keys) return ST_KEY;
    if (!in_range(off, len, blob_len) || len < 2) return ST_RANGE;
    if ((flags & FLAG_RND) != 0 && !in_range(rnd_off, RND_LEN, blob_len)) return ST_RANGE;
    if (len > max_tbs_len(c)) return ST_LONG;
    return ST_OK;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// The TBS's len bytes (2 <= len: the caller's range check) under the set that will sign it: ST_DER unless the TBS is one 0x30 TLV filling
// [0, len) exactly that holds, at the very positions step 3 of mldsa_x509::walk reads, an optional 0xA0, 0x02, 0x30 (the inner
// algorithm), 0x30, 0x30, 0x30, and 0x30 the SPKI whose content is 0x30 then 0x03 ending at its end; then ST_ALG unless the inner
// algorithm's content is exactly the OID_LEN bytes of `set`.  A fixed sequence of at most 10 read_tlv steps; no position at or behind
// len is fetched.
template <class Fetch>
constexpr int walk_tbs(const Fetch& f, uint32_t len, uint32_t set) {
    const Tlv tbs = read_tlv(f, 0, len);
    if (!tbs.ok || tbs.tag != 0x30 || tbs.at + tbs.len != len) return ST_DER;
    Tlv t = read_tlv(f, tbs.at, len);
    if (t.ok && t.tag == 0xA0) t = read_tlv(f, t.at + t.len, len);
    if (!t.ok || t.tag != 0x02) return ST_DER;
    const Tlv inner = read_tlv(f, t.at + t.len, len);
    if (!inner.ok || inner.tag != 0x30) return ST_DER;
    const Tlv issuer = read_tlv(f, inner.at + inner.len, len);
    if (!issuer.ok || issuer.tag != 0x30) return ST_DER;
    const Tlv validity = read_tlv(f, issuer.at + issuer.len, len);
    if (!validity.ok || validity.tag != 0x30) return ST_DER;
    const Tlv subject = read_tlv(f, validity.at + validity.len, len);
    if (!subject.ok || subject.tag != 0x30) return ST_DER;
    const Tlv spki = read_tlv(f, subject.at + subject.len, len);
    if (!spki.ok || spki.tag != 0x30) return ST_DER;
    const uint32_t send = spki.at + spki.len;
    const Tlv kalg = read_tlv(f, spki.at, send);
    if (!kalg.ok || kalg.tag != 0x30) return ST_DER;
    const Tlv key = read_tlv(f, kalg.at + kalg.len, send);
    if (!key.ok || key.tag != 0x03 || key.at + key.len != send) return ST_DER;
    // (a minimal length: an inner algorithm of OID_LEN bytes has the header 30 0B, as the trailer's has)
    if (inner.len != OID_LEN || oid_set(f, inner.at) != set) return ST_ALG;
    return ST_OK;
}

// ---- the working memory (include/mldsa_x509sign.h spells the formula out) -----------------------------------------------------------------
// the placement scan's of ../rec/rec_plan.h under this library's block and cap: the sums of certificate lengths and accepted requests,
// the lengths
constexpr size_t MAX_CERTS = (size_t)1 << 30;
constexpr size_t n_blocks(size_t n) { return mldsa_rec::scan_blocks(n, CHECK_BLOCK); }
constexpr size_t plan_sums_bytes(size_t n) { return mldsa_rec::place_sums_bytes(n, CHECK_BLOCK, mldsa_rec::PLACE_SUMS); }
constexpr size_t plan_bytes(size_t n) { return mldsa_rec::place_plan_bytes(n, CHECK_BLOCK, MAX_CERTS); }

}  // namespace mldsa_x509sign
