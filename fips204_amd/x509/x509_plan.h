// The pure arithmetic of libmldsa_x509.so (include/mldsa_x509.h): the strict DER reader, the walk over one X.509 Certificate and the
// link rule that ties a certificate to its issuer.  No HIP here: every function is constexpr and takes the certificate's bytes through
// a fetch functor f(pos) -> byte pos of the certificate, 0 <= pos < len, so the kernels of x509.hip call these very functions on the
// blob and tests/cpp/x509_plan_main.cpp compiles the file alone, under the sanitizers, on a heap block of exactly len bytes.  The range
// check, the key and signature lengths and the classes are those of ../rec/rec_plan.h, included and not copied.
//
// Positions are relative to the certificate's first byte and 32 bits wide, as its length is.  No function fetches a position at or
// behind the `end` it was given, and every `end` is at most len: the walk never reads outside [off, off + len).
// The walk is a fixed sequence of at most 13 read_tlv steps; no loop in it runs to a count taken from the data.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../rec/rec_plan.h"

namespace mldsa_x509 {

using mldsa_rec::class_of_set;
using mldsa_rec::CLASS_REFUSED;
using mldsa_rec::in_range;
using mldsa_rec::pk_len;
using mldsa_rec::sig_len;

// the status codes and the flag of include/mldsa_x509.h (x509.hip asserts the equality)
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_ALG = 3, ST_SIG = 4, ST_ISSUER = 5, ST_NAME = 6, ST_PARSE_ONLY = 7;
constexpr uint32_t FLAG_CHECK_NAMES = 1;
constexpr uint32_t NO_ISSUER = 0xFFFFFFFFu;
constexpr uint32_t OID_LEN = 11;  // 06 09 60 86 48 01 65 03 04 03 xx: the content of an ML-DSA AlgorithmIdentifier, parameters absent

// ---- one TLV ----------------------------------------------------------------------------------------------------------------------------
struct Tlv {
    bool ok = false;
    uint32_t tag = 0;
    uint32_t at = 0;   // first content byte
    uint32_t len = 0;  // content bytes: the TLV ends at at + len <= end
};

// The TLV at pos inside [pos, end).  Refused (ok = false): fewer than two bytes before end; a high-tag-number tag ((tag & 0x1F) == 0x1F);
// the length byte 0x80 (indefinite) or above 0x84; a long form whose length bytes overrun end, whose first length byte is 0 or whose
// value fits a shorter form (0x81 with a value below 128; k bytes with a value below 2^(8 (k - 1)), which is a first byte of 0 again);
// content that overruns end.
template <class Fetch>
constexpr Tlv read_tlv(const Fetch& f, uint32_t pos, uint32_t end) {
    Tlv t;
    if (pos > end || end - pos < 2) return t;
    t.tag = f(pos);
    if ((t.tag & 0x1F) == 0x1F) return t;
    const uint32_t l0 = f(pos + 1);
    uint32_t hl = 2, value = l0;
    if (l0 >= 0x80) {
        const uint32_t k = l0 & 0x7F;
        if (k == 0 || k > 4 || k > end - pos - 2) return t;
        value = 0;
        for (uint32_t j = 0; j < 4; ++j)  // four steps at most, whatever the data says
            if (j < k) value = (value << 8) | f(pos + 2 + j);
        if (value >> (8 * (k - 1)) == 0) return t;  // the first length byte is 0
        if (k == 1 && value < 128) return t;
        hl = 2 + k;
    }
    if (value > end - pos - hl) return t;
    t.at = pos + hl;
    t.len = value;
    t.ok = true;
    return t;
}

// 44 / 65 / 87 where the OID_LEN bytes at pos are id-ml-dsa-44 / -65 / -87, else 0.  The caller vouches for pos + OID_LEN <= end.
template <class Fetch>
constexpr uint32_t oid_set(const Fetch& f, uint32_t pos) {
    uint64_t lo = 0;
    for (uint32_t j = 0; j < 8; ++j) lo |= (uint64_t)f(pos + j) << (8 * j);
    if (lo != 0x0365014886600906ull || f(pos + 8) != 0x04 || f(pos + 9) != 0x03) return 0;
    const uint32_t b = f(pos + 10);
    return b == 0x11 ? 44 : b == 0x12 ? 65 : b == 0x13 ? 87 : 0;
}

// the OID_LEN bytes at a_at and at b_at are the same, byte for byte.  The caller vouches for both ranges: the contents of two
// AlgorithmIdentifiers of OID_LEN bytes each.  The walks of a certificate, a CRL and a certification request call this; their signed
// envelope and ALG / SIG rule stay written out in each, because as functions they change the registers of the kernels that inline them
// (the rule of ../layer/layer_dev.h; DESIGN.md has the numbers).
template <class Fetch>
constexpr bool same_alg(const Fetch& f, uint32_t a_at, uint32_t b_at) {
    bool same = true;
    for (uint32_t j = 0; j < OID_LEN; ++j)
        if (same && f(a_at + j) != f(b_at + j)) same = false;
    return same;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// What the walk finds, relative to the certificate.  A status of ST_DER leaves everything else 0.  sig_off and sig_set are nonzero only
// where the status is ST_OK; key_off and key_set only where the subject key is an ML-DSA key of the right length.
struct Walk {
    uint32_t tbs_off = 0, tbs_len = 0, sig_off = 0, key_off = 0, issuer_off = 0, issuer_len = 0, subject_off = 0, subject_len = 0;
    uint32_t sig_set = 0, key_set = 0;
    int status = ST_DER;
};

// The certificate's len bytes (2 <= len: the caller's range check).  Structure first, everywhere on the path, then the algorithm
// identifiers, then the signature's length: the first rule broken in that order is the status.
template <class Fetch>
constexpr Walk walk(const Fetch& f, uint32_t len) {
    const Walk der;  // what every structural refusal returns
    // 1. Certificate ::= SEQUENCE, filling [0, len) exactly
    const Tlv cert = read_tlv(f, 0, len);
    if (!cert.ok || cert.tag != 0x30 || cert.at + cert.len != len) return der;
    // 2. tbsCertificate, signatureAlgorithm, signatureValue, ending at the Certificate's end
    const Tlv tbs = read_tlv(f, cert.at, len);
    if (!tbs.ok || tbs.tag != 0x30) return der;
    const Tlv alg = read_tlv(f, tbs.at + tbs.len, len);
    if (!alg.ok || alg.tag != 0x30) return der;
    const Tlv sig = read_tlv(f, alg.at + alg.len, len);
    if (!sig.ok || sig.tag != 0x03 || sig.at + sig.len != len) return der;
    // 3. inside the TBS: [0] version (optional), serialNumber, signature, issuer, validity, subject, subjectPublicKeyInfo
    const uint32_t tend = tbs.at + tbs.len;
    Tlv t = read_tlv(f, tbs.at, tend);
    if (t.ok && t.tag == 0xA0) t = read_tlv(f, t.at + t.len, tend);
    if (!t.ok || t.tag != 0x02) return der;
    const Tlv inner = read_tlv(f, t.at + t.len, tend);
    if (!inner.ok || inner.tag != 0x30) return der;
    const Tlv issuer = read_tlv(f, inner.at + inner.len, tend);
    if (!issuer.ok || issuer.tag != 0x30) return der;
    const Tlv validity = read_tlv(f, issuer.at + issuer.len, tend);
    if (!validity.ok || validity.tag != 0x30) return der;
    const Tlv subject = read_tlv(f, validity.at + validity.len, tend);
    if (!subject.ok || subject.tag != 0x30) return der;
    const Tlv spki = read_tlv(f, subject.at + subject.len, tend);
    if (!spki.ok || spki.tag != 0x30) return der;
    const uint32_t send = spki.at + spki.len;
    const Tlv kalg = read_tlv(f, spki.at, send);
    if (!kalg.ok || kalg.tag != 0x30) return der;
    const Tlv key = read_tlv(f, kalg.at + kalg.len, send);
    if (!key.ok || key.tag != 0x03 || key.at + key.len != send) return der;

    Walk w;
    w.tbs_off = cert.at;
    w.tbs_len = tend - cert.at;
    w.issuer_off = inner.at + inner.len;
    w.issuer_len = issuer.at + issuer.len - w.issuer_off;
    w.subject_off = validity.at + validity.len;
    w.subject_len = subject.at + subject.len - w.subject_off;
    // the subject key: not a rule of the certificate, it only decides whether the certificate can be an issuer
    const uint32_t kset = kalg.len == OID_LEN ? oid_set(f, kalg.at) : 0;
    if (kset != 0 && key.len == 1 + pk_len(class_of_set(kset)) && f(key.at) == 0) {
        w.key_set = kset;
        w.key_off = key.at + 1;
    }
    // the outer algorithm, and the inner one byte for byte the same TLV (the outer one is 30 0B and OID_LEN bytes by now)
    const uint32_t sset = alg.len == OID_LEN ? oid_set(f, alg.at) : 0;
    const bool same = sset != 0 && inner.len == OID_LEN && same_alg(f, inner.at, alg.at);  // (a minimal length: both headers are 30 0B)
    w.status = ST_ALG;
    if (!same) return w;
    w.status = ST_SIG;
    if (sig.len != 1 + sig_len(class_of_set(sset)) || f(sig.at) != 0) return w;
    w.status = ST_OK;
    w.sig_set = sset;
    w.sig_off = sig.at + 1;
    return w;
}

// ---- the link rule ----------------------------------------------------------------------------------------------------------------------
// The status of a signed item (a certificate, a CRL) after its own walk (own_status, own_sig_set) and before the names are compared.
// `issuer` is its issuer's index among n certificates; issuer_status and issuer_key_set are read from the issuer's fields row only
// where issuer < n (pass 0 otherwise).  An issuer whose own status is ST_ALG or ST_SIG (or anything the link gave it) still lends its
// key.
constexpr int signer_status(int own_status, uint32_t own_sig_set, uint32_t issuer, uint64_t n, int issuer_status, uint32_t issuer_key_set) {
    if (own_status != ST_OK) return own_status;
    if (issuer >= n) return ST_ISSUER;
    if (issuer_status == ST_RANGE || issuer_status == ST_DER) return ST_ISSUER;
    if (issuer_key_set == 0 || issuer_key_set != own_sig_set) return ST_ISSUER;
    return ST_OK;
}

// the certificate's: a certificate may name no issuer at all and is then parsed only
constexpr int link_status(int own_status, uint32_t own_sig_set, uint32_t issuer, uint64_t n, int issuer_status, uint32_t issuer_key_set) {
    if (own_status != ST_OK) return own_status;
    if (issuer == NO_ISSUER) return ST_PARSE_ONLY;
    return signer_status(own_status, own_sig_set, issuer, n, issuer_status, issuer_key_set);
}

// Byte idx of the two Name TLVs at blob positions a and b, both len bytes long: their difference, 0 behind the Names' end.  Here f
// fetches from the blob, and the caller vouches for both ranges lying inside it.
template <class Fetch>
constexpr uint32_t name_byte_diff(const Fetch& f, uint64_t a, uint64_t b, uint32_t len, uint64_t idx) {
    return idx < len ? (uint32_t)(f(a + idx) ^ f(b + idx)) : 0;
}

// the whole comparison, as one lane would make it: true where the Names differ in length or in any byte
template <class Fetch>
constexpr bool names_differ(const Fetch& f, uint64_t a, uint32_t a_len, uint64_t b, uint32_t b_len) {
    if (a_len != b_len) return true;
    uint32_t diff = 0;
    for (uint64_t idx = 0; idx < a_len; ++idx) diff |= name_byte_diff(f, a, b, a_len, idx);
    return diff != 0;
}

}  // namespace mldsa_x509
