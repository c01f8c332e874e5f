// The pure arithmetic of libmldsa_csr.so (include/mldsa_csr.h): the strict walk over one DER CertificationRequest, the refusal rules of
// an untrusted issue entry and the bytes of the TBSCertificate assembled from it.  No HIP here: every function is constexpr and takes
// bytes through a fetch functor, so the kernels of csr.hip call these very functions on the blob and tests/cpp/csr_plan_main.cpp
// compiles the file alone, under the sanitizers, on heap blocks of exactly len bytes.  The TLV reader and the OID test are those of
// ../x509/x509_plan.h, the range check, the lengths and the classes those of ../rec/rec_plan.h, the LONG bound and the algorithm
// identifier's bytes those of ../x509sign/x509sign_plan.h: included and not copied.
//
// The walk's fetch functor f(pos) gives byte pos of the request, 0 <= pos < len; positions are 32 bits wide, as the length is.  No
// function fetches a position at or behind the `end` it was given.  The entry rules' functor gives byte pos of the BLOB (64 bits).
//
// The TBSCertificate:
//     30 82 hh ll | A0 03 02 01 02 | 02 sl | <serial> | 30 0B 06 09 60 86 48 01 65 03 04 03 {11|12|13} | issuer | validity | subject | SPKI | [ext]
// PREFIX_LEN = 11 fixed bytes in front of the serial, ALG_LEN = 13 behind it, then the pieces copied from the blob.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mldsa_csr.h"
#include "../rec/rec_plan.h"
#include "../x509/x509_plan.h"
#include "../x509sign/x509sign_plan.h"

namespace mldsa_csr {

using mldsa_rec::class_of_set;
using mldsa_rec::CLASS_44;
using mldsa_rec::CLASS_65;
using mldsa_rec::CLASS_87;
using mldsa_rec::CLASS_REFUSED;
using mldsa_rec::in_range;
using mldsa_rec::pk_len;
using mldsa_rec::sig_len;
using mldsa_x509::oid_set;
using mldsa_x509::OID_LEN;
using mldsa_x509::read_tlv;
using mldsa_x509::same_alg;
using mldsa_x509::Tlv;
using mldsa_x509sign::max_tbs_len;

// the status codes of include/mldsa_csr.h (csr.hip asserts the equality); 0 ... 4 are mldsa_x509.h's
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_ALG = 3, ST_SIG = 4;
constexpr int ST_VERSION = 12, ST_KEY = 13, ST_POP = 14, ST_ENTRY = 15, ST_TEMPLATE = 16, ST_LONG = 17, ST_SPACE = 18;
constexpr uint32_t FLAG_RND = 1;
constexpr uint32_t SERIAL_MAX = 20;
constexpr uint32_t PREFIX_LEN = 11, ALG_LEN = 13, FIXED_LEN = PREFIX_LEN + ALG_LEN;
constexpr size_t SCAN_BLOCK = 256;  // MLDSA_CSR_SCAN_BLOCK

// ---- stage 1: the walk ------------------------------------------------------------------------------------------------------------------
// What the walk finds, relative to the request.  A status of ST_DER leaves everything else 0; sig_off, key_off and set are nonzero only
// where the status is ST_OK.
struct Walk {
    uint32_t cri_off = 0, cri_len = 0, sig_off = 0, key_off = 0, subject_off = 0, subject_len = 0, spki_off = 0, spki_len = 0;
    uint32_t set = 0;
    int status = ST_DER;
};

// The request's len bytes (2 <= len: the caller's range check).  Structure first, everywhere on the path, then the version, the outer
// algorithm, the key, the signature's length: the first rule broken in that order is the status.  Ten read_tlv steps.
template <class Fetch>
constexpr Walk walk(const Fetch& f, uint32_t len) {
    const Walk der;  // what every structural refusal returns
    // 1. CertificationRequest ::= SEQUENCE, filling [0, len) exactly
    const Tlv req = read_tlv(f, 0, len);
    if (!req.ok || req.tag != 0x30 || req.at + req.len != len) return der;
    // 2. certificationRequestInfo, signatureAlgorithm, signature, ending at the request's end
    const Tlv cri = read_tlv(f, req.at, len);
    if (!cri.ok || cri.tag != 0x30) return der;
    const uint32_t cend = cri.at + cri.len;
    const Tlv alg = read_tlv(f, cend, len);
    if (!alg.ok || alg.tag != 0x30) return der;
    const Tlv sig = read_tlv(f, alg.at + alg.len, len);
    if (!sig.ok || sig.tag != 0x03 || sig.at + sig.len != len) return der;
    // 3. inside the CertificationRequestInfo: version, subject, subjectPKInfo, [0] attributes
    const Tlv version = read_tlv(f, cri.at, cend);
    if (!version.ok || version.tag != 0x02) return der;
    const Tlv subject = read_tlv(f, version.at + version.len, cend);
    if (!subject.ok || subject.tag != 0x30) return der;
    const Tlv spki = read_tlv(f, subject.at + subject.len, cend);
    if (!spki.ok || spki.tag != 0x30) return der;
    const uint32_t send = spki.at + spki.len;
    const Tlv kalg = read_tlv(f, spki.at, send);
    if (!kalg.ok || kalg.tag != 0x30) return der;
    const Tlv key = read_tlv(f, kalg.at + kalg.len, send);
    if (!key.ok || key.tag != 0x03 || key.at + key.len != send) return der;
    const Tlv attrs = read_tlv(f, send, cend);
    if (!attrs.ok || attrs.tag != 0xA0 || attrs.at + attrs.len != cend) return der;

    Walk w;
    w.cri_off = req.at;
    w.cri_len = cend - req.at;
    w.subject_off = version.at + version.len;
    w.subject_len = subject.at + subject.len - w.subject_off;
    w.spki_off = subject.at + subject.len;
    w.spki_len = send - w.spki_off;
    w.status = ST_VERSION;
    if (version.len != 1 || f(version.at) != 0) return w;
    w.status = ST_ALG;
    const uint32_t set = alg.len == OID_LEN ? oid_set(f, alg.at) : 0;
    if (set == 0) return w;
    // the SPKI's algorithm byte for byte the outer one (both contents are OID_LEN bytes by now), the key of that set's length
    w.status = ST_KEY;
    const bool same = kalg.len == OID_LEN && same_alg(f, kalg.at, alg.at);
    if (!same || key.len != 1 + pk_len(class_of_set(set)) || f(key.at) != 0) return w;
    w.status = ST_SIG;
    if (sig.len != 1 + sig_len(class_of_set(set)) || f(sig.at) != 0) return w;
    w.status = ST_OK;
    w.set = set;
    w.sig_off = sig.at + 1;
    w.key_off = key.at + 1;
    return w;
}

// ---- stage 2: the rules -------------------------------------------------------------------------------------------------------------------
// byte pos of a range of the blob that begins at `base`, as read_tlv wants it
template <class Fetch>
struct From {
    const Fetch& f;
    uint64_t base;
    constexpr uint32_t operator()(uint32_t pos) const { return f(base + pos); }
};

// [off, off + len) of the blob (inside it: the caller's range check) is exactly one TLV of `tag`
template <class Fetch>
constexpr bool one_tlv(const Fetch& blob, uint64_t off, uint32_t len, uint32_t tag) {
    const Tlv t = read_tlv(From<Fetch>{blob, off}, 0, len);
    return t.ok && t.tag == tag && t.at + t.len == len;
}

// the length of the TBSCertificate of entry e and row r: 64 bits, so six 32-bit lengths cannot wrap it
constexpr uint64_t tbs_len(const mldsa_csr_issue& e, const mldsa_csr_fields& r) {
    return (uint64_t)4 + 20 + e.serial_len + e.issuer_len + e.validity_len + r.subject_len + r.spki_len + e.ext_len;
}

// The first rule of include/mldsa_csr.h's stage-2 list a request breaks, up to LONG; ST_OK where its TBSCertificate may be laid out.
// Of the blob it reads the headers of the template TLVs and two bytes of the serial, each only behind its range check.
template <class Fetch>
constexpr int tbs_status(const Fetch& blob, uint64_t blob_len, const mldsa_csr_fields& r, const mldsa_csr_issue& e, uint32_t ok) {
    if (r.status != ST_OK) return r.status;
    if (!in_range(r.subject_off, r.subject_len, blob_len) || !in_range(r.spki_off, r.spki_len, blob_len)) return ST_RANGE;
    if (ok != 1) return ST_POP;
    const int c = class_of_set(e.set);
    if (c == CLASS_REFUSED || (e.flags & ~FLAG_RND) != 0 || e.reserved != 0 || e.serial_len == 0 || e.serial_len > SERIAL_MAX) return ST_ENTRY;
    if (!in_range(e.serial_off, e.serial_len, blob_len) || !in_range(e.issuer_off, e.issuer_len, blob_len) ||
        !in_range(e.validity_off, e.validity_len, blob_len) || (e.ext_len > 0 && !in_range(e.ext_off, e.ext_len, blob_len)))
        return ST_TEMPLATE;
    if (!one_tlv(blob, e.issuer_off, e.issuer_len, 0x30) || !one_tlv(blob, e.validity_off, e.validity_len, 0x30)) return ST_TEMPLATE;
    if (e.ext_len > 0 && !one_tlv(blob, e.ext_off, e.ext_len, 0xA3)) return ST_TEMPLATE;
    const uint32_t s0 = blob(e.serial_off);
    if (s0 >= 0x80) return ST_TEMPLATE;
    if (e.serial_len > 1 && s0 == 0 && blob(e.serial_off + 1) < 0x80) return ST_TEMPLATE;
    if (tbs_len(e, r) > max_tbs_len(c)) return ST_LONG;
    return ST_OK;
}

// What k_csr_tbs_write asks before it follows an offset or writes a byte: every range of the entry and the row inside the blob, the
// request row's length the one recomputed from the pieces and inside the bound, its range inside `out`.  Nothing of the blob is read.
constexpr bool write_allowed(const mldsa_csr_fields& r, const mldsa_csr_issue& e, uint64_t q_off, uint32_t q_len, uint64_t blob_len,
                             uint64_t out_len) {
    const int c = class_of_set(e.set);
    if (c == CLASS_REFUSED || e.serial_len == 0 || e.serial_len > SERIAL_MAX) return false;
    if (!in_range(e.serial_off, e.serial_len, blob_len) || !in_range(e.issuer_off, e.issuer_len, blob_len) ||
        !in_range(e.validity_off, e.validity_len, blob_len) || (e.ext_len > 0 && !in_range(e.ext_off, e.ext_len, blob_len)))
        return false;
    if (!in_range(r.subject_off, r.subject_len, blob_len) || !in_range(r.spki_off, r.spki_len, blob_len)) return false;
    const uint64_t len = tbs_len(e, r);
    return len <= max_tbs_len(c) && len == q_len && in_range(q_off, q_len, out_len);
}

// ---- stage 2: the bytes -------------------------------------------------------------------------------------------------------------------
// byte j < PREFIX_LEN of a TBSCertificate of `total` bytes: SEQUENCE and two length bytes, [0] { INTEGER 2 } (v3), the serial's header
constexpr uint32_t prefix_byte(uint32_t j, uint32_t total, uint32_t serial_len) {
    const uint32_t content = total - 4;
    switch (j) {
        case 0: return 0x30;
        case 1: return 0x82;
        case 2: return (content >> 8) & 0xFF;
        case 3: return content & 0xFF;
        case 4: return 0xA0;
        case 5: return 0x03;
        case 6: return 0x02;
        case 7: return 0x01;
        case 8: return 0x02;
        case 9: return 0x02;
        default: return serial_len;
    }
}

// byte j < ALG_LEN behind the serial: the AlgorithmIdentifier of class c, which is the first ALG_LEN bytes of x509sign's trailer
constexpr uint32_t alg_byte(uint32_t j, int c) { return mldsa_x509sign::trailer_byte(j, c); }

// where the six copied pieces begin inside the TBSCertificate, in the order serial, issuer, validity, subject, SPKI, extensions
struct Pieces {
    uint32_t at[6] = {0, 0, 0, 0, 0, 0};
    uint32_t len[6] = {0, 0, 0, 0, 0, 0};
    uint32_t alg_at = 0;
};

// (the caller vouches for a length inside the LONG bound: 32 bits hold every position)
constexpr Pieces pieces(const mldsa_csr_issue& e, const mldsa_csr_fields& r) {
    Pieces p;
    p.len[0] = e.serial_len;
    p.len[1] = e.issuer_len;
    p.len[2] = e.validity_len;
    p.len[3] = r.subject_len;
    p.len[4] = r.spki_len;
    p.len[5] = e.ext_len;
    p.at[0] = PREFIX_LEN;
    p.alg_at = PREFIX_LEN + e.serial_len;
    p.at[1] = p.alg_at + ALG_LEN;
    for (int k = 2; k < 6; ++k) p.at[k] = p.at[k - 1] + p.len[k - 1];
    return p;
}

// the blob offset of piece k
constexpr uint64_t piece_off(const mldsa_csr_issue& e, const mldsa_csr_fields& r, int k) {
    return k == 0 ? e.serial_off : k == 1 ? e.issuer_off : k == 2 ? e.validity_off : k == 3 ? r.subject_off : k == 4 ? r.spki_off : e.ext_off;
}

// ---- the working memory (include/mldsa_csr.h spells the formula out) --------------------------------------------------------------------------
// the placement scan's of ../rec/rec_plan.h under this library's block and cap: the sums of TBS lengths and accepted requests, the lengths
constexpr size_t MAX_REQUESTS = (size_t)1 << 30;
constexpr size_t n_blocks(size_t n) { return mldsa_rec::scan_blocks(n, SCAN_BLOCK); }
constexpr size_t plan_sums_bytes(size_t n) { return mldsa_rec::place_sums_bytes(n, SCAN_BLOCK, mldsa_rec::PLACE_SUMS); }
constexpr size_t plan_bytes(size_t n) { return mldsa_rec::place_plan_bytes(n, SCAN_BLOCK, MAX_REQUESTS); }

}  // namespace mldsa_csr
