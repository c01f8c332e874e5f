/* mldsa_csr.h -- certification requests on the device: PKCS#10 CSRs in a blob to proof-of-possession descriptors and to
 * TBSCertificates laid out in an output buffer (libmldsa_csr.so).
 *
 * A CA that issues ML-DSA certificates (the IETF profile cited in mldsa_seed.h) does not start from a TBSCertificate: it starts from a
 * DER CertificationRequest.  It checks that the request is signed by the key it carries (proof of possession), then builds the
 * TBSCertificate from the request's subject and key and its own issuer Name, serial number, validity and extensions.  This library does
 * both steps on the device: it walks every request, writes one mldsa_rec_op per request -- key = the request's own key, message = its
 * CertificationRequestInfo, pure mode with an empty context -- and, given the verdicts, assembles the TBSCertificates back to back in
 * `out` with one mldsa_x509sign_req each.  Any mix of ML-DSA-44 / 65 / 87; the host touches no byte.
 *
 * A C caller turns a batch of requests into a batch of signed certificates with five calls on one stream:
 *     mldsa_csr_parse(ctx, blob, blob_len, items, n, fields, ops, parse_status, stream);
 *     mldsa_rec_verify(ctx, MLDSA_MODE_PURE, blob, blob_len, ops, n, ok, scratch, scratch_bytes, NULL, stream);
 *     mldsa_csr_tbs(ctx, blob, blob_len, fields, entries, ok, n, tbs, tbs_len, reqs, status, totals, plan, plan_bytes, stream);
 *     mldsa_x509sign_issue_ops(ctx, tbs, tbs_len, reqs, n, n_keys, out, out_len, out_certs, sign_ops, sign_status, ...);
 *     mldsa_recsign_sign(ctx, MLDSA_MODE_PURE, keys, tbs, tbs_len, sign_ops, n, out, out_len, sig_status, ...);
 * Request i becomes a certificate where status[i], sign_status[i] and sig_status[i] are all 0.  A refused request's rows are all zero,
 * which each call behind refuses by its own first rule without reading or writing a byte for it.  A caller that signs hedged keeps
 * the randomness in the TBS buffer behind the tbs_len it gives mldsa_csr_tbs and gives mldsa_x509sign_issue_ops the larger length:
 * rnd_off goes through uninterpreted.  MlDsaCertificateRequests.issue_device of the Python package is these five calls.
 *
 * THE CONTRACT: every TBSCertificate this library writes passes mldsa_x509sign_plan, given a valid key row and room: walk_tbs of
 * fips204_amd/x509sign/x509sign_plan.h and its ALG rule accept it for the entry's set.  After mldsa_x509sign_issue_ops and
 * mldsa_recsign_sign, mldsa_x509_parse finds the certificate's subject Name and subject key equal to the request's bytes and its issuer
 * Name equal to the template's bytes.
 *
 * IN SCOPE: the strict DER structure of the request fields walked, its two algorithm identifiers, the lengths of key and signature,
 * the assembly of a v3 TBSCertificate from caller-supplied template ranges, the layout of `out`.
 * NOT IN SCOPE, and not looked at: attribute or extensionRequest contents; name policy and validity dates; PEM; CRLs; HashML-DSA and
 * external-mu variants; host-memory, group and batcher forms; the C++ and Rust mirrors.  A caller that needs them does them elsewhere.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.  It takes the types mldsa_rec_op
 * (mldsa_rec.h) and mldsa_x509sign_req (mldsa_x509sign.h) and the status codes 0 ... 4 of mldsa_x509.h -- it neither links nor calls
 * libmldsa_rec.so, libmldsa_recsign.so, libmldsa_x509.so or libmldsa_x509sign.so.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched, and no
 * call waits for the host.
 *
 * Public data only: requests, names and keys.  Nothing here is cleared.
 *
 * Cost, from counts (the expectation): the walk is about 10 dependent header reads per request, the assembly reads and writes 1.4 ... 2.7
 *   KB per request; mldsa_x509.h's walk is 1.6 ... 3.4 % of the verification behind it and mldsa_x509sign.h's frame about 1 % of the
 *   signing behind it, so both stages here should cost a few per cent of the two crypto calls.
 * Measured on an MI355X, 65 536 requests signed by their own keys, 5 mod 16 bytes apart, 1 024 keys per set, one shared issuer Name and
 *   Validity, an 8-byte serial each, no extensions (profiles/csr_bench.jsonl; medians of alternating runs in one process; "copy" is a
 *   device-to-device copy that moves the bytes the write kernel moves, in the same run):
 *                                                     ML-DSA-44   ML-DSA-65   ML-DSA-87   even three-way mix
 *     mldsa_csr_parse                                 0.029 ms    0.031 ms    0.032 ms    0.031 ms     (under 0.5 ns per request)
 *     mldsa_csr_parse / mldsa_rec_verify on its ops   0.015       0.011       0.008       0.008        (1.90 / 2.82 / 4.27 / 4.02 ms)
 *     mldsa_csr_tbs                                   0.126 ms    0.135 ms    0.151 ms    0.137 ms     (1.9 ... 2.3 ns per request)
 *     mldsa_csr_tbs / mldsa_x509sign_issue_ops
 *       + mldsa_recsign_sign on its output            0.023       0.017       0.015       0.014        (5.40 / 7.74 / 9.90 / 10.05 ms)
 *     the five calls / the three existing ones        1.019       1.015       1.010       1.011
 *     k_csr_tbs_write, read + written                 1.47 TB/s   2.02 TB/s   2.43 TB/s   1.93 TB/s
 *     copy                                            4.39 TB/s   5.10 TB/s   5.14 TB/s   4.91 TB/s
 *     Python walk + assembly + upload + the existing
 *       calls / the five calls                        40          30          23          23           (4.4 ... 4.8 us per request on the host)
 *   The write kernel's rate grows with the SPKI: a request is six pieces, four of them under 64 bytes, so a wave's fixed cost per piece
 *   shows, not the bytes.
 */
#ifndef MLDSA_CSR_H
#define MLDSA_CSR_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_rec.h"
#include "mldsa_x509.h"
#include "mldsa_x509sign.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_CSR_ABI_VERSION 1
/* most requests of one call */
#define MLDSA_CSR_MAX_REQUESTS (1u << 30)
/* requests per workgroup of the walk and of the plan's check and apply passes (one request per thread): the unit of the scan */
#define MLDSA_CSR_SCAN_BLOCK 256
/* flags bit 0 of an issue entry: copied through to the mldsa_x509sign_req, where it is MLDSA_X509SIGN_RND */
#define MLDSA_CSR_RND 1
/* the longest serial number content (RFC 5280) */
#define MLDSA_CSR_SERIAL_MAX 20

/* ---- status: the first rule broken.  Codes 0 ... 4 are mldsa_x509.h's; the new ones are disjoint from its 4 ... 7 and from
 * mldsa_x509sign.h's 8 ... 11. */
#define MLDSA_CSR_VERSION 12  /* stage 1: the version's content is not the single byte 00 */
#define MLDSA_CSR_KEY 13      /* stage 1: the SPKI algorithm's content is not the outer algorithm's 11 bytes, or the key BIT STRING is not
                                 1 + PK_LEN of that set long with unused-bits byte 0 */
#define MLDSA_CSR_POP 14      /* stage 2: ok[i] != 1 */
#define MLDSA_CSR_ENTRY 15    /* stage 2: set none of MLDSA_44 / 65 / 87, a flag bit other than bit 0, reserved nonzero, serial_len 0 or
                                 above MLDSA_CSR_SERIAL_MAX */
#define MLDSA_CSR_TEMPLATE 16 /* stage 2: a template range outside the blob or not the TLV it must be (below) */
#define MLDSA_CSR_LONG 17     /* stage 2: tbs_len > 65517 - SIG_LEN of the entry's set: mldsa_x509sign.h's own LONG limit */
#define MLDSA_CSR_SPACE 18    /* stage 2: the TBSCertificate's range does not lie inside [0, out_len) */

/* ==== stage 1: the walk ====================================================================================================================
 * input: one per request, a device array, 8-byte aligned, 16 bytes each.  [off, off + len) of the blob -- uint8[blob_len] in device
 * memory, NO alignment requirement -- is one DER CertificationRequest.  Blob and array are untrusted. */
typedef struct {
    uint64_t off;
    uint32_t len;
    uint32_t reserved; /* ignored */
} mldsa_csr_item;

/* what the walk finds: one row per request, a device array, 8-byte aligned, 56 bytes each.  Offsets are absolute blob offsets.
 *   cri_off, cri_len          the whole CertificationRequestInfo TLV: the message of the proof of possession
 *   sig_off                   the first byte behind the unused-bits byte of the signature BIT STRING
 *   key_off                   the first byte behind the unused-bits byte of the subjectPublicKey BIT STRING
 *   subject_off, subject_len  the whole subject Name TLV;  spki_off, spki_len the whole SubjectPublicKeyInfo TLV
 *   set                       MLDSA_44 / MLDSA_65 / MLDSA_87: the set of key and signature
 * A status of RANGE or DER leaves every other field 0.  sig_off, key_off and set are nonzero only where the status is OK. */
typedef struct {
    uint64_t cri_off, sig_off, key_off, subject_off, spki_off;
    uint32_t cri_len, subject_len, spki_len;
    uint8_t set, status;
    uint8_t reserved[2];
} mldsa_csr_fields;

/* The walk (fips204_amd/csr/csr_plan.h: one function, which the kernel and a stand-alone host program both run).  read_tlv is
 * mldsa_x509.h's.
 *   1. The CertificationRequest: tag 0x30, filling [0, len) exactly (trailing bytes are DER).
 *   2. Its content: CertificationRequestInfo 0x30, AlgorithmIdentifier 0x30, BIT STRING 0x03, ending exactly at the end.
 *   3. Inside the CertificationRequestInfo, in this order: 0x02 the version, 0x30 the subject (recorded), 0x30 the SubjectPublicKeyInfo
 *      (recorded), whose content is 0x30 then 0x03 ending exactly at its end, and 0xA0 the attributes, ending exactly at the
 *      CertificationRequestInfo's end.  The attributes' content is not walked: A0 00 is fine.
 * A fixed sequence of 10 read_tlv steps: no loop depends on data for its bound.  No byte outside [off, off + len) is ever read.
 * Status, the first rule broken in this order:
 *   MLDSA_X509_RANGE 1    rec's test off <= blob_len && len <= blob_len - off fails, or len < 2
 *   MLDSA_X509_DER 2      any structural failure above
 *   MLDSA_CSR_VERSION 12  the version's content is not the single byte 00
 *   MLDSA_X509_ALG 3      the outer algorithm's content is not exactly 06 09 60 86 48 01 65 03 04 03 {11|12|13}
 *   MLDSA_CSR_KEY 13      see above
 *   MLDSA_X509_SIG 4      the signature BIT STRING is not 1 + SIG_LEN long with unused-bits byte 0 */

int mldsa_csr_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_csr_last_error(void);

/* fields[i], ops[i], status[i] = the walk of request i.  For an accepted request (status OK)
 *     ops[i]: pk_off = key_off, sig_off = sig_off, msg_off / msg_len = the CertificationRequestInfo TLV, ctx_off = 0, ctx_len = 0,
 *     set = the request's, reserved = 0;
 * for every other request the op is all zero, which mldsa_rec_verify refuses (set = 0) without reading a byte: its ok[i] is 0.
 * One launch, k_csr_parse: one request per lane, MLDSA_CSR_SCAN_BLOCK lanes per workgroup -- the walk is a chain of dependent small
 * loads, so what scales is the number of chains in flight.  Asynchronous on `stream`.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, items, fields, ops or status, NULL blob with blob_len > 0, items, fields or ops not
 *   8-byte aligned, n > MLDSA_CSR_MAX_REQUESTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_csr_parse(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_csr_item *items, size_t n, mldsa_csr_fields *fields,
                    mldsa_rec_op *ops, uint8_t *status, void *stream);

/* ==== stage 2: the TBSCertificate ==========================================================================================================
 * input: entry i belongs to request i; a device array, 8-byte aligned, 64 bytes each, untrusted.  The template ranges lie in the same
 * blob as the requests; many entries may share them, and the issuer Name may point into a CA certificate. */
typedef struct {
    uint64_t serial_off;   /* serial_len content bytes of the serialNumber INTEGER */
    uint64_t issuer_off;   /* the issuer Name TLV */
    uint64_t validity_off; /* the Validity TLV */
    uint64_t ext_off;      /* with ext_len > 0: the [3] extensions TLV; else neither followed nor checked */
    uint64_t rnd_off;      /* copied through to reqs_out[i].rnd_off, not interpreted */
    uint32_t issuer_len, validity_len, ext_len;
    uint32_t key;    /* copied through: the row of the issuer's private key */
    uint32_t issuer; /* copied through */
    uint8_t serial_len; /* 1 ... MLDSA_CSR_SERIAL_MAX */
    uint8_t set;        /* MLDSA_44 / MLDSA_65 / MLDSA_87: the set of the key that will sign the certificate */
    uint8_t flags;      /* bit 0 = MLDSA_CSR_RND, copied through */
    uint8_t reserved;   /* must be 0 */
} mldsa_csr_issue;

/* The TBSCertificate written:
 *     30 82 hh ll | A0 03 02 01 02 | 02 sl <serial> | 30 0B 06 09 60 86 48 01 65 03 04 03 {11|12|13} (the entry's set)
 *                 | issuer Name TLV | validity TLV | subject TLV (from the request) | SPKI TLV (from the request) | extensions TLV if ext_len > 0
 * tbs_len = 4 + 20 + serial_len + issuer_len + validity_len + subject_len + spki_len + ext_len.  The content is never below 256 bytes
 * -- the SPKI alone is at least 1334 --, and LONG keeps it below 65536: the two-byte long form is always the minimal one.
 * TBSCertificates are laid out in input order, back to back from out + 0, by a stable exclusive scan of tbs_len: a refused request
 * takes no room.  `out` -- uint8[out_len] in device memory -- has NO alignment requirement and must not overlap the blob.
 *
 * Status, the first rule broken in this order (`ok` is the verdict array of mldsa_rec_verify, uint8[n]):
 *   (stage 1's status)     the fields row's status where it is not OK
 *   MLDSA_X509_RANGE 1     the row's subject or SPKI range does not lie inside the blob
 *   MLDSA_CSR_POP 14       ok[i] != 1
 *   MLDSA_CSR_ENTRY 15     see above
 *   MLDSA_CSR_TEMPLATE 16  the serial, issuer, validity or (with ext_len > 0) extensions range does not lie inside the blob; the issuer
 *                          or the validity range is not exactly one 0x30 TLV filling it; the extensions range is not exactly one 0xA3
 *                          TLV filling it; the serial's first byte is >= 0x80 (negative); serial_len > 1 with a first byte of 0 and a
 *                          second below 0x80 (not minimal)
 *   MLDSA_CSR_LONG 17      see above
 *   MLDSA_CSR_SPACE 18     see above.  Offsets only grow, so once one request is SPACE every later accepted one is too.
 * For a refused request no byte of `out` is written.
 *
 * output, per request:
 *   reqs_out[i]  mldsa_x509sign_req: off / len = the TBSCertificate in `out`; rnd_off, key, issuer, set and flags the entry's, not
 *                interpreted; reserved = 0.  All zero when the request is refused.  8-byte aligned.
 *   status[i]    uint8
 *   totals       one struct in device memory, 8-byte aligned */
typedef struct {
    uint64_t accepted;  /* requests with status MLDSA_X509_OK */
    uint64_t refused;   /* all others: accepted + refused = n */
    uint64_t out_bytes; /* what all requests that pass every rule but SPACE need back to back */
} mldsa_csr_totals;

/* ---- host helpers ---------------------------------------------------------------------------------------------------------------------------
 * tbs_len of the pieces under `set`; 0 for an unknown set, a serial_len of 0 or above MLDSA_CSR_SERIAL_MAX, or a LONG length. */
size_t mldsa_csr_tbs_len(int set, size_t serial_len, size_t issuer_len, size_t validity_len, size_t subject_len, size_t spki_len,
                         size_t ext_len);
/* The plan's working memory.  With R(x) = x rounded up to a multiple of 256 and B = ceil(n / MLDSA_CSR_SCAN_BLOCK) workgroups:
 *   R(16 B) + R(4 n)            two 64-bit sums per workgroup (TBS bytes, accepted requests); tbs_len of every request
 * 0 for n > MLDSA_CSR_MAX_REQUESTS. */
size_t mldsa_csr_plan_bytes(size_t n);

/* ---- 1. the plan: status, place and mldsa_x509sign_req of every request -----------------------------------------------------------------------
 *   plan     mldsa_csr_plan_bytes(n) bytes, 256-byte aligned, caller-owned, used in stream order.
 * Asynchronous on `stream`: three launches ordered by the kernel boundaries.  k_csr_check (one request per lane) applies the rules up
 *   to LONG and writes tbs_len (0 when refused) and two sums per workgroup; k_csr_offsets (one wave) turns the sums into exclusive
 *   prefixes and writes the totals; k_csr_apply scans inside each workgroup, runs the SPACE rule and writes reqs_out and status.  No
 *   kernel waits on another workgroup and every loop runs to a count the host passed.  `out` is not touched.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, fields, entries, ok, reqs_out, status, totals or plan, NULL blob with blob_len > 0,
 *   fields, entries, reqs_out or totals not 8-byte aligned, plan not 256-byte aligned or smaller than mldsa_csr_plan_bytes,
 *   n > MLDSA_CSR_MAX_REQUESTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_csr_tbs_plan(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_csr_fields *fields, const mldsa_csr_issue *entries,
                       const uint8_t *ok, size_t n, uint64_t out_len, mldsa_x509sign_req *reqs_out, uint8_t *status, mldsa_csr_totals *totals,
                       void *plan, size_t plan_bytes, void *stream);

/* ---- 2. the write: every accepted request's TBSCertificate --------------------------------------------------------------------------------------
 * One launch, k_csr_tbs_write: one request per wave.  Individual lanes write the 24 fixed bytes; the six pieces -- serial, issuer,
 *   validity, subject, SPKI, extensions -- are copied by the plan of fips204_amd/rec/rec_plan.h: bytes one by one up to the
 *   destination's first 16-byte boundary, then aligned 16-byte loads funnel-shifted in registers to aligned 16-byte stores, then the
 *   rest one by one.  It re-derives nothing from the requests' DER: it reads the entry, the fields row, reqs_out[i] and status[i], and it
 *   checks every range of the entry and the row against blob_len, reqs_out[i] against out_len and reqs_out[i].len against the length
 *   recomputed from the pieces -- so a row that was tampered with reads nothing outside the blob and writes nothing outside `out`: such a
 *   request is skipped.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, fields, entries, reqs_out or status, NULL blob with blob_len > 0, NULL out with
 *   out_len > 0, fields, entries or reqs_out not 8-byte aligned, `out` overlapping the blob (checked from the two pointer ranges),
 *   n > MLDSA_CSR_MAX_REQUESTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_csr_tbs_write(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_csr_fields *fields, const mldsa_csr_issue *entries,
                        size_t n, uint8_t *out, uint64_t out_len, const mldsa_x509sign_req *reqs_out, const uint8_t *status, void *stream);

/* ---- 3. both on `stream`: mldsa_csr_tbs_plan then mldsa_csr_tbs_write; the argument errors of both, before anything is launched ------------- */
int mldsa_csr_tbs(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_csr_fields *fields, const mldsa_csr_issue *entries,
                  const uint8_t *ok, size_t n, uint8_t *out, uint64_t out_len, mldsa_x509sign_req *reqs_out, uint8_t *status,
                  mldsa_csr_totals *totals, void *plan, size_t plan_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_CSR_H */
