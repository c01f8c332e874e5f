/* mldsa_x509sign.h -- issuing X.509 certificates on the device: TBSCertificates in a blob to finished DER certificates in an output
 * buffer (libmldsa_x509sign.so).
 *
 * A CA or a test PKI that issues ML-DSA certificates (the IETF profile cited in mldsa_seed.h) holds a buffer of DER TBSCertificates,
 * often already on the device.  mldsa_recsign_sign (mldsa_recsign.h) signs messages where they lie and writes each signature into a
 * hole; what is left for a certificate is the frame around it -- Certificate ::= SEQUENCE { tbs, AlgorithmIdentifier, BIT STRING } --,
 * the check that the TBS is well formed and names the algorithm of the key that will sign it, and the place of the hole.  This library
 * does that on the device: it checks every TBSCertificate, lays the finished certificates out back to back in `out`, writes each
 * frame -- header, the TBS itself, algorithm identifier, BIT STRING header -- and one mldsa_recsign_op per certificate whose hole is
 * the BIT STRING's content.  Any mix of ML-DSA-44 / 65 / 87; the host takes no part.  It is the signing counterpart of mldsa_x509.h, as
 * mldsa_recsign.h is of mldsa_rec.h.
 *
 * A C caller issues a batch with two calls on one stream:
 *     mldsa_x509sign_issue_ops(ctx, blob, blob_len, reqs, n, n_keys, out, out_len, out_certs, ops, status, totals, plan, plan_bytes, stream);
 *     mldsa_recsign_sign(ctx, MLDSA_MODE_PURE, keys, blob, blob_len, ops, n, out, out_len, sig_status, scratch, scratch_bytes, NULL, stream);
 * Certificate i is issued where status[i] == MLDSA_X509_OK and sig_status[i] == MLDSA_OK: out_certs[i] then names its bytes in `out`.
 * Where the signer gave up on an accepted op (a sig_status other than MLDSA_OK) the hole holds zeros, as mldsa_recsign.h documents: the
 * frame is there, the certificate is not.  A refused request's op is all zero, which mldsa_recsign_sign refuses by its own rule 1
 * without reading or writing a byte.  out_certs is what mldsa_x509_ops (mldsa_x509.h) takes as it is, with `out` as its blob.
 * MlDsaCertificateIssuer.issue_device of the Python package is these two calls.
 *
 * THE CONTRACT: every certificate this library accepts and frames gets status MLDSA_X509_OK from mldsa_x509_parse, with
 * tbs_off = cert_off + 4, tbs_len = len and sig_off = the hole.
 *
 * IN SCOPE: the strict DER structure of the TBS fields that mldsa_x509.h walks, the inner signature algorithm against the signing
 * key's set, the frame, the layout of `out`.
 * NOT IN SCOPE, and not looked at: validity dates, extensions, name chaining or any other policy; PEM; CSRs; CRLs; HashML-DSA or
 * external-mu signatures; host-memory, group or batcher forms; the C++ / Rust mirrors.  A caller that needs them does them elsewhere.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.  From mldsa_recsign.h it takes the
 * descriptor type mldsa_recsign_op and from mldsa_x509.h the type mldsa_x509_cert -- it neither links nor calls libmldsa_recsign.so or
 * libmldsa_x509.so.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched, and no
 * call waits for the host.
 *
 * Public data only: TBSCertificates and frames.  The per-signature randomness is only pointed at (rnd_off goes through to the op),
 * never copied, so nothing here is cleared.
 */
#ifndef MLDSA_X509SIGN_H
#define MLDSA_X509SIGN_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_recsign.h"
#include "mldsa_x509.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_X509SIGN_ABI_VERSION 1
/* most certificates of one call */
#define MLDSA_X509SIGN_MAX_CERTS (1u << 30)
/* requests per workgroup of the check and apply passes (one request per thread): the unit of the scan */
#define MLDSA_X509SIGN_SCAN_BLOCK 256
/* flags bit 0: the request's 32 bytes of randomness lie at rnd_off in the blob (the hedged variant); clear: deterministic */
#define MLDSA_X509SIGN_RND 1

/* ---- input: one per certificate, a device array, 8-byte aligned, 32 bytes each ----------------------------------------------------------
 * The blob -- uint8[blob_len] in device memory, NO alignment requirement -- and the entries are untrusted. */
typedef struct {
    uint64_t off;      /* [off, off + len) of the blob = one DER TBSCertificate */
    uint64_t rnd_off;  /* with MLDSA_X509SIGN_RND: 32 bytes of randomness in the blob; else neither followed nor checked */
    uint32_t len;
    uint32_t key;      /* row of the set's private-key table: the issuer's key */
    uint32_t issuer;   /* copied through to out_certs[i].issuer, not interpreted */
    uint8_t set;       /* MLDSA_44 / MLDSA_65 / MLDSA_87: the signing key's set */
    uint8_t flags;     /* bit 0 = MLDSA_X509SIGN_RND */
    uint16_t reserved; /* must be 0 */
} mldsa_x509sign_req;

/* ---- status: the first rule broken, tested in this order ---------------------------------------------------------------------------------
 * Codes 1 ... 3 are MLDSA_X509_RANGE, _DER and _ALG of mldsa_x509.h; the codes below are disjoint from its 4 ... 7. */
#define MLDSA_X509SIGN_ENTRY 8  /* set none of MLDSA_44 / 65 / 87, a flag bit other than bit 0, or reserved nonzero */
#define MLDSA_X509SIGN_KEY 9    /* key >= n_keys of its set (a set with n_keys = 0 is not served) */
/*      MLDSA_X509_RANGE 1         rec's test off <= blob_len && len <= blob_len - off fails, or len < 2; with the RND flag,
                                   [rnd_off, rnd_off + 32) does not lie inside the blob */
#define MLDSA_X509SIGN_LONG 10  /* len > 65517 - SIG_LEN (63097 / 62208 / 60890): the outer header would need three length bytes */
/*      MLDSA_X509_DER 2           the strict walk fails (below) */
/*      MLDSA_X509_ALG 3           the TBS's inner `signature` AlgorithmIdentifier content is not exactly the 11 bytes
                                   06 09 60 86 48 01 65 03 04 03 {11|12|13} of the entry's set (parameters absent) */
#define MLDSA_X509SIGN_SPACE 11 /* the certificate's range does not lie inside [0, out_len) */
/* For a refused certificate no byte of the blob beyond the header reads of its walk is read, and no byte of `out` is written.
 * Offsets only grow, so once one certificate is SPACE every later accepted one is too. */

/* ---- the frame -----------------------------------------------------------------------------------------------------------------------------
 *     30 82 hh ll | TBS | 30 0B 06 09 60 86 48 01 65 03 04 03 {11|12|13} | 03 82 hh ll 00 | SIG_LEN bytes
 * The BIT STRING's length is SIG_LEN + 1 (0x0975, 0x0CEE, 0x1214); cert_len = len + 22 + SIG_LEN; the hole lies at cert_off + len + 22.
 * The outer header is always the two-byte long form: its content is never below 2438 bytes and LONG keeps it at most 65535.
 * Certificates are laid out in input order, back to back from out + 0, by a stable exclusive scan of cert_len: a refused certificate
 * takes no room.  `out` -- uint8[out_len] in device memory -- has NO alignment requirement and must not overlap the blob: the frame is
 * written before the signer reads the TBS from the blob.
 *
 * ---- the walk (fips204_amd/x509sign/x509sign_plan.h: one function, walk_tbs, which the kernels and a stand-alone host program both run)
 * read_tlv is mldsa_x509.h's.  The TBS is a 0x30 TLV filling [0, len) exactly (trailing bytes are DER).  Inside it, at the very
 * positions step 3 of mldsa_x509.h's walk reads: an optional 0xA0, 0x02, 0x30 the inner algorithm, 0x30 the issuer, 0x30 the validity,
 * 0x30 the subject, 0x30 the subjectPublicKeyInfo, whose content is 0x30 then 0x03 ending exactly at its end.  Whatever follows the
 * SPKI inside the TBS is not walked.  At most 10 read_tlv steps; no loop depends on data for its bound; no byte at or behind len is
 * read.  Only then is the inner algorithm compared with the entry's set (ALG). */

/* ---- output, per certificate --------------------------------------------------------------------------------------------------------------
 *   out_certs[i]  mldsa_x509_cert {off, len, issuer}: the finished certificate's range in `out` and the entry's issuer; {0, 0,
 *                 MLDSA_X509_NO_ISSUER} when the certificate is refused.  8-byte aligned.
 *   ops[i]        mldsa_recsign_op: msg_off / msg_len = the TBS in the BLOB, ctx_off = 0, ctx_len = 0, rnd_off / flags = the entry's,
 *                 sig_off = the hole in `out`, key and set = the entry's, reserved = 0; all zero when refused.  8-byte aligned.
 *   status[i]     uint8: MLDSA_X509_OK or the first rule broken.
 *   totals        one struct in device memory, 8-byte aligned. */
typedef struct {
    uint64_t accepted;  /* certificates with status MLDSA_X509_OK */
    uint64_t refused;   /* all others: accepted + refused = n */
    uint64_t out_bytes; /* what all certificates that pass every rule but SPACE need back to back: a caller whose `out` was too small
                           learns the need here */
} mldsa_x509sign_totals;

int mldsa_x509sign_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_x509sign_last_error(void);

/* ---- host helpers ---------------------------------------------------------------------------------------------------------------------------
 * cert_len of a TBS of tbs_len bytes under `set`: tbs_len + 22 + SIG_LEN; 0 for an unknown set or a LONG length. */
size_t mldsa_x509sign_cert_len(int set, size_t tbs_len);
/* An `out` no batch of n TBSs of tbs_bytes bytes in all can outgrow: tbs_bytes + n (22 + 4627); 0 when n exceeds
 * MLDSA_X509SIGN_MAX_CERTS or the size does not fit. */
size_t mldsa_x509sign_out_bytes_max(size_t n, uint64_t tbs_bytes);
/* The plan's working memory.  With R(x) = x rounded up to a multiple of 256 and B = ceil(n / MLDSA_X509SIGN_SCAN_BLOCK) workgroups:
 *   R(16 B) + R(4 n)            two 64-bit sums per workgroup (certificate bytes, accepted requests); cert_len of every request
 * 0 for n > MLDSA_X509SIGN_MAX_CERTS. */
size_t mldsa_x509sign_plan_bytes(size_t n);

/* ---- 1. the plan: status, place and op of every certificate ---------------------------------------------------------------------------------
 *   n_keys   HOST array of three: the rows of the key tables in class order 44 / 65 / 87, as mldsa_recsign_plan takes them.
 *   plan     mldsa_x509sign_plan_bytes(n) bytes, 256-byte aligned, caller-owned, used in stream order.
 * Asynchronous on `stream`, never waits for the host: three launches ordered by the kernel boundaries.  k_x509sign_check (one request
 *   per lane, MLDSA_X509SIGN_SCAN_BLOCK per workgroup, as k_x509_parse) applies the rules up to ALG and writes cert_len (0 when refused)
 *   and two sums per workgroup; k_x509sign_offsets (one wave) turns the sums into exclusive prefixes and writes the totals;
 *   k_x509sign_apply scans inside each workgroup, runs the SPACE rule and writes out_certs, ops and status.  No kernel waits on another
 *   workgroup and every loop runs to a count the host passed.  `out` is not touched.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, reqs, n_keys, out_certs, ops, status, totals or plan, NULL blob with blob_len > 0,
 *   reqs, out_certs, ops or totals not 8-byte aligned, plan not 256-byte aligned or smaller than mldsa_x509sign_plan_bytes, an n_keys
 *   above UINT32_MAX, n > MLDSA_X509SIGN_MAX_CERTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_x509sign_plan(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509sign_req *reqs, size_t n,
                        const size_t *n_keys /* host [3] */, uint64_t out_len, mldsa_x509_cert *out_certs, mldsa_recsign_op *ops,
                        uint8_t *status, mldsa_x509sign_totals *totals, void *plan, size_t plan_bytes, void *stream);

/* ---- 2. the frame: every accepted certificate but its signature -------------------------------------------------------------------------------
 * For every certificate with status[i] == MLDSA_X509_OK: the 4 header bytes, the TBS copied from the blob, the 18 bytes behind it.
 * The SIG_LEN bytes of the hole are not touched, and no byte outside the certificate's range.
 * One launch, k_x509sign_frame: one certificate per wave.  It re-derives nothing from the blob: it reads the request, out_certs[i] and
 *   status[i], and it checks both ranges again -- the TBS against blob_len, the certificate against out_len, and out_certs[i].len
 *   against the request's len and set -- so a row that was tampered with writes nothing outside `out` and reads nothing outside the
 *   blob: such a certificate is skipped.  The TBS is copied by the plan of fips204_amd/rec/rec_plan.h: bytes one by one up to the
 *   destination's first 16-byte boundary, then aligned 16-byte loads funnel-shifted in registers to aligned 16-byte stores, then the
 *   rest one by one.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, reqs, out_certs or status, NULL blob with blob_len > 0, NULL out with out_len > 0, reqs or
 *   out_certs not 8-byte aligned, `out` overlapping the blob (checked from the two pointer ranges), n > MLDSA_X509SIGN_MAX_CERTS.  n = 0 returns
 *   MLDSA_OK without a context and touches nothing. */
int mldsa_x509sign_frame(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509sign_req *reqs, size_t n, uint8_t *out,
                         uint64_t out_len, const mldsa_x509_cert *out_certs, const uint8_t *status, void *stream);

/* ---- 3. both on `stream` ------------------------------------------------------------------------------------------------------------------------
 * mldsa_x509sign_plan then mldsa_x509sign_frame; the argument errors of both, before anything is launched.
 *
 * Cost, from byte counts (an expectation): per certificate about 10 dependent header reads, one 32-byte request read three times, 16 +
 *   48 + 1 bytes of rows written, and the frame: len bytes read, len + 22 written -- against the signing call behind it, which moves
 *   the same TBS once more and SIG_LEN bytes twice and spends milliseconds on arithmetic.  The framing should cost a few per cent of the
 *   signing call, as mldsa_x509.h's walk does of verification.
 * Measured on an MI355X, 65 536 TBSs in the depth-3 shape of tools/bench_x509.py, 5 mod 16 bytes apart, 1 024 keys per set
 *   (profiles/x509sign_bench.jsonl; medians of alternating runs in one process; "copy" is a device-to-device copy that moves the bytes
 *   the frame kernel moves, in the same run):
 *                                                   ML-DSA-44   ML-DSA-65   ML-DSA-87   even three-way mix
 *     this call                                     0.096 ms    0.108 ms    0.121 ms    0.111 ms     (1.5 ... 1.8 ns per certificate)
 *     this call / mldsa_recsign_sign on its ops     0.018       0.014       0.012       0.010        (5.46 / 7.77 / 9.99 / 10.58 ms)
 *     both calls / mldsa_recsign_sign alone         1.011       1.013       1.009       1.012
 *     k_x509sign_frame, read + written              2.53 TB/s   3.13 TB/s   3.55 TB/s   3.14 TB/s
 *     copy                                          4.18 TB/s   4.32 TB/s   4.47 TB/s   4.36 TB/s
 *     Python framing + upload + mldsa_recsign_sign
 *       / both calls                                33          25          26          19           (2.6 ... 3.8 us per certificate framed)
 *   The frame kernel's rate grows with the TBS: a certificate is one to three 1 KiB steps of its wave, so the wave's fixed cost shows. */
int mldsa_x509sign_issue_ops(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509sign_req *reqs, size_t n,
                             const size_t *n_keys /* host [3] */, uint8_t *out, uint64_t out_len, mldsa_x509_cert *out_certs,
                             mldsa_recsign_op *ops, uint8_t *status, mldsa_x509sign_totals *totals, void *plan, size_t plan_bytes,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_X509SIGN_H */
