/* mldsa_x509.h -- the signature leg of X.509 path validation on the device: certificates in a blob to mldsa_rec_op descriptors
 * (libmldsa_x509.so).
 *
 * A service that verifies ML-DSA certificates (the IETF profile cited in mldsa_seed.h) holds a buffer of DER certificates, often
 * already on the device, and for each of them the index of the certificate that issued it.  mldsa_rec_verify (mldsa_rec.h) verifies
 * from such a buffer, given one 40-byte descriptor per signature with the offsets of key, signature and message; for a certificate
 * those offsets come from a DER walk, and the key of one certificate lies inside another.  This library makes that walk on the
 * device: it reads each certificate's structure, checks the algorithm identifiers, chains issuer and subject names byte for byte and
 * writes one mldsa_rec_op per certificate -- key = the issuer's subject key, message = the certificate's own TBSCertificate, pure
 * mode with an empty context, which is what the profile prescribes.  Any mix of ML-DSA-44 / 65 / 87; the host takes no part.
 *
 * A C caller verifies a batch of chains with two calls on one stream, the way mldsa_mus.h describes verify_host_streamed:
 *     mldsa_x509_ops(ctx, blob, blob_len, certs, n, MLDSA_X509_CHECK_NAMES, fields, ops, status, stream);
 *     mldsa_rec_verify(ctx, MLDSA_MODE_PURE, blob, blob_len, ops, n, ok, scratch, scratch_bytes, NULL, stream);
 * Certificate i is valid under its issuer's key where status[i] == MLDSA_X509_OK and ok[i] == 1; every other certificate's op is all
 * zero, which mldsa_rec_verify refuses (set = 0) without reading a byte, so its ok[i] is 0.  Any call behind rec's pack seam
 * (mldsa_rec_plan + mldsa_rec_pack) takes the same ops.  MlDsaCertificates.verify_device of the Python package is these two calls.
 *
 * IN SCOPE: the strict DER structure of the fields walked, the algorithm identifiers, issuer / subject name chaining byte for byte,
 * the signature under the issuer's subject key.
 * NOT IN SCOPE, and not looked at: validity dates, extensions, basicConstraints, key usage, revocation; PEM; any signature algorithm
 * other than ML-DSA (such a certificate gets MLDSA_X509_ALG).  A caller that needs them checks them elsewhere.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only, and takes from mldsa_rec.h the descriptor
 * type alone -- it neither links nor calls libmldsa_rec.so.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.
 *
 * Public data only: certificates.  Nothing here is cleared.
 */
#ifndef MLDSA_X509_H
#define MLDSA_X509_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_rec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_X509_ABI_VERSION 1
/* most certificates of one call: keeps every issuer index apart from MLDSA_X509_NO_ISSUER */
#define MLDSA_X509_MAX_CERTS (1u << 30)

/* ---- input: one per certificate, a device array, 8-byte aligned, 16 bytes each ----------------------------------------------------------
 * [off, off + len) of the blob -- uint8[blob_len] in device memory, NO alignment requirement -- is one DER Certificate.  `issuer` is
 * the index, in the same array, of the certificate whose subject key signs this one: a self-signed root names itself, many
 * certificates may name one issuer, ranges may overlap or coincide.  Blob and array are untrusted. */
typedef struct {
    uint64_t off;
    uint32_t len;
    uint32_t issuer;
} mldsa_x509_cert;
/* parse only: the certificate is a key source, its own signature is not verified */
#define MLDSA_X509_NO_ISSUER 0xFFFFFFFFu

/* ---- what the walk finds: one row per certificate, a device array, 8-byte aligned, 56 bytes each ----------------------------------------
 *   tbs_off, tbs_len          the whole TBSCertificate TLV: the message
 *   sig_off                   the first byte behind the unused-bits byte of the signatureValue BIT STRING; sig_set its parameter set
 *   key_off                   the first byte behind the unused-bits byte of the subjectPublicKey BIT STRING; key_set its parameter set
 *   issuer_off, issuer_len    the whole issuer Name TLV;  subject_off, subject_len the whole subject Name TLV
 * Offsets are absolute blob offsets.  sig_set and key_set are MLDSA_44 / MLDSA_65 / MLDSA_87 or 0.
 * A status of RANGE or DER leaves every other field 0.  sig_off and sig_set are nonzero only where the walk's status is OK.  key_off and
 * key_set are nonzero only where the subject key is an ML-DSA key: key_set = 0 is NOT an error of the certificate (a leaf may carry any
 * key), it only makes the certificate useless as an issuer.  `status` is the walk's: OK, RANGE, DER, ALG or SIG. */
typedef struct {
    uint64_t tbs_off, sig_off, key_off, issuer_off, subject_off;
    uint32_t tbs_len, issuer_len, subject_len;
    uint8_t sig_set, key_set, status, reserved;
} mldsa_x509_fields;

/* ---- status: the first rule broken, tested in this order ---------------------------------------------------------------------------------
 * ISSUER: issuer >= n and not MLDSA_X509_NO_ISSUER; the issuer's own status is RANGE or DER; the issuer's key_set is 0 or differs from
 * this certificate's sig_set.  An issuer whose own status is ALG or SIG -- a root signed with something else -- still lends its key. */
#define MLDSA_X509_OK 0         /* accepted: ops[i] describes the signature */
#define MLDSA_X509_RANGE 1      /* [off, off + len) not inside [0, blob_len) -- rec's test, off <= blob_len && len <= blob_len - off -- or len < 2 */
#define MLDSA_X509_DER 2        /* a structural failure anywhere on the walked path (below) */
#define MLDSA_X509_ALG 3        /* the outer signatureAlgorithm's content is not exactly 06 09 60 86 48 01 65 03 04 03 {11|12|13}
                                   (id-ml-dsa-44 / -65 / -87, parameters absent), or the TBS's inner `signature` TLV is not byte for byte
                                   the outer one */
#define MLDSA_X509_SIG 4        /* signatureValue's content is not 1 + SIG_LEN of the set long, or its unused-bits byte is not 0 */
#define MLDSA_X509_ISSUER 5     /* see above */
#define MLDSA_X509_NAME 6       /* only with MLDSA_X509_CHECK_NAMES: this certificate's issuer Name TLV differs from the issuer's subject
                                   Name TLV, in length or in any byte */
#define MLDSA_X509_PARSE_ONLY 7 /* issuer == MLDSA_X509_NO_ISSUER and the certificate is otherwise OK */

/* flags of mldsa_x509_link and mldsa_x509_ops */
#define MLDSA_X509_CHECK_NAMES 1u

/* ---- the walk (fips204_amd/x509/x509_plan.h: one function, which the kernels and a stand-alone host program both run) -------------------
 * read_tlv(pos, end) needs pos + 2 <= end and refuses: a tag with (tag & 0x1F) == 0x1F; the length byte 0x80; length bytes above 0x84; a
 *   long form whose first length byte is 0, or whose value would fit a shorter form (0x81 with a value < 128); length bytes or content
 *   that overrun `end`.  Every refusal is DER.
 *   1. The Certificate: tag 0x30, filling [0, len) exactly (trailing bytes are DER).
 *   2. Its content: TBSCertificate 0x30, AlgorithmIdentifier 0x30, BIT STRING 0x03, ending exactly at the Certificate's end.
 *   3. Inside the TBS, in this order: an optional 0xA0 (skipped), 0x02 (skipped), 0x30 the inner signature AlgorithmIdentifier, 0x30 the
 *      issuer (recorded), 0x30 the validity (skipped), 0x30 the subject (recorded), 0x30 the subjectPublicKeyInfo, whose content is 0x30
 *      then 0x03 ending exactly at its end.  Whatever follows the SPKI inside the TBS -- unique IDs, extensions -- is not walked.
 *   A wrong tag at any of these positions is DER.  Only then are the algorithm identifiers compared (ALG), then the signature's length
 *   and unused-bits byte (SIG).  key_set is nonzero only when the SPKI algorithm's content is exactly one of the three 11-byte OIDs and
 *   the key BIT STRING is 1 + PK_LEN long with unused-bits byte 0.
 * A fixed sequence of at most 14 read_tlv steps: no loop depends on data for its bound.  No byte outside [off, off + len) is ever read,
 * and therefore none outside the blob. */

int mldsa_x509_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_x509_last_error(void);

/* fields[i] = the walk of certificate i.  One launch, k_x509_parse: one certificate per lane, 256 lanes per workgroup -- the walk is a
 * chain of dependent small loads, so what scales is the number of chains in flight.  Asynchronous on `stream`, never waits for the host.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs or fields, NULL blob with blob_len > 0, certs or fields not 8-byte aligned,
 *   n > MLDSA_X509_MAX_CERTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_x509_parse(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, size_t n,
                     mldsa_x509_fields *fields, void *stream);

/* ops[i], status[i] from the rows mldsa_x509_parse wrote.  For an accepted certificate (status OK)
 *     pk_off = the issuer's key_off, sig_off = its own, msg_off / msg_len = its own TBS, ctx_off = 0, ctx_len = 0, set = its own sig_set,
 *     reserved = 0;
 * for every other certificate the op is all zero.  One launch, k_x509_link: one certificate per wave.  Lane 0 decides from the
 * certificate's row and its issuer's row -- never the issuer's DER again -- and with MLDSA_X509_CHECK_NAMES the wave compares the two
 * Name TLVs 64 bytes per step.  `fields` is untrusted like everything else: a Name range of a row that does not lie inside the blob is
 * not followed and counts as a mismatch, and mldsa_rec_verify checks every range of an op itself.
 * Argument errors (MLDSA_ERR_PARAM): as above, and NULL ops or status, ops not 8-byte aligned, an unknown flag bit. */
int mldsa_x509_link(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs,
                    const mldsa_x509_fields *fields, size_t n, unsigned flags, mldsa_rec_op *ops, uint8_t *status, void *stream);

/* mldsa_x509_parse then mldsa_x509_link on `stream`: fields is written on the way and is the call's only working memory.
 *
 * Cost, from counts (an expectation): per certificate about 14 dependent header reads of at most 6 bytes, one 56-byte row, one 40-byte
 *   op and two Names, against the roughly 4 - 7 KB that rec's pack then moves for the same certificate.
 * Measured on an MI355X, 65 536 validly signed certificates in chains of depth 3, 5 mod 16 bytes apart (profiles/x509_bench.jsonl;
 *   medians of alternating runs in one process):
 *                                               ML-DSA-44   ML-DSA-65   ML-DSA-87   even three-way mix
 *     this call                                 0.065 ms    0.064 ms    0.066 ms    0.069 ms     (about 1 ns per certificate)
 *     this call / mldsa_rec_verify on its ops   0.034       0.022       0.016       0.017        (1.90 / 2.85 / 4.15 / 4.08 ms)
 *     both calls / mldsa_rec_verify alone       1.030       1.023       1.015       1.017
 *     a plain Python walk on the host
 *       / this call                             5 800       6 200       5 800       5 100        (5.4 ... 6.0 us per certificate)
 *   Rec's own plan + pack is 7 - 16 % of its call; the walk in front of it adds 1.6 - 3.4 %. */
int mldsa_x509_ops(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, size_t n, unsigned flags,
                   mldsa_x509_fields *fields, mldsa_rec_op *ops, uint8_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_X509_H */
