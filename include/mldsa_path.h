/* mldsa_path.h -- the last leg of X.509 path validation on the device: validity dates, the CA constraints of the extensions and one
 * verdict per certificate for its whole chain (libmldsa_path.so).
 *
 * mldsa_x509.h puts the signature under the issuer's key and Name chaining on the device, mldsa_crl.h revocation; both leave validity
 * dates, extensions, basicConstraints and key usage to the caller, and neither folds the per-certificate bytes (status, ok, revocation)
 * along a chain.  That fold is what turns "this signature verifies" into "this certificate may be trusted".  This library computes it:
 *   1. the two Times of every certificate's validity and of every CRL's thisUpdate / nextUpdate, as seconds since 1970;
 *   2. the walk behind the subjectPublicKeyInfo: version, unique IDs, every extension's frame, basicConstraints, keyUsage, and the
 *      refusal of critical extensions it does not understand;
 *   3. the climb from every certificate to a trust anchor, which stops at the first certificate on the way that breaks a rule.
 *
 * A C caller validates a batch with these calls on one stream (certs, fields, the CRL arrays: mldsa_x509.h, mldsa_crl.h):
 *     mldsa_x509_ops(ctx, blob, blob_len, certs, n, MLDSA_X509_CHECK_NAMES, fields, cert_ops, cert_status, stream);
 *     mldsa_rec_verify(ctx, MLDSA_MODE_PURE, blob, blob_len, cert_ops, n, cert_ok, ...);
 *     mldsa_path_parse(ctx, blob, blob_len, certs, n, 0, policy, stream);
 *     mldsa_crl_ops(...);  mldsa_rec_verify(... crl_ops, n_crls, crl_ok ...);  mldsa_crl_table(...);
 *     mldsa_path_crl_times(ctx, blob, blob_len, crl_fields, crl_status, crl_ok, n_crls, now, 0, this_s, next_s, time_status, fresh_ok, stream);
 *     mldsa_crl_check(... crl_status, fresh_ok, ... revocation, stream);        (fresh_ok in the place of crl_ok)
 *     mldsa_path_chain(ctx, certs, policy, cert_status, cert_ok, revocation, anchor, n, now, 0, results, scratch, scratch_bytes, stream);
 * Certificate i may be trusted at `now` where results[i].verdict == MLDSA_PATH_TRUSTED.  MlDsaPathValidator.validate of the Python
 * package is these calls.
 *
 * IN SCOPE: the strict DER structure of the fields walked, the version rule, both validity Times, the frame of every extension,
 * basicConstraints (cA, pathLenConstraint), keyUsage (keyCertSign), unknown critical extensions, the freshness of a CRL, and the climb.
 * NOT IN SCOPE, and not looked at:
 *   - self-issued certificates are not exempt from pathLen: every certificate between the leaf and the one that carries the
 *     constraint counts;
 *   - name and policy constraints (critical ones are refused as unknown, others ignored);
 *   - extended key usage;
 *   - AKI / SKI: the issuer of a certificate is the one its caller names;
 *   - cRLSign on CRL issuers;
 *   - delta and indirect CRLs;
 *   - PEM;
 *   - RFC 5280's rule that dates before 2050 use UTCTime is not enforced: either form is taken at any date;
 *   - the host-memory, group and batcher forms of the other libraries;
 *   - the C++ / Rust mirrors.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.  From mldsa_x509.h, mldsa_crl.h and
 * mldsa_rec.h it takes types and codes alone -- it neither links nor calls libmldsa_x509.so, libmldsa_crl.so or libmldsa_rec.so.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.  Every
 * call is asynchronous on `stream` and never waits for the host.  `now` and every time are int64 seconds since 1970-01-01T00:00:00Z.
 *
 * Public data only: certificates and CRLs.  Nothing here is cleared for secrecy.
 */
#ifndef MLDSA_PATH_H
#define MLDSA_PATH_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_rec.h"
#include "mldsa_x509.h"
#include "mldsa_crl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_PATH_ABI_VERSION 1
#define MLDSA_PATH_MAX_CERTS MLDSA_X509_MAX_CERTS
/* extensions walked per certificate: the bound of the one loop of the walk */
#define MLDSA_PATH_MAX_EXTS 32
/* certificates between a certificate and its trust anchor, the anchor included: the bound of the climb */
#define MLDSA_PATH_MAX_DEPTH 16
/* path_len: no pathLenConstraint */
#define MLDSA_PATH_NO_PATH_LEN 0xFFFFFFFFu

/* flags.  Each call takes its own and refuses every other bit. */
#define MLDSA_PATH_ALLOW_UNKNOWN_CRITICAL 1u /* mldsa_path_parse: an unknown critical extension is recorded and not refused */
#define MLDSA_PATH_REQUIRE_NEXT_UPDATE 2u    /* mldsa_path_crl_times: a CRL without nextUpdate is STALE */
#define MLDSA_PATH_ALLOW_NO_CRL 4u           /* mldsa_path_chain: revocation[i] == MLDSA_CRL_NO_CRL breaks no rule */

/* ---- what the walk finds: one row per certificate, a device array, 8-byte aligned, 48 bytes each -----------------------------------------
 *   not_before, not_after   the validity, in seconds; 0, 0 where the status is TIME
 *   ext_off, ext_len        the CONTENT of the Extensions SEQUENCE inside [3], ext_off an absolute blob offset; 0, 0 where absent
 *   crit_off                the first extension TLV (its 0x30) that is marked critical and is neither basicConstraints nor keyUsage, an
 *                           absolute blob offset; 0: none
 *   path_len                pathLenConstraint, MLDSA_PATH_NO_PATH_LEN where absent
 *   key_usage               bit i = KeyUsage bit i of RFC 5280 (digitalSignature = 0, keyCertSign = 5, cRLSign = 6); 0 without keyUsage
 *   flags                   MLDSA_PATH_V3, _HAS_BC, _IS_CA, _HAS_KU (below)
 *   n_ext                   extensions walked, at most MLDSA_PATH_MAX_EXTS
 * A status of RANGE or DER leaves every other field 0.  Under every other status the fields hold what was read by the rules: a
 * basicConstraints or keyUsage whose value is refused (EXT) is not recorded, a second one neither. */
typedef struct {
    int64_t not_before, not_after;
    uint64_t ext_off, crit_off;
    uint32_t ext_len, path_len;
    uint16_t key_usage;
    uint8_t flags, n_ext, status, reserved[3];
} mldsa_path_fields;

#define MLDSA_PATH_V3 1u     /* the version is v3 */
#define MLDSA_PATH_HAS_BC 2u /* a well-formed basicConstraints */
#define MLDSA_PATH_IS_CA 4u  /* ... whose cA is TRUE */
#define MLDSA_PATH_HAS_KU 8u /* a well-formed keyUsage */

/* ---- status of the walk: the first class broken, in this order: RANGE, DER, VERSION, TIME, EXT, CRITICAL ---------------------------------
 * 0 ... 2 are mldsa_x509.h's, with the same meaning: MLDSA_X509_OK, _RANGE, _DER.  The whole path is walked for its structure first, so
 * a DER failure anywhere outranks a VERSION failure in front of it.  The new codes are disjoint from every code of mldsa_x509.h,
 * mldsa_x509sign.h, mldsa_csr.h and mldsa_crl.h (0 ... 21). */
#define MLDSA_PATH_VERSION 22  /* [0] whose content is not exactly 02 01 01 or 02 01 02 (the explicit default 02 01 00 included); a unique
                                  ID in a v1 certificate; extensions in a v1 or v2 certificate */
#define MLDSA_PATH_TIME 23     /* the validity's content is not exactly two Times that parse_time accepts */
#define MLDSA_PATH_EXT 24      /* an empty Extensions SEQUENCE; more than MLDSA_PATH_MAX_EXTS extensions; a critical BOOLEAN that is not
                                  01 01 FF; a basicConstraints or keyUsage value that breaks its rule (below); either of the two twice */
#define MLDSA_PATH_CRITICAL 25 /* a critical extension that is neither basicConstraints nor keyUsage, without
                                  MLDSA_PATH_ALLOW_UNKNOWN_CRITICAL */

/* ---- the rules (fips204_amd/path/path_plan.h: constexpr functions on a fetch functor, which the kernels and a stand-alone host program
 * both run; read_tlv is mldsa_x509.h's, with every refusal it lists) -------------------------------------------------------------------------
 * parse_time, one Time TLV:
 *   tag 0x17 with exactly 13 content bytes YYMMDDhhmmssZ, YY < 50 meaning 20YY and else 19YY; tag 0x18 with exactly 15 content bytes
 *   YYYYMMDDhhmmssZ, year 0001 ... 9999.  Refused: any other tag or length, a non-digit, month 0 or above 12, day 0 or past the month's
 *   end (29 February only where y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)), hour above 23, minute or second above 59, a last byte
 *   that is not `Z`.  The seconds are counted in the proleptic Gregorian calendar by days-from-civil arithmetic: no table is indexed
 *   by data.  Leap seconds do not exist (second 60 is refused).
 * walk_policy, one certificate: a fixed sequence of at most 20 read_tlv steps and one loop over the extensions, bounded by
 * MLDSA_PATH_MAX_EXTS, of at most 4 steps each and 3 more for basicConstraints or keyUsage:
 *   1. The steps of mldsa_x509.h's walk down to the subjectPublicKeyInfo, with the same DER refusals (so DER here wherever DER there).
 *   2. Version: [0] absent means v1; present, its content is exactly 02 01 01 (v2) or 02 01 02 (v3), else VERSION.
 *   3. Validity: exactly two Times by parse_time, else TIME.
 *   4. Behind the SPKI, in this order and ending exactly at the TBS's end: an optional 0x81 and an optional 0x82 unique ID (v2 or v3,
 *      else VERSION); an optional 0xA3 whose content is one 0x30 filling it exactly (v3, else VERSION).  A wrong tag or trailing bytes
 *      is DER.
 *   5. Each extension: 0x30 holding 0x06, an optional 0x01, then 0x04 ending exactly at the extension's end; a wrong tag or trailing
 *      bytes is DER.  The BOOLEAN is 01 01 FF, else EXT (DER forbids the default FALSE).
 *   6. basicConstraints (OID 55 1D 13): the value is one 0x30 filling it exactly that holds an optional 01 01 FF, then an optional 0x02
 *      pathLenConstraint of 1 ... 4 content bytes, non-negative and minimally encoded, and ends exactly; pathLenConstraint without cA
 *      is refused.  keyUsage (55 1D 0F): the value is one 0x03 filling it exactly, of 2 or 3 content bytes; the unused-bits byte is
 *      0 ... 7, the unused bits are zero and the lowest used bit is one (DER's named-bit-list rule, which also makes one bit at least
 *      set).  Every refusal inside one of these two values is EXT.
 *   7. Any other extension with the BOOLEAN is counted; the first is recorded in crit_off.
 * No byte outside [off, off + len) of a certificate is ever read. */

/* ---- the verdict of the climb: one row per certificate, a device array, 8-byte aligned, 8 bytes ------------------------------------------
 * `where` is the certificate at which the climb stopped -- the anchor, or the certificate that broke the rule --, `depth` the number of
 * steps from certificate i to it. */
typedef struct {
    uint32_t where;
    uint8_t verdict, depth, reserved[2];
} mldsa_path_result;

#define MLDSA_PATH_TRUSTED 0
/* the rules a certificate breaks for itself, tested in this order */
#define MLDSA_PATH_CERT 1       /* cert_status != 0 */
#define MLDSA_PATH_SIG 2        /* cert_ok == 0 */
#define MLDSA_PATH_POLICY 3     /* the policy row's status is not OK */
#define MLDSA_PATH_NOT_YET 4    /* now < not_before */
#define MLDSA_PATH_EXPIRED 5    /* now > not_after */
#define MLDSA_PATH_REVOKED 6    /* revocation == MLDSA_CRL_REVOKED */
#define MLDSA_PATH_REVOCATION 7 /* any other value that is not MLDSA_CRL_GOOD; MLDSA_CRL_NO_CRL passes with MLDSA_PATH_ALLOW_NO_CRL */
/* the rules it breaks as somebody's issuer, tested in this order */
#define MLDSA_PATH_NOT_CA 8     /* not v3, no basicConstraints, or cA not TRUE */
#define MLDSA_PATH_KEY_USAGE 9  /* keyUsage present and keyCertSign clear */
#define MLDSA_PATH_PATH_LEN 10  /* more certificates below it on this path than its pathLenConstraint allows */
/* the climb's own ends */
#define MLDSA_PATH_NO_ANCHOR 11 /* the issuer is MLDSA_X509_NO_ISSUER, >= n or the certificate itself, and it is no anchor */
#define MLDSA_PATH_DEPTH 12     /* no anchor within MLDSA_PATH_MAX_DEPTH steps: a cycle ends here too */

/* time_status of mldsa_path_crl_times, the rules tested in this order */
#define MLDSA_PATH_CRL_FRESH 0
#define MLDSA_PATH_CRL_REFUSED 1 /* crl_status[c] != 0 or the row's own status != 0: nothing of the row is followed */
#define MLDSA_PATH_CRL_TIME 2    /* this_off (or a nonzero next_off) with fewer than two bytes inside the blob, or a Time refused */
#define MLDSA_PATH_CRL_NOT_YET 3 /* now < thisUpdate */
#define MLDSA_PATH_CRL_STALE 4   /* now > nextUpdate; or no nextUpdate, with MLDSA_PATH_REQUIRE_NEXT_UPDATE */

int mldsa_path_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_path_last_error(void);

/* working memory of mldsa_path_chain: R(8 n) bytes, R(x) = x rounded up to a multiple of 256: one 8-byte node per certificate.  0 for
 * n > MLDSA_PATH_MAX_CERTS. */
size_t mldsa_path_scratch_bytes(size_t n);

/* The generic seam of parse_time: seconds[i], status[i] of the Time TLV at blob offset offs[i], bounded by the blob's end.  status is
 * MLDSA_X509_OK, MLDSA_X509_RANGE (fewer than two bytes from offs[i] to the blob's end) or MLDSA_PATH_TIME (a TLV that overruns the
 * blob's end included); seconds[i] is 0 where it is not OK.  One launch, k_path_times, one Time per lane.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, offs, seconds or status, NULL blob with blob_len > 0, offs or seconds not 8-byte aligned,
 *   n > MLDSA_PATH_MAX_CERTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_path_times(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const uint64_t *offs, size_t n, int64_t *seconds,
                     uint8_t *status, void *stream);

/* fields[i] = walk_policy of certificate i.  One launch, k_path_parse: one certificate per lane, 256 lanes per workgroup, as
 * k_x509_parse.  flags: MLDSA_PATH_ALLOW_UNKNOWN_CRITICAL.
 *
 * Cost, from counts (an expectation): per certificate about 20 dependent header reads, two Times of 13 - 15 bytes, per extension 3 - 4
 *   more dependent reads, and one 48-byte row: a chain about twice as long as mldsa_x509_parse's for a certificate with three
 *   extensions, and lanes of one wave that leave the extension loop at different counts wait for the longest.
 * Measured: not measured (tools/bench_path.py writes profiles/path_bench.jsonl; the table goes here once that file exists).
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs or fields, NULL blob with blob_len > 0, certs or fields not 8-byte aligned,
 *   n > MLDSA_PATH_MAX_CERTS, an unknown flag bit.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_path_parse(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, size_t n, unsigned flags,
                     mldsa_path_fields *fields, void *stream);

/* The freshness of every CRL at `now`, from this_off / next_off of the rows mldsa_crl_ops wrote; crl_status is its status array, crl_ok
 * (may be NULL) mldsa_rec_verify's verdicts on its ops.  this_s[c], next_s[c]: the two Times in seconds, 0 where not read or absent;
 * time_status[c] as listed above; fresh_ok[c] = (crl_ok == NULL || crl_ok[c] != 0) && time_status[c] == MLDSA_PATH_CRL_FRESH, made to
 * be passed as the crl_ok argument of mldsa_crl_check, which then answers MLDSA_CRL_CRL_REFUSED for every certificate under a CRL
 * that is not fresh.  The rows are untrusted: an offset that does not lie in the blob is not followed.  One launch, k_path_crl_times,
 * one CRL per lane.  flags: MLDSA_PATH_REQUIRE_NEXT_UPDATE.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, crl_fields, crl_status, this_s, next_s, time_status or fresh_ok, NULL blob with
 *   blob_len > 0, crl_fields, this_s or next_s not 8-byte aligned, n_crls > MLDSA_CRL_MAX_CRLS, an unknown flag bit.  n_crls = 0
 *   returns MLDSA_OK without a context and touches nothing. */
int mldsa_path_crl_times(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_crl_fields *crl_fields,
                         const uint8_t *crl_status, const uint8_t *crl_ok, size_t n_crls, int64_t now, unsigned flags, int64_t *this_s,
                         int64_t *next_s, uint8_t *time_status, uint8_t *fresh_ok, void *stream);

/* results[i] for every certificate: the verdict of its chain at `now`.  certs gives every certificate's issuer, policy is
 * mldsa_path_parse's rows, cert_status and cert_ok are mldsa_x509_ops' status and mldsa_rec_verify's verdicts, revocation (may be NULL:
 * revocation is not checked) is mldsa_crl_check's answers, anchor[i] != 0 marks a trust anchor.  flags: MLDSA_PATH_ALLOW_NO_CRL.
 * Two launches, ordered by the kernel boundary alone:
 *   k_path_node   one certificate per lane: an 8-byte node in scratch, {uint32 issuer; uint8 own; uint8 as_issuer; uint8 path_len;
 *                 uint8 anchor} -- own: the first rule of CERT ... REVOCATION the certificate breaks for itself, or 0; as_issuer: NOT_CA,
 *                 else KEY_USAGE, else 0; path_len saturated to 254, 255 = none.
 *   k_path_climb  one certificate per lane: a_0 = i, a_(k+1) = issuer(a_k).  For k = 0, 1, ...:
 *                   1. anchor[a_k]: TRUSTED, depth = k, where = a_k.  An anchor is checked for nothing and lends no pathLen.
 *                   2. else the first broken of own(a_k); for k >= 1, as_issuer(a_k); for k >= 1, PATH_LEN where k - 1 > path_len(a_k):
 *                      that verdict, where = a_k, depth = k.
 *                   3. else NO_ANCHOR where the issuer of a_k is MLDSA_X509_NO_ISSUER, >= n or a_k itself.
 *                   4. else DEPTH where k + 1 > MLDSA_PATH_MAX_DEPTH.
 *                 The loop's bound is the constant; each step reads one 8-byte node.
 * Cost, from counts (an expectation): 68 bytes read and 8 written per certificate by k_path_node, then one dependent 8-byte read per
 *   step of the climb and 8 bytes written: for chains of depth 3 a few times a device-to-device copy of the node array.
 * Measured: not measured (profiles/path_bench.jsonl).
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs, policy, cert_status, cert_ok, anchor or results, certs, policy or results not
 *   8-byte aligned, n > MLDSA_PATH_MAX_CERTS, an unknown flag bit, scratch NULL, not 256-byte aligned or smaller than
 *   mldsa_path_scratch_bytes(n).  n = 0 returns MLDSA_OK and touches nothing. */
int mldsa_path_chain(mldsa_ctx *ctx, const mldsa_x509_cert *certs, const mldsa_path_fields *policy, const uint8_t *cert_status,
                     const uint8_t *cert_ok, const uint8_t *revocation, const uint8_t *anchor, size_t n, int64_t now, unsigned flags,
                     mldsa_path_result *results, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_PATH_H */
