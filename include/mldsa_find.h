/* mldsa_find.h -- the front of X.509 path validation on the device: every certificate's issuer, every CRL's issuer and every
 * certificate's CRL found among an unordered bag of certificates, by subject Name and key identifier (libmldsa_find.so).
 *
 * mldsa_x509.h, mldsa_crl.h and mldsa_path.h verify, look up and climb from indices their caller supplies: mldsa_x509_cert.issuer,
 * mldsa_crl_item.issuer and cert_crl[i].  To supply them a caller has to read the issuer and subject Names of every certificate, which
 * is the host DER walk those libraries were built to avoid.  This library finds the indices on the device: a hash table over the
 * candidates' (parameter set, subject Name, subjectKeyIdentifier), one lookup per certificate and per CRL with (signature set, issuer
 * Name, authorityKeyIdentifier), every answer confirmed byte for byte.
 *
 * A C caller builds the paths of a batch with these calls on one stream and then goes on as mldsa_path.h describes, with certs_out in the
 * place of certs and crls_out in the place of crls:
 *     mldsa_x509_parse(ctx, blob, blob_len, certs, n, fields, stream);                       (certs[i].issuer is not read)
 *     mldsa_path_parse(ctx, blob, blob_len, certs, n, 0, policy, stream);
 *     mldsa_find_build(ctx, blob, blob_len, certs, fields, policy, n, seed, 64, ids, totals, certs_out, results, scratch, scratch_bytes, stream);
 *     mldsa_crl_parse(ctx, blob, blob_len, crls, n_crls, crl_fields, stream);
 *     mldsa_find_crl_issuers(ctx, blob, blob_len, crls, crl_fields, n_crls, certs, fields, ids, n, seed, 64, totals, scratch, scratch_bytes,
 *                            crls_out, crl_results, stream);
 *     mldsa_find_cert_crls(ctx, certs_out, n, crls_out, n_crls, cert_crl, scratch, scratch_bytes, stream);
 * MlDsaPathBuilder.build of the Python package is these calls.
 *
 * IN SCOPE: the strict DER structure of subjectKeyIdentifier and authorityKeyIdentifier, the matching of issuer Name to subject Name byte
 * for byte, of the authorityKeyIdentifier's keyIdentifier to the subjectKeyIdentifier, and of the signature's parameter set to the key's.
 * NOT IN SCOPE, and not looked at: authorityCertIssuer / authorityCertSerialNumber (skipped); Name comparison by RFC 5280's string
 * preparation rules (Names are compared as bytes, as mldsa_x509.h does); choosing among several matching issuers by trying their keys (the
 * lowest index is named, `candidates` says how many there were); AIA fetching; PEM; the C++ / Rust mirrors.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.  From mldsa_rec.h, mldsa_x509.h, mldsa_crl.h
 * and mldsa_path.h it takes types and codes alone -- it neither links nor calls their libraries.
 *
 * Conventions are those of mldsa_path.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.  Every
 * call is asynchronous on `stream` and never waits for the host.  The blob and every input array are untrusted.
 *
 * Public data only: certificates and CRLs.  Nothing here is cleared.
 */
#ifndef MLDSA_FIND_H
#define MLDSA_FIND_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_rec.h"
#include "mldsa_x509.h"
#include "mldsa_crl.h"
#include "mldsa_path.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_FIND_ABI_VERSION 1
/* most certificates, and most CRLs, of one call: four table slots per certificate stay below 2^31 */
#define MLDSA_FIND_MAX_CERTS (1u << 28)
/* content bytes of a key identifier */
#define MLDSA_FIND_MAX_KEYID 64
/* table slots a probe visits at most: the bound of every probe loop */
#define MLDSA_FIND_PROBE_MAX 256
/* entries of the overflow list */
#define MLDSA_FIND_OVERFLOW_MAX 1024

/* ---- the identifiers: one row per certificate, a device array, 8-byte aligned, 24 bytes ---------------------------------------------------
 *   ski_off, ski_len   the CONTENT of the subjectKeyIdentifier's OCTET STRING, an absolute blob offset; 0, 0 where absent
 *   aki_off, aki_len   the CONTENT of the authorityKeyIdentifier's [0] keyIdentifier; 0, 0 where absent
 *   status             MLDSA_X509_OK, _RANGE, _DER or MLDSA_FIND_EXT; every status but OK leaves the other fields 0 */
typedef struct {
    uint64_t ski_off, aki_off;
    uint8_t ski_len, aki_len, status, reserved[5];
} mldsa_find_id;

/* New status code, disjoint from every code of mldsa_x509.h, mldsa_x509sign.h, mldsa_csr.h, mldsa_crl.h and mldsa_path.h (0 ... 25). */
#define MLDSA_FIND_EXT 26 /* subjectKeyIdentifier or authorityKeyIdentifier twice, more than MLDSA_PATH_MAX_EXTS extensions, or a value
                             of one of the two that breaks its rule (below) */

/* ---- the rules (fips204_amd/find/find_plan.h: constexpr functions on a fetch functor, which the kernels and a stand-alone host program
 * both run; read_tlv is mldsa_x509.h's, with every refusal it lists) -------------------------------------------------------------------------
 * walk_ids, the content of one Extensions SEQUENCE: one loop bounded by MLDSA_PATH_MAX_EXTS of at most 4 read_tlv steps each, then at
 * most 5 more steps for the two values:
 *   1. Each extension: 0x30 holding 0x06, an optional 0x01 (skipped: mldsa_path_parse judges it), then 0x04 ending exactly at the
 *      extension's end.  A TLV that read_tlv refuses, a wrong tag or trailing bytes is DER.  Extensions left behind the loop's bound: EXT.
 *   2. subjectKeyIdentifier (OID 55 1D 0E): the extnValue is one 0x04 filling it exactly, of 1 ... MLDSA_FIND_MAX_KEYID content bytes.
 *   3. authorityKeyIdentifier (55 1D 23): the extnValue is one 0x30 filling it exactly, which holds in this order an optional 0x80
 *      keyIdentifier of 1 ... MLDSA_FIND_MAX_KEYID content bytes, an optional 0xA1 and an optional 0x82, both skipped, and ends exactly.
 *   4. Either of the two twice, or any refusal inside one of the two values (read_tlv's included): EXT.  DER outranks EXT.
 * Which certificates take part:
 *   a CANDIDATE is a certificate j whose range lies in the blob, whose mldsa_x509_fields row has status OK, ALG or SIG and key_set != 0,
 *   whose mldsa_find_id row has status OK, and whose subject Name range and subjectKeyIdentifier range (of at most MLDSA_FIND_MAX_KEYID
 *   bytes) lie inside its own [off, off + len).  It is entered under two keys; the kind is part of the key:
 *     ANY   = (key_set, subject Name TLV)
 *     SKI   = (key_set, subject Name TLV, subjectKeyIdentifier bytes) where it has one, else NOSKI = (key_set, subject Name TLV).
 *   a SEEKER is a certificate i whose range lies in the blob, whose row has status OK (so sig_set != 0), whose mldsa_find_id row has status
 *   OK, and whose issuer Name range and keyIdentifier range lie inside its own [off, off + len).  With N its issuer Name TLV it asks for
 *     ANY(sig_set, N)                               without a keyIdentifier,
 *     SKI(sig_set, N, keyIdentifier) and NOSKI(sig_set, N) together   with one: an issuer without a subjectKeyIdentifier is not
 *                                                   excluded by an authorityKeyIdentifier (RFC 5280's practice).
 *   The issuer is the LOWEST index among the candidates entered under the keys asked for; the certificate itself is allowed (a
 *   self-signed root names itself, as mldsa_x509.h prescribes), so a caller who lists its trust anchors first gets them preferred.
 *   A CRL seeks in the same way with its sig_set, its issuer Name and the authorityKeyIdentifier of its crlExtensions, where its
 *   mldsa_crl_fields row has status OK and the ranges lie inside the CRL's own range.
 * No byte outside a certificate's (a CRL's) own range is read: every range of a row is checked against it before it is followed. */

/* ---- the answer: one row per certificate or CRL, a device array, 4-byte aligned, 12 bytes --------------------------------------------------
 *   issuer       the lowest matching candidate, MLDSA_X509_NO_ISSUER unless the status is FOUND
 *   candidates   the number of matching candidates, 0 unless the status is FOUND */
typedef struct {
    uint32_t issuer, candidates;
    uint8_t status, reserved[3];
} mldsa_find_result;

#define MLDSA_FIND_FOUND 0
#define MLDSA_FIND_NONE 1  /* a seeker, and no candidate matches */
#define MLDSA_FIND_CERT 2  /* not a seeker: nothing is looked up */
#define MLDSA_FIND_SPACE 3 /* totals.overflow > MLDSA_FIND_OVERFLOW_MAX and one of the keys asked for is in no table group (below) */

/* ---- what the table build counts: one row in device memory, 4-byte aligned, 16 bytes ----------------------------------------------------
 * candidates; keys = entries made, two per candidate; slots = table slots claimed, one per distinct hash value that found one;
 * overflow = entries that are not in their slot's group (the list keeps the first MLDSA_FIND_OVERFLOW_MAX of them). */
typedef struct {
    uint32_t candidates, keys, slots, overflow;
} mldsa_find_totals;

/* ---- the table ----------------------------------------------------------------------------------------------------------------------------
 * Open addressing over distinct hash values (tags) in S(n) = the power of two >= max(64, 4 n) slots, so the load is at most 1/2.  Entry
 * e = 2 j + k is certificate j's k-th key (0: ANY; 1: SKI or NOSKI).  The hash is a keyed 64-bit hash of kind, set, the lengths and
 * every byte of Name and identifier under `seed` (16 bytes of HOST memory, read during the call): certificates are chosen by the other
 * side, so the argument of mldsa_keys.h applies unchanged -- the seed only stops somebody who picks the Names from forcing shared slots
 * and long probes; correctness never rests on it.  hash_bits (1 ... 64; 64 is the normal value) keeps only that many bits, so that
 * tests can force collisions.
 *   k_find_claim     one certificate per wave: both hashes, 64 bytes per step; each entry walks linearly from its hash's home slot, at
 *                    most MLDSA_FIND_PROBE_MAX slots, to the first slot that is empty (atomicCAS claims it for the tag) or carries its
 *                    tag; owner = atomicMin over the entries the slot took.  The entry's key -- its ranges, checked against the
 *                    certificate's own range, kind and set -- is kept in scratch: no later step reads a candidate's rows again.  Slots only ever go from empty to one tag, so all holders
 *                    of one tag share path, slot and owner -- or run out together.
 *   k_find_confirm   one certificate per wave: each entry's key against its slot owner's, lengths first and then 64 bytes per step.
 *                    Equal: counted into the slot's group.  Different, or no slot: appended to the overflow list.
 * A key therefore lives wholly in its slot's group, whose lowest certificate is the owner's, or wholly in the overflow list.  A batch in
 * which every certificate carries one subject Name costs one comparison per entry: O(n), not O(n^2).
 * The lookup hashes the key asked for, walks the same path to its tag, compares with the owner's key byte for byte and, where that is
 * equal, answers (owner, group count).  Otherwise the key is in no group: with totals.overflow == 0 nothing matches; with at most
 * MLDSA_FIND_OVERFLOW_MAX entries the list is scanned, every entry compared in full; with more the answer is SPACE.  Results therefore
 * do not depend on the hash, the seed, hash_bits or the order in which waves ran, with that one exception, which is deterministic
 * too: which keys are in a group depends on the hash alone.  A wrong issuer is never named. */

int mldsa_find_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_find_last_error(void);

/* S(n) above; 0 for n > MLDSA_FIND_MAX_CERTS */
size_t mldsa_find_table_slots(size_t n);
/* working memory of every call here that takes `scratch`, for n certificates: with S = S(n) and R(x) = x rounded up to a multiple of 256,
 *   R(8 S) tags + R(4 S) owners + R(4 S) group counts + R(8 n) the entries' slots + R(64 n) the entries' keys (32 bytes each: the two
 *   ranges, kind and set, every range checked once by k_find_claim) + R(4 MLDSA_FIND_OVERFLOW_MAX) the overflow list
 *   + R(4 n) the lowest CRL of every CA (mldsa_find_cert_crls).
 * 0 for n > MLDSA_FIND_MAX_CERTS.  The table lives here from mldsa_find_table on; mldsa_find_cert_crls writes its own part only. */
size_t mldsa_find_scratch_bytes(size_t n);

/* ids[i] = walk_ids over the extensions range that mldsa_path_parse recorded in policy[i] (ext_off, ext_len).  A policy row whose
 * status is RANGE or DER, or whose ext_len is 0, gives status OK and no identifiers.  A certificate range outside the blob, or an
 * extensions range that does not lie inside the certificate's own [off, off + len), is not followed: status RANGE.  policy may be
 * NULL: then nothing is read, every row is OK without identifiers, and matching is by Name alone.  One launch, k_find_ids, one
 * certificate per lane.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs or ids, NULL blob with blob_len > 0, certs, policy or ids not 8-byte aligned,
 *   n > MLDSA_FIND_MAX_CERTS.  n = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_find_ids(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, const mldsa_path_fields *policy,
                   size_t n, mldsa_find_id *ids, void *stream);

/* The table over the candidates, in scratch, and *totals.  Tags, owners, counts and totals are cleared first; then k_find_claim and
 * k_find_confirm, ordered by the kernel boundary alone.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs, fields, ids, seed or totals, NULL blob with blob_len > 0, certs, fields or ids not
 *   8-byte aligned, totals not 4-byte aligned, n > MLDSA_FIND_MAX_CERTS, hash_bits outside 1 ... 64, scratch NULL, not 256-byte aligned
 *   or smaller than mldsa_find_scratch_bytes(n).  n = 0 returns MLDSA_OK and touches nothing. */
int mldsa_find_table(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, const mldsa_x509_fields *fields,
                     const mldsa_find_id *ids, size_t n, const uint8_t seed[16], int hash_bits, mldsa_find_totals *totals, void *scratch,
                     size_t scratch_bytes, void *stream);

/* results[i] and certs_out[i] = {certs[i].off, certs[i].len, results[i].issuer} for every certificate, from the table that
 * mldsa_find_table built in `scratch` with the same certs, fields, ids, n, seed and hash_bits.  certs_out may be certs itself.  One
 * launch, k_find_issuers, one certificate per wave, 64 bytes per step of every comparison; the overflow list is scanned only where
 * totals->overflow is not 0.
 * Argument errors (MLDSA_ERR_PARAM): as mldsa_find_table, and NULL certs_out or results, certs_out not 8-byte aligned, results not
 *   4-byte aligned. */
int mldsa_find_issuers(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, const mldsa_x509_fields *fields,
                       const mldsa_find_id *ids, size_t n, const uint8_t seed[16], int hash_bits, const mldsa_find_totals *totals,
                       const void *scratch, size_t scratch_bytes, mldsa_x509_cert *certs_out, mldsa_find_result *results, void *stream);

/* mldsa_find_ids, mldsa_find_table and mldsa_find_issuers on `stream`; ids and totals are written on the way.  After it
 * mldsa_x509_link and mldsa_path_chain run on certs_out unchanged.
 *
 * Cost, from counts (an expectation): per certificate one 48-byte, one 56-byte and one 16-byte row read and a 24-byte row written, a
 *   walk of 3 - 4 dependent header reads per extension, the subject Name read three times (two hashes, one comparison) and the issuer
 *   Name twice, a few 8-byte table probes and four atomics: near mldsa_x509_ops, which reads two Names per certificate once.
 * Measured: not measured (tools/bench_find.py writes profiles/find_bench.jsonl; the table goes here once that file exists).
 * Argument errors (MLDSA_ERR_PARAM): those of the three calls; policy may be NULL. */
int mldsa_find_build(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs, const mldsa_x509_fields *fields,
                     const mldsa_path_fields *policy, size_t n, const uint8_t seed[16], int hash_bits, mldsa_find_id *ids,
                     mldsa_find_totals *totals, mldsa_x509_cert *certs_out, mldsa_find_result *results, void *scratch, size_t scratch_bytes,
                     void *stream);

/* crl_results[c] and crls_out[c] = {crls[c].off, crls[c].len, crl_results[c].issuer} for every CRL, from the same table: the key's set is
 * crl_fields[c].sig_set, its Name the row's issuer_off / issuer_len, its keyIdentifier the authorityKeyIdentifier that walk_ids finds in
 * the row's ext_off / ext_len (none where ext_len is 0).  A CRL whose row is not OK, whose ranges do not lie inside its own range, or
 * whose extensions walk_ids refuses, is no seeker (CERT).  Where nothing is found the issuer written is MLDSA_X509_NO_ISSUER, which
 * mldsa_crl_ops refuses with its ISSUER code.  crls_out may be crls itself.  One launch, k_find_crl_issuers, one CRL per wave.
 * Argument errors (MLDSA_ERR_PARAM): as mldsa_find_issuers, and NULL crls, crl_fields, crls_out or crl_results, crls, crl_fields or
 *   crls_out not 8-byte aligned, crl_results not 4-byte aligned, n_crls > MLDSA_FIND_MAX_CERTS.  n_crls = 0 returns MLDSA_OK and touches
 *   nothing. */
int mldsa_find_crl_issuers(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_crl_item *crls,
                           const mldsa_crl_fields *crl_fields, size_t n_crls, const mldsa_x509_cert *certs, const mldsa_x509_fields *fields,
                           const mldsa_find_id *ids, size_t n, const uint8_t seed[16], int hash_bits, const mldsa_find_totals *totals,
                           const void *scratch, size_t scratch_bytes, mldsa_crl_item *crls_out, mldsa_find_result *crl_results, void *stream);

/* cert_crl[i] = the lowest CRL index c with crls[c].issuer == certs[i].issuer, MLDSA_CRL_NONE where there is none or where
 * certs[i].issuer >= n.  The last part of scratch (one uint32 per certificate) is set to MLDSA_CRL_NONE; then k_find_ca_min, one CRL per
 * lane, an atomicMin on its CA's word, and k_find_cert_crl, one certificate per lane, one read.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs or cert_crl, NULL crls with n_crls > 0, certs or crls not 8-byte aligned, cert_crl
 *   not 4-byte aligned, n or n_crls > MLDSA_FIND_MAX_CERTS, scratch as above.  n = 0 returns MLDSA_OK and touches nothing. */
int mldsa_find_cert_crls(mldsa_ctx *ctx, const mldsa_x509_cert *certs, size_t n, const mldsa_crl_item *crls, size_t n_crls,
                         uint32_t *cert_crl, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_FIND_H */
