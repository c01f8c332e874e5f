/* mldsa_crl.h -- the revocation leg of X.509 path validation on the device: certificate revocation lists in a blob to mldsa_rec_op
 * descriptors, to a table of revoked serials, to one answer per certificate (libmldsa_crl.so).
 *
 * mldsa_x509.h puts the signature leg of path validation on the device and names revocation as out of its scope.  A relying party that
 * has the verdicts of 65 536 certificate signatures still has to walk every CRL and look every serial up before it may trust one of
 * them.  This library does both on the device, the host touches no byte:
 *   1. the strict DER walk of every CertificateList (RFC 5280 5.1) and of every revoked entry in it;
 *   2. the CRL's own ML-DSA signature as one mldsa_rec_op -- key = the subject key of the CA certificate the caller names, message = the
 *      tbsCertList, pure mode with an empty context -- for mldsa_rec_verify (mldsa_rec.h), exactly as certificates are handled;
 *   3. a device-resident table of the revoked serials, built once per CRL refresh, and a batched lookup that answers good / revoked /
 *      unknown for every certificate of a batch.
 *
 * A C caller validates a batch with six calls on one stream (certs, fields: mldsa_x509.h):
 *     mldsa_x509_ops(ctx, blob, blob_len, certs, n_certs, MLDSA_X509_CHECK_NAMES, fields, cert_ops, cert_status, stream);
 *     mldsa_rec_verify(ctx, MLDSA_MODE_PURE, blob, blob_len, cert_ops, n_certs, cert_ok, ...);
 *     mldsa_crl_ops(ctx, blob, blob_len, crls, n_crls, fields, n_certs, MLDSA_CRL_CHECK_NAMES, crl_fields, entries, max_entries, crl_ops,
 *                   crl_status, totals, scratch, scratch_bytes, stream);
 *     mldsa_rec_verify(ctx, MLDSA_MODE_PURE, blob, blob_len, crl_ops, n_crls, crl_ok, ...);
 *     mldsa_crl_table(ctx, entries, max_entries, table, table_slots, totals, stream);
 *     mldsa_crl_check(ctx, blob, blob_len, certs, fields, cert_crl, n_certs, crls, crl_fields, crl_status, crl_ok, n_crls, entries,
 *                     max_entries, table, table_slots, revocation, stream);
 * Certificate i is valid and not revoked where cert_status[i] == 0, cert_ok[i] == 1 and revocation[i] == MLDSA_CRL_GOOD.
 * MlDsaRevocationLists.check of the Python package is these six calls.
 *
 * IN SCOPE: the strict DER structure of the fields walked, the algorithm identifiers, the version rule, every revoked entry's structure
 * and serial, issuer Name chaining byte for byte, the CRL's signature under its issuer's subject key, the lookup of a certificate's
 * serial in the CRL that its caller names for it, and that this CRL was issued by the certificate's own issuer.
 * NOT IN SCOPE, and not looked at:
 *   - thisUpdate / nextUpdate against a clock: their offsets are recorded for the caller;
 *   - delta CRLs;
 *   - indirect CRLs and the certificateIssuer entry extension;
 *   - issuingDistributionPoint;
 *   - critical extensions: the range of crlExtensions is recorded, and a caller must refuse what it does not understand;
 *   - OCSP;
 *   - PEM;
 *   - serials longer than 20 bytes (RFC 5280's limit): such an entry refuses its CRL, such a certificate is MLDSA_CRL_CERT;
 *   - the host-memory, group and batcher forms of the other libraries;
 *   - the C++ / Rust mirrors.
 * Times, reason codes and the content of any extension are not interpreted.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.  From mldsa_rec.h and mldsa_x509.h it takes
 * types and codes alone -- it neither links nor calls libmldsa_rec.so or libmldsa_x509.so.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.  Every
 * call is asynchronous on `stream` and never waits for the host.
 *
 * Public data only: CRLs and certificates.  Nothing here is cleared for secrecy.
 */
#ifndef MLDSA_CRL_H
#define MLDSA_CRL_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"
#include "mldsa_rec.h"
#include "mldsa_x509.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_CRL_ABI_VERSION 1
#define MLDSA_CRL_MAX_CRLS (1u << 30)
#define MLDSA_CRL_MAX_ENTRIES (1u << 30)
#define MLDSA_CRL_MAX_CERTS MLDSA_X509_MAX_CERTS
/* content bytes of a serial number, RFC 5280's limit */
#define MLDSA_CRL_SERIAL_MAX 20
/* CRLs per workgroup of the walk and of the placement's scan */
#define MLDSA_CRL_SCAN_BLOCK 256
/* cert_crl[i]: no CRL covers certificate i */
#define MLDSA_CRL_NONE 0xFFFFFFFFu

/* ---- input: one per CRL, a device array, 8-byte aligned, 16 bytes each -------------------------------------------------------------------
 * [off, off + len) of the blob -- uint8[blob_len] in device memory, NO alignment requirement -- is one DER CertificateList.  `issuer`
 * is a row of the mldsa_x509_fields array that mldsa_x509_parse wrote for the certificates: the CA certificate whose subject key signs
 * this CRL.  Ranges may overlap or coincide.  Blob, array and the fields rows are untrusted. */
typedef struct {
    uint64_t off;
    uint32_t len;
    uint32_t issuer;
} mldsa_crl_item;

/* ---- what the walk finds: one row per CRL, a device array, 8-byte aligned, 88 bytes each -------------------------------------------------
 *   tbs_off, tbs_len            the whole tbsCertList TLV: the message
 *   sig_off, sig_set            the first byte behind the unused-bits byte of the signatureValue BIT STRING, and its parameter set
 *   issuer_off, issuer_len      the whole issuer Name TLV
 *   this_off, next_off          the thisUpdate and nextUpdate TLVs (tag 17 or 18); next_off = 0: no nextUpdate
 *   revoked_off, revoked_len    the CONTENT of revokedCertificates: the entries; 0, 0 where the field is absent
 *   ext_off, ext_len            the CONTENT of the Extensions SEQUENCE inside [0] crlExtensions; 0, 0 where the field is absent
 *   first, count                the CRL's slots of the entry table are [first, first + revoked_len / 20), of which the first `count`
 *                               hold its entries, in the CRL's order (mldsa_crl_ops; mldsa_crl_parse leaves both 0)
 *   status                      after mldsa_crl_parse the walk's: OK, RANGE, DER, ALG, SIG, VERSION or ENTRY; mldsa_crl_ops then
 *                               writes SPACE and ENTRY here too.  ISSUER and NAME appear in the status array only.
 * Offsets are absolute blob offsets.  A status of RANGE or DER leaves every other field 0; sig_off and sig_set are nonzero only where
 * the walk's status is OK; count is nonzero only where the CRL's final status is OK. */
typedef struct {
    uint64_t tbs_off, sig_off, issuer_off, this_off, next_off, revoked_off, ext_off;
    uint32_t tbs_len, issuer_len, revoked_len, ext_len, first, count;
    uint8_t sig_set, status, reserved[6];
} mldsa_crl_fields;

/* ---- the entry table: max_entries rows of 32 bytes, a device array the caller owns, 8-byte aligned ---------------------------------------
 *   serial, serial_len   the content bytes of userCertificate as they stand in the DER (a sign byte 00 included), zero-padded
 *   crl                  the CRL's index;  off the entry's first byte, relative to the CRL's first byte
 * serial_len == 0 marks an empty slot.  Placement: CRL i gets bound_i = revoked_len_i / 20 slots (the smallest legal entry is 20 bytes)
 * at first_i = the sum of bound_j over the CRLs j < i whose header walk was OK -- an exclusive scan in CRL order, known from the headers
 * alone, so the entries are walked once.  Holes behind count_i stay empty, and so do all slots of a CRL whose final status is not OK. */
typedef struct {
    uint8_t serial[20];
    uint8_t serial_len;
    uint8_t reserved[3];
    uint32_t crl;
    uint32_t off;
} mldsa_crl_entry;

/* ---- what a call counts: one row in device memory, 8-byte aligned, 40 bytes --------------------------------------------------------------
 * mldsa_crl_ops writes the first four: CRLs whose status is OK and not OK, entry rows written for the accepted CRLs, slots reserved
 * (the sum of bound_i over the CRLs that got their slots).  mldsa_crl_table writes `overflow` alone: 1 where an insert found no free
 * slot -- impossible in a table of mldsa_crl_table_slots slots, and the lookup is then not to be trusted. */
typedef struct {
    uint64_t accepted, refused, entries, slots;
    uint32_t overflow, reserved;
} mldsa_crl_totals;

/* ---- status of a CRL: the first rule broken, tested in this order ------------------------------------------------------------------------
 * 0 ... 6 are mldsa_x509.h's, with the same meaning: MLDSA_X509_OK, _RANGE, _DER, _ALG (the outer signatureAlgorithm's content is not
 * exactly one of the three 11-byte ML-DSA OIDs, or the TBS's inner `signature` TLV is not byte for byte the outer one), _SIG (the BIT
 * STRING is not 1 + SIG_LEN bytes or its unused-bits byte is not 0); then the codes below; then _ISSUER (issuer >= n_certs, the issuer's
 * own status is RANGE or DER, its key_set is 0 or differs from the CRL's sig_set) and, with MLDSA_CRL_CHECK_NAMES, _NAME (the CRL's
 * issuer Name TLV differs from the CA's subject Name TLV in length or in any byte).  The new codes are disjoint from every code of
 * mldsa_x509.h, mldsa_x509sign.h and mldsa_csr.h (0 ... 18). */
#define MLDSA_CRL_VERSION 19 /* a version that is not 02 01 01 (v2), or crlExtensions without a version */
#define MLDSA_CRL_ENTRY 20   /* revokedCertificates present but empty, or any entry malformed (below): one entry that cannot be read
                                refuses the whole CRL -- a list that cannot be read completely cannot vouch for anybody */
#define MLDSA_CRL_SPACE 21   /* first_i + bound_i > max_entries: the CRL's slots do not lie inside the entry table (a CRL without a list,
                                bound_i = 0, is refused too where first_i itself lies behind the table's end) */

/* flags of mldsa_crl_ops */
#define MLDSA_CRL_CHECK_NAMES 1u

/* ---- revocation[i]: one byte per certificate, the rules tested in this order -------------------------------------------------------------*/
#define MLDSA_CRL_GOOD 0        /* none of the below: the serial is not in the CRL */
#define MLDSA_CRL_REVOKED 1     /* the serial is in the CRL */
#define MLDSA_CRL_NO_CRL 2      /* cert_crl[i] == MLDSA_CRL_NONE */
#define MLDSA_CRL_CRL_INDEX 3   /* cert_crl[i] >= n_crls */
#define MLDSA_CRL_CRL_REFUSED 4 /* the CRL's status is not OK, or crl_ok is not NULL and crl_ok[c] == 0 */
#define MLDSA_CRL_CERT 5        /* the certificate's own row is RANGE or DER, its TBS range is not inside the blob, or its serial does
                                   not pass the INTEGER rule below */
#define MLDSA_CRL_SCOPE 6       /* certs[i].issuer != crls[c].issuer: the CRL was not issued by the certificate's issuer.  With both
                                   link steps done (CHECK_NAMES in both libraries) equal issuers imply equal Names */

/* ---- the walk (fips204_amd/crl/crl_plan.h: constexpr functions on a fetch functor, which the kernels and a stand-alone host program
 * both run; read_tlv is mldsa_x509.h's, with every refusal it lists) -------------------------------------------------------------------------
 * walk_crl, a fixed sequence of at most 12 read_tlv steps:
 *   1. The CertificateList: tag 0x30, filling [0, len) exactly.
 *   2. Its content: tbsCertList 0x30, AlgorithmIdentifier 0x30, BIT STRING 0x03, ending exactly at the list's end.
 *   3. Inside the TBS, in this order and ending exactly at the TBS's end: an optional 0x02 version; 0x30 the inner algorithm; 0x30 the
 *      issuer Name; thisUpdate, tag 0x17 or 0x18; an optional nextUpdate, tag 0x17 or 0x18; an optional 0x30 revokedCertificates; an
 *      optional 0xA0 crlExtensions whose content is one 0x30 filling it exactly.
 *   A wrong tag or trailing bytes is DER.  Then ALG, SIG, VERSION and ENTRY (the empty list) in this order.
 * walk_entry, one revoked entry: 0x30; inside it a 0x02 userCertificate of 1 ... MLDSA_CRL_SERIAL_MAX content bytes, minimally encoded
 *   (a leading 00 only before a byte >= 0x80, a leading FF only before a byte < 0x80); a Time, tag 0x17 or 0x18, of at least 13 content
 *   bytes (the shortest form RFC 5280 allows, which makes 20 bytes the smallest entry); an optional 0x30 crlEntryExtensions; the entry
 *   ends exactly at its own end.  The entries must fill revokedCertificates exactly.
 * No byte outside [off, off + len) of a CRL is ever read, the aligned wide loads of the entry walk included, and no loop runs to a count
 * taken from the data: the hop over the entries of CRL i makes at most bound_i steps. */

int mldsa_crl_abi_version(void);
/* message of the last failed call of this thread */
const char *mldsa_crl_last_error(void);

/* host helpers.  bytes / 20: the slots a revokedCertificates content of `bytes` bytes can need; a caller who sizes `entries` as the sum
 * of mldsa_crl_entries_bound(len_i) over its CRLs never sees SPACE. */
size_t mldsa_crl_entries_bound(size_t bytes);
/* slots of the lookup table over max_entries entry rows: the power of two >= 2 max_entries, at least 64 (uint32 each); 0 for
 * max_entries > MLDSA_CRL_MAX_ENTRIES */
size_t mldsa_crl_table_slots(size_t max_entries);
/* working memory of mldsa_crl_ops: R(8 B) bytes, R(x) = x rounded up to a multiple of 256 and B = ceil(n_crls / MLDSA_CRL_SCAN_BLOCK): one
 * 64-bit sum per workgroup of the scan.  0 for n_crls > MLDSA_CRL_MAX_CRLS. */
size_t mldsa_crl_scratch_bytes(size_t n_crls);

/* crl_fields[i] = the header walk of CRL i (first = count = 0).  mldsa_crl_ops' first step, on its own as a test seam.  One launch,
 * k_crl_parse: one CRL per lane, 256 lanes per workgroup.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, crls or crl_fields, NULL blob with blob_len > 0, crls or crl_fields not 8-byte aligned,
 *   n_crls > MLDSA_CRL_MAX_CRLS.  n_crls = 0 returns MLDSA_OK without a context and touches nothing. */
int mldsa_crl_parse(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_crl_item *crls, size_t n_crls,
                    mldsa_crl_fields *crl_fields, void *stream);

/* The CRLs to rows, entry rows, ops and status.  `entries` (max_entries rows) and `totals` are cleared, then four steps ordered by the
 * kernel boundaries alone:
 *   parse     k_crl_parse, as above.
 *   place     the exclusive scan of the bounds (k_crl_place_sums, k_crl_place_offsets, k_crl_place: a plain block scan of
 *             MLDSA_CRL_SCAN_BLOCK lanes, the blocks' sums in `scratch`): first_i, and SPACE.
 *   entries   k_crl_entries, one CRL per wave, four waves per workgroup.  The wave stages a 1 KiB window of the revoked list into LDS
 *             with aligned 16-byte loads, 64 lanes x 16 bytes; lane 0 hops from entry header to entry header inside the window and
 *             notes the starts; the lanes then run walk_entry on one entry each and write the 32-byte rows; the window is reloaded,
 *             aligned down, where the next header leaves it.  A byte outside the window is read from the blob, so an entry that
 *             straddles or outgrows the window needs no special case.  count_i, and ENTRY where any entry was refused, where the
 *             entries do not end at the list's end or where they are more than bound_i.
 *   link      k_crl_link, one CRL per wave: ISSUER, NAME (with MLDSA_CRL_CHECK_NAMES, 64 bytes per step), status[i] and ops[i] --
 *             pk_off = the CA's key_off, sig_off = the CRL's, msg_off / msg_len = its tbsCertList, ctx_off = ctx_len = 0, set = its
 *             sig_set.  Every CRL that is not OK gets an all-zero op, count = 0 and its slots emptied again.
 * cert_fields (n_certs rows) is read as it is; a Name range of a row that does not lie inside the blob is not followed and counts as a
 * mismatch.  Nothing outside [first_i, first_i + bound_i) of `entries` is written for CRL i.
 *
 * Cost, from counts (an expectation): per CRL about 12 dependent header reads and one 88-byte row; per entry one hop of two to six LDS
 *   byte reads by lane 0, about 20 - 40 bytes of the list read once through the window, and one 32-byte row written -- against the
 *   2.4 - 4.6 KB signature and the key that mldsa_rec_verify then moves per CRL.
 * Measured on an MI355X (tools/bench_crl.py -> profiles/crl_bench.jsonl; medians of alternating runs in one process), entries of 27
 *   bytes, CRLs 5 mod 16 bytes apart, 65 536 certificates looked up:
 *                                                  4 096 CRLs of 64 entries              one CRL of 262 144 entries
 *                                                  ML-DSA-44   ML-DSA-65   ML-DSA-87     ML-DSA-44
 *     mldsa_crl_parse                              0.019 ms    0.019 ms    0.021 ms      0.012 ms
 *     this call                                    0.182 ms    0.181 ms    0.182 ms      126 ms
 *       entries per second                         1.44 G      1.45 G      1.44 G        2.1 M
 *     this call / mldsa_rec_verify on its ops      0.33        0.30        0.25          1.09     (0.55 / 0.61 / 0.72 / 115 ms)
 *     mldsa_crl_table                              0.027 ms    0.027 ms    0.027 ms      0.039 ms
 *       / a device-to-device copy of the rows      3.2         3.0         3.4           1.5
 *     mldsa_crl_check                              0.018 ms    0.017 ms    0.019 ms      0.024 ms (about 0.3 ns per certificate)
 *       / mldsa_x509_ops on the same certificates  0.33        0.32        0.33          0.42
 *     a Python walk into a set and the lookups
 *       / the three calls                          1 040       1 080       1 140         1.9      (0.45 - 0.50 us per entry, 1.7 - 2.0 us per lookup)
 *   One CRL is one wave's work: across 4 096 CRLs the hops run side by side, inside one CRL they are a chain -- the wave takes about
 *   480 ns per entry there, several times the 100 cycles expected of a hop --, so a single list of 262 144 entries takes as long as
 *   its own signature check (whose 7 MB message is hashed by one chain as well).  Splitting one long list among waves is not built.
 * Argument errors (MLDSA_ERR_PARAM): as mldsa_crl_parse, and NULL cert_fields with n_certs > 0, NULL entries with max_entries > 0, NULL
 *   ops, status or totals, cert_fields, entries, ops or totals not 8-byte aligned, n_certs > MLDSA_CRL_MAX_CERTS, max_entries >
 *   MLDSA_CRL_MAX_ENTRIES, an unknown flag bit, scratch NULL, not 256-byte aligned or smaller than mldsa_crl_scratch_bytes(n_crls).
 *   n_crls = 0 returns MLDSA_OK and touches nothing. */
int mldsa_crl_ops(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_crl_item *crls, size_t n_crls,
                  const mldsa_x509_fields *cert_fields, size_t n_certs, unsigned flags, mldsa_crl_fields *crl_fields,
                  mldsa_crl_entry *entries, size_t max_entries, mldsa_rec_op *ops, uint8_t *status, mldsa_crl_totals *totals,
                  void *scratch, size_t scratch_bytes, void *stream);

/* The lookup table over the entry rows: built once per CRL refresh and reused by every mldsa_crl_check.  `table` (table_slots uint32)
 * is cleared; then k_crl_insert, one entry slot per lane, grid-stride over max_entries: an empty slot is skipped, a full one hashes
 * (crl, serial_len, serial) -- a fixed mix, crl_plan.h -- and claims a table slot by atomicCAS on empty, with linear probing; a claimed
 * slot holds entry index + 1.  The probe loop is bounded by table_slots; an insert that runs out sets totals->overflow (cleared first).
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, table or totals, NULL entries with max_entries > 0, entries or totals not 8-byte aligned,
 *   table not 4-byte aligned, max_entries > MLDSA_CRL_MAX_ENTRIES, table_slots not a power of two, below
 *   mldsa_crl_table_slots(max_entries) or above 2^31. */
int mldsa_crl_table(mldsa_ctx *ctx, const mldsa_crl_entry *entries, size_t max_entries, uint32_t *table, size_t table_slots,
                    mldsa_crl_totals *totals, void *stream);

/* revocation[i] for every certificate of a batch (values above).  cert_crl[i] names the CRL that covers certificate i, or
 * MLDSA_CRL_NONE.  crl_status is mldsa_crl_ops' status array; crl_ok, where not NULL, mldsa_rec_verify's verdicts on its ops.  One
 * launch, k_crl_check, one certificate per lane: the serial is read from tbs_off of the certificate's fields row -- the TBS header, an
 * optional 0xA0, then 0x02 by the INTEGER rule --, the table is probed from the serial's home slot, and crl, serial_len and the bytes
 * are compared with the entry row: no blob read is made for the entries.  The certificates need not be the ones mldsa_crl_ops saw, as
 * long as `issuer` means the same rows.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, certs, cert_fields, cert_crl, crl_status, table or revocation, NULL blob with blob_len >
 *   0, NULL crls or crl_fields with n_crls > 0, NULL entries with max_entries > 0, certs, cert_fields, crls, crl_fields or entries not
 *   8-byte aligned, cert_crl or table not 4-byte aligned, the caps, and table_slots as above.  n_certs = 0 returns MLDSA_OK and touches
 *   nothing. */
int mldsa_crl_check(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_x509_cert *certs,
                    const mldsa_x509_fields *cert_fields, const uint32_t *cert_crl, size_t n_certs, const mldsa_crl_item *crls,
                    const mldsa_crl_fields *crl_fields, const uint8_t *crl_status, const uint8_t *crl_ok, size_t n_crls,
                    const mldsa_crl_entry *entries, size_t max_entries, const uint32_t *table, size_t table_slots, uint8_t *revocation,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_CRL_H */
