/* mldsa_keycheck.h -- strict import of wire-format ML-DSA private keys on the device (libmldsa_keycheck.so).
 *
 * FIPS 204 (August 2024) Algorithm 25 (skDecode) unpacks s1 and s2 from fields of 3 (eta = 2) or 4 (eta = 4) bits and marks its lines
 * 3 and 6 "may lie outside [-eta, eta], if input is malformed": the check is left to the importer.  Nothing in Algorithm 25 relates
 * the t0 and tr fields of a key to its rho, s1 and s2 either, nor the private key to the public key delivered with it.  The core's
 * mldsa_sk_expand imports any byte string of the right length, as the reference crate does, so the entries below cite FIPS 204
 * instead of crate lines.  They give every wire key a verdict byte:
 *   - the range check of Algorithm 25, lines 3 and 6;
 *   - the pairwise consistency of the key: t = A s1 + s2 with A = ExpandA(rho) (Algorithm 6, lines 3 and 5), (t1, t0) =
 *     Power2Round(t) (Algorithm 35; Algorithm 6, line 6) against the key's t0 field, tr = H(pkEncode(rho, t1), 64) (Algorithm 6,
 *     lines 8 and 9; Algorithm 22) against its tr field, and pkEncode(rho, t1) against a public key given with it.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h, like libmldsa_ph.so, libmldsa_keys.so, libmldsa_mu.so and
 * libmldsa_seed.so: it reaches the core only through the core's public entry points (mldsa_expand_a and mldsa_verify_arith do the
 * arithmetic, mldsa_sk_expand the import itself) and adds the kernels between them.
 *
 * Conventions are those of mldsa_seed.h: pointers to operation data are DEVICE pointers, `stream` is a hipStream_t (NULL = the default
 * stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on mldsa_ctx_device(ctx) and
 * restores the caller's current device.  Every call is asynchronous on `stream`.
 *
 * Scratch is the caller's (256-byte aligned device memory), used in stream order, and may be reused by the next call on the same
 * stream.  mldsa_keycheck_scratch_bytes(set, n_keys) is what ONE pass over n_keys keys needs.  A smaller scratch is legal: the call
 * then checks the keys in passes of the largest P whose scratch fits, with identical results.  A pass is at least min(n_keys, 64)
 * keys; below that the call returns MLDSA_ERR_NOMEM before anything is launched.  The scratch holds secrets during the call (s1 and
 * t = A s1 + s2 before rounding): every entry point that takes one zeroes ALL scratch_bytes on `stream` behind its last kernel (the
 * core's mldsa_memset).
 *
 * Secrets and control flow: s1, s2, t0 and the comparisons against them never decide a branch, a trip count or an address; what a
 * kernel does depends on the parameter set and the key's number only.  The verdict bytes are public once written.
 *
 * On error: MLDSA_ERR_PARAM and MLDSA_ERR_NOMEM are returned before anything is launched and leave every output untouched.  Any other
 * error (MLDSA_ERR_DEVICE, a failed core call) may come up after work was launched: the outputs are then UNDEFINED and must not be
 * used; the scratch is still zeroed on `stream`.
 */
#ifndef MLDSA_KEYCHECK_H
#define MLDSA_KEYCHECK_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_KEYCHECK_ABI_VERSION 1
/* most keys of one call */
#define MLDSA_KEYCHECK_MAX_KEYS ((size_t)1 << 24)

/* Verdict bits of one key; 0 = the key is good.  A key with a range bit reports the three consistency bits as 0 (they are computed
 * all the same and masked at the end), so a verdict is one of 0, 1, 2, 3 or a subset of {4, 8, 16}.  The t0 field has no range bit:
 * every 13-bit value is a legal field of BitPack(t0, 2^12 - 1, 2^12). */
#define MLDSA_KEY_S1_RANGE 1 /* a coefficient of s1 lies outside [-eta, eta]: a wire field v > 2 eta (Algorithm 25, line 3)         */
#define MLDSA_KEY_S2_RANGE 2 /* the same for s2 (Algorithm 25, line 6)                                                           */
#define MLDSA_KEY_T0 4       /* the t0 field differs from r0 of Power2Round(A s1 + s2), A = ExpandA(rho of the private key)      */
#define MLDSA_KEY_TR 8       /* the tr field differs from H(rho | SimpleBitPack(t1, 10 bits), 64)                                */
#define MLDSA_KEY_PK 16      /* a pk was given and differs from rho | SimpleBitPack(t1, 10 bits) byte for byte                   */

/* what mldsa_sk_import checks */
#define MLDSA_KEYCHECK_RANGE 1 /* mldsa_sk_range_check: the range bits only, no scratch */
#define MLDSA_KEYCHECK_PAIR 2  /* mldsa_keypair_check: every bit                        */

int mldsa_keycheck_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_keycheck_last_error(void);

/* Bytes of one pass of mldsa_keypair_check over n_keys keys; 0 for an unknown set or n_keys > MLDSA_KEYCHECK_MAX_KEYS.  With K, L of
 * the set:
 *   n_keys (1024 (K L + L + 2 K + 1) + 320 K + 48) = n_keys * 31024 / 51120 / 84528 (ML-DSA-44 / 65 / 87)
 *   per key: A_hat (K L polynomials of 1024 bytes), s1 as int32 (L), A s1 in canonical form (K), the all-zero c and t1 rows that
 *   mldsa_verify_arith reads beside them (1 + K), PK_LEN = 32 + 320 K bytes for pk' = rho | SimpleBitPack(t1), and 16 bytes of
 *   partial verdicts (one per row of t, one for tr, one for the ranges). */
size_t mldsa_keycheck_scratch_bytes(int set, size_t n_keys);

/* The range check of skDecode (FIPS 204 Algorithm 25, lines 3 and 6) for n_keys wire private keys sk[n_keys][SK_LEN]:
 * flag[i] = MLDSA_KEY_S1_RANGE and / or MLDSA_KEY_S2_RANGE, or 0.  One wave per key reads the (L + K) 32 b bytes of the s1 | s2
 * region (b = 3 for eta = 2, b = 4 for eta = 4; byte 128 onwards) in units of 32 coefficients -- three dwords of 3-bit fields or
 * four dwords of 4-bit fields per lane --, tests all fields of a dword at once with word-wide bit arithmetic (field > 2 eta) and ORs
 * the result across the wave.  No scratch.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set, n_keys > MLDSA_KEYCHECK_MAX_KEYS, a NULL sk
 *   or flag.  n_keys = 0 returns MLDSA_OK. */
int mldsa_sk_range_check(mldsa_ctx *ctx, int set, const uint8_t *sk, uint8_t *flag /* [n_keys] */, size_t n_keys, void *stream);

/* Every verdict bit for n_keys wire private keys sk[n_keys][SK_LEN] and, when pk is not NULL, the wire public keys pk[n_keys][PK_LEN]
 * delivered with them.  Per pass: the range check; s1 decoded to int32; A_hat = ExpandA(rho) (mldsa_expand_a); A s1 in canonical
 * form from ONE fused kernel of the core (mldsa_verify_arith with z = s1 and all-zero c and t1: forward NTTs, the matrix-vector
 * product and the inverse NTTs without a trip through memory between them); one wave per row (key, i < K) then decodes s2_i and the
 * 13-bit t0_i fields from the wire key, forms t = A s1 + s2 mod q, applies Power2Round, ORs the differences against the t0 field,
 * packs t1 into the pk' row (and ORs the differences against pk); tr' = H(pk', 64) is compared with bytes 64 ... 127 of the key; a
 * last kernel merges the partial verdicts, masks the consistency bits of a key with a range bit, and writes flag[i].
 * Argument errors as for mldsa_sk_range_check, and a NULL or misaligned scratch; MLDSA_ERR_NOMEM for a scratch below
 *   mldsa_keycheck_scratch_bytes(set, min(n_keys, 64)). */
int mldsa_keypair_check(mldsa_ctx *ctx, int set, const uint8_t *sk, const uint8_t *pk /* may be NULL */, uint8_t *flag /* [n_keys] */,
                        size_t n_keys, void *scratch, size_t scratch_bytes, void *stream);

/* The strict counterpart of mldsa_sk_expand: the keys are expanded into the caller's fields (rho, cap_k [n_keys][32], tr
 * [n_keys][64], s_1_hat_mont [n_keys][L][256], s_2_hat_mont / t_0_hat_mont [n_keys][K][256]; int32, 16-byte aligned) by
 * mldsa_sk_expand itself, checked at `level` -- MLDSA_KEYCHECK_RANGE (pk and scratch are not used and may be NULL) or
 * MLDSA_KEYCHECK_PAIR (mldsa_keypair_check's pk, scratch and passes) --, and every output row of a key whose flag is not 0 is then
 * set to zero; the flag is public by then.  Good keys get byte for byte what mldsa_sk_expand gives.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set or level, n_keys > MLDSA_KEYCHECK_MAX_KEYS,
 *   a NULL sk, flag or field, an int32 output that is not 16-byte aligned, at MLDSA_KEYCHECK_PAIR a NULL or misaligned scratch;
 *   MLDSA_ERR_NOMEM as for mldsa_keypair_check.  n_keys = 0 returns MLDSA_OK. */
int mldsa_sk_import(mldsa_ctx *ctx, int set, int level, const uint8_t *sk, const uint8_t *pk /* may be NULL */, uint8_t *rho,
                    uint8_t *cap_k, uint8_t *tr, int32_t *s_1_hat_mont, int32_t *s_2_hat_mont, int32_t *t_0_hat_mont,
                    uint8_t *flag /* [n_keys] */, size_t n_keys, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_KEYCHECK_H */
