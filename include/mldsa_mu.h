/* mldsa_mu.h -- ML-DSA with an externally computed message representative mu on the device (libmldsa_mu.so).
 *
 * FIPS 204 lets mu = H(BytesToBits(tr) || M', 64) be computed outside the signing module: line 6 of Algorithm 7
 * (ML-DSA.Sign_internal) and line 7 of Algorithm 8 (ML-DSA.Verify_internal) are the only places where tr and the message enter,
 * and section 6.2 / 6.3 name the "externally computed mu" option; ACVP tests it as `externalMu`.  The reference crate has no such
 * interface, so the entries below cite FIPS 204 (August 2024) instead of crate lines.  A client that holds the message and the
 * 64-byte tr hashes locally and hands over 64 bytes per operation; the device signs or verifies from them.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h, like libmldsa_ph.so and libmldsa_keys.so: it reaches the core
 * only through the core's public entry points (the seam-level primitives do all the arithmetic and every codec) and adds the
 * kernels that touch mu: the hash of mu itself, the commitment hash c_tilde = H(mu || w1Encode(w1)) fused with UseHint / HighBits,
 * rho'' = H(K || rnd || mu), and the accept step and compaction of the signer's rejection loop.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers, keys are passed expanded, field by field
 * (mldsa_pk_expand / mldsa_sk_expand), key_idx[op] < n_keys selects the key of an op (NULL: op i uses key i), `stream` is a
 * hipStream_t (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  tr is an input of mldsa_mu_compute only: mu has consumed it.
 *
 * Scratch is the caller's (256-byte aligned device memory), used in stream order, and may be reused by the next call on the same
 * stream.  mldsa_mu_*_scratch_bytes(set, n_ops) is what ONE pass over n_ops operations needs.  A smaller scratch is legal: the call
 * then runs in passes of the largest P with mldsa_mu_*_scratch_bytes(set, P) <= scratch_bytes, with identical results.  The minimum
 * is mldsa_mu_*_scratch_bytes(set, min(n_ops, 64)) -- a pass is at least one wave of operations --; below it the call returns
 * MLDSA_ERR_NOMEM before anything is launched.
 */
#ifndef MLDSA_MU_H
#define MLDSA_MU_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_MU_ABI_VERSION 1
#define MLDSA_MU_LEN 64
/* most operations of one call */
#define MLDSA_MU_MAX_OPS ((size_t)1 << 30)

int mldsa_mu_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_mu_last_error(void);

/* Bytes of one pass over n_ops operations; 0 for an unknown set or n_ops > MLDSA_MU_MAX_OPS.  With K, L of the set:
 *   verify: n_ops (1024 (K L + 3 K + L + 1) + 128)
 *           per op: A_hat (K L polynomials of 1024 bytes), the key's t1 row, h and w' (K each), z (L), c (1); rho 32, c_tilde 64,
 *           the decode verdict 16, ||z||inf and the key flag 16.
 *   sign:   256 + n_ops (1024 (K L + 5 L + 6 K + 1) + 400) + ceil(n_ops / 2) (1024 K L + 192)
 *           per op: A_hat (K L), the key's s1 | s2 | t0 rows and c s1 | c s2 | c t0 (L + 2 K each), y, NTT(y) and the accepted z (L
 *           each), w and the accepted h (K each), c (1); 400 bytes of per-op state (mu, rho'', kappa, c_tilde, indices, flags);
 *           per two ops: the second A_hat buffer and state set that compaction gathers into (the live ops have at least halved
 *           whenever it runs); 256 bytes of counters. */
size_t mldsa_mu_verify_scratch_bytes(int set, size_t n_ops);
size_t mldsa_mu_sign_scratch_bytes(int set, size_t n_ops);

/* mu = H(BytesToBits(tr) || M', 64) for n_ops operations (FIPS 204 Algorithm 7 line 6 / Algorithm 8 line 7), M' formatted by `mode`
 * as in mldsa_verify / mldsa_sign: MLDSA_MODE_INTERNAL M' = M; MLDSA_MODE_PURE M' = 0x00 | len(ctx) | ctx | M (Algorithm 2 line 10);
 * MLDSA_MODE_PREHASH M' = 0x01 | len(ctx) | ctx | OID | PH(M) with the message = OID | PH(M) (Algorithm 4 line 23).
 *   tr[n_keys][64], key_idx as everywhere; msgs / msg_off / ctxs / ctx_off: concatenated byte strings and n_ops + 1 offsets each
 *   (ctx_off NULL = every ctx empty), untrusted like in the core: the call vouches for [off[0], off[n_ops]) and reads nothing else.
 *   mu[n_ops][64].  mu_flag[n_ops] (may be NULL): 0 = hashed; 2 = the op's offset pair is not in order inside the call's range, or
 *   its key index is not below n_keys; 1 = its ctx is longer than 255 bytes (Algorithm 2 line 1).  Nothing of a flagged op is read
 *   and its mu row is all zero.  Precedence: offsets, then ctx length, then the key index.
 * One message per lane, absorbed straight from where it lies.  Asynchronous on `stream`; needs no scratch.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown mode, a NULL tr / msg_off / mu, n_keys = 0,
 *   n_ops > MLDSA_MU_MAX_OPS.  n_ops = 0 returns MLDSA_OK. */
int mldsa_mu_compute(mldsa_ctx *ctx, int mode, const uint8_t *tr /* [n_keys][64] */, size_t n_keys, const uint32_t *key_idx,
                     const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off,
                     uint8_t *mu /* [n_ops][64] */, int32_t *mu_flag /* [n_ops], may be NULL */, size_t n_ops, void *stream);

/* ML-DSA.Verify_internal from mu (FIPS 204 Algorithm 8 with line 7 done by the caller): ok[op] = 1 iff the algorithm accepts
 * sigs[op] under key key_idx[op] with mu[op].  ok[op] = 0 when mu_flag[op] is non-zero (mu_flag may be NULL), the key index is
 * not below n_keys, the hints are malformed (Algorithm 21 returns the error symbol), ||z||inf >= gamma1 - beta or c_tilde differs; such an op
 * never touches memory outside the tables.  rho[n_keys][32], t1_d2_hat_mont[n_keys][K][256] as for mldsa_verify.
 * Asynchronous on `stream`.  Argument errors: MLDSA_ERR_PARAM for a NULL ctx, an unknown set, a NULL rho / t1_d2_hat_mont / mu /
 *   sigs / ok, n_keys = 0, n_ops > MLDSA_MU_MAX_OPS, a NULL or misaligned scratch; MLDSA_ERR_NOMEM for a scratch below the minimum.
 *   n_ops = 0 returns MLDSA_OK. */
int mldsa_verify_mu(mldsa_ctx *ctx, int set, const uint8_t *rho, const int32_t *t1_d2_hat_mont, size_t n_keys, const uint32_t *key_idx,
                    const uint8_t *mu, const int32_t *mu_flag /* may be NULL */, const uint8_t *sigs, uint8_t *ok, size_t n_ops,
                    void *scratch, size_t scratch_bytes, void *stream);

/* ML-DSA.Sign_internal from mu (FIPS 204 Algorithm 7 with line 6 done by the caller): sigs[op] is the signature of the first
 * accepted kappa, byte for byte what mldsa_sign(MLDSA_MODE_INTERNAL) gives on a message M with mu = H(tr || M, 64).  rnd[n_ops][32]
 * (all zero = the deterministic variant, Algorithm 2 line 5).  Private keys expanded as for mldsa_sign.
 *   status (may be NULL): MLDSA_OK; MLDSA_ERR_CTX_LEN where mu_flag[op] = 1; MLDSA_ERR_PARAM where mu_flag[op] is another non-zero
 *   value or the key index is not below n_keys.  The signature of a failed op is all zero.  mu_flag may be NULL.
 * Blocks like mldsa_sign: every op is signed when the call returns.  The rejection loop tests one candidate per unfinished op and
 *   round and reads the number of unfinished ops on the host once per round; finished ops are compacted away whenever at least
 *   half of the rows have finished.
 * Before the call returns -- also after an error that came up once work was launched -- the whole scratch (all scratch_bytes) is zeroed on `stream`: it held rho'',
 *   y, c s1, c s2, c t0 and copies of K, s1, s2, t0.
 * Argument errors as for mldsa_verify_mu, with a NULL rho / cap_k / s_1_hat_mont / s_2_hat_mont / t_0_hat_mont / mu / rnd / sigs. */
int mldsa_sign_mu(mldsa_ctx *ctx, int set, const uint8_t *rho, const uint8_t *cap_k, const int32_t *s_1_hat_mont,
                  const int32_t *s_2_hat_mont, const int32_t *t_0_hat_mont, size_t n_keys, const uint32_t *key_idx,
                  const uint8_t *mu, const int32_t *mu_flag, const uint8_t *rnd, uint8_t *sigs, int32_t *status /* may be NULL */,
                  size_t n_ops, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_MU_H */
