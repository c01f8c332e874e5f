/* mldsa_seed.h -- ML-DSA private keys in seed form on the device (libmldsa_seed.so).
 *
 * FIPS 204 defines a key pair as ML-DSA.KeyGen_internal(xi) (Algorithm 6) of a 32-byte seed xi, and the seed is the form private
 * keys are stored and moved in: the IETF certificate profile for ML-DSA gives a private key three encodings -- the seed only, the
 * expanded key only, both -- prefers the seed, and asks an importer of "both" to check that the expanded key is the one the seed
 * generates.  The reference crate offers KeyGen::keygen_from_seed and nothing that signs from a seed, so the entries below cite
 * FIPS 204 (August 2024) instead of crate lines.  The entry points here take seeds where the core takes keys: expand a seed
 * straight into the fields mldsa_sign reads (no wire-format private key is ever written), check a wire-format private key against
 * its seed, and sign from a table of seeds.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h, like libmldsa_ph.so, libmldsa_keys.so and libmldsa_mu.so: it
 * reaches the core only through the core's public entry points (mldsa_expand_a, mldsa_expand_s, mldsa_ntt, mldsa_mat_vec_mul,
 * mldsa_inv_ntt, mldsa_to_mont do the arithmetic; mldsa_keygen and mldsa_sign whole operations) and adds the kernels between them:
 * the seed hash, t = A s1 + s2 with Power2Round and the packing of t1, tr = H(pk), and the constant-flow key comparison.
 *
 * Conventions are those of mldsa_mu.h: pointers to operation data are DEVICE pointers, `stream` is a hipStream_t (NULL = the default
 * stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on mldsa_ctx_device(ctx) and
 * restores the caller's current device.
 *
 * Scratch is the caller's (256-byte aligned device memory), used in stream order, and may be reused by the next call on the same
 * stream.  mldsa_seed_*_scratch_bytes(set, n_keys) is what ONE pass over n_keys keys needs.  A smaller scratch is legal: the call
 * then expands (checks) the keys in passes of the largest P whose scratch fits, with identical results.  A pass is at least
 * min(n_keys, 64) keys -- one wave of seeds --; below that the call returns MLDSA_ERR_NOMEM before anything is launched.  The
 * scratch holds secrets during the call (rho', s1, s2, t, t0; the generated wire keys of the check; the expanded table of the
 * signer): every entry point zeroes ALL scratch_bytes on `stream` behind its last kernel (the core's mldsa_memset).
 *
 * On error: MLDSA_ERR_PARAM and MLDSA_ERR_NOMEM are returned before anything is launched and leave every output untouched.  Any other
 * error (MLDSA_ERR_DEVICE, a failed core call) may come up after work was launched: the outputs (the key fields, pk, match, sigs,
 * status) are then UNDEFINED -- possibly partly written -- and must not be used; the scratch is still zeroed on `stream`.
 */
#ifndef MLDSA_SEED_H
#define MLDSA_SEED_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_SEED_ABI_VERSION 1
#define MLDSA_SEED_LEN 32
/* most keys of one call */
#define MLDSA_SEED_MAX_KEYS ((size_t)1 << 24)

int mldsa_seed_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_seed_last_error(void);

/* Bytes of one pass over n_keys keys; 0 for an unknown set or n_keys > MLDSA_SEED_MAX_KEYS.  With K, L of the set:
 *   expand: n_keys (1024 (K L + L + 2 K) + 320 K + 96)
 *           per key: A_hat (K L polynomials of 1024 bytes), s1 | s2 as ExpandS leaves them (L + K), A s1 (K; first in the NTT
 *           domain, then canonical), rho' 64, and PK_LEN = 32 + 320 K bytes for the wire public key that tr is hashed from
 *           (unused when the caller takes pk).
 *   check:  n_keys (PK_LEN + SK_LEN) = n_keys * 3872 / 5984 / 7488 (ML-DSA-44 / 65 / 87)
 *           the wire key pair mldsa_keygen writes for the seed.
 *   sign:   n_keys (1024 (L + 2 K) + 128) + expand(n_keys)
 *           the expanded key table (s1, s2, t0 rows; rho 32, K 32, tr 64) and one pass of the expansion that fills it.  The least
 *           mldsa_sign_seed accepts is the table plus expand(min(n_keys, 64)). */
size_t mldsa_seed_expand_scratch_bytes(int set, size_t n_keys);
size_t mldsa_seed_check_scratch_bytes(int set, size_t n_keys);
size_t mldsa_seed_sign_scratch_bytes(int set, size_t n_keys);

/* ML-DSA.KeyGen_internal(xi) (FIPS 204 Algorithm 6) for n_keys seeds xi[n_keys][32], delivered as the expanded private key that
 * mldsa_sign takes: rho, cap_k [n_keys][32], tr [n_keys][64], s_1_hat_mont [n_keys][L][256], s_2_hat_mont / t_0_hat_mont
 * [n_keys][K][256] (int32, 16-byte aligned).  pk (may be NULL): the public keys in wire format, pk[n_keys][PK_LEN].
 *   rho, cap_k, tr and pk are byte for byte what mldsa_keygen followed by mldsa_sk_expand gives for the same seed.  Every int32
 *   output is congruent modulo q, coefficient by coefficient, to that route's and lies in (-q, q) -- the range of mldsa_to_mont,
 *   inside the general contract of mldsa_hip.h (|x| < 2^31 - 2^22) that mldsa_sign accepts.  The wire private key is never
 *   materialised.
 *   Per pass: (rho, rho', K) = H(xi | K | L, 128); A_hat = ExpandA(rho); (s1, s2) = ExpandS(rho'); NTT(s1), NTT(s2) into the output
 *   rows; A_hat o NTT(s1); inverse NTT; t = A s1 + s2, Power2Round, t0 into its output rows and t1 packed into the pk row;
 *   NTT(t0); the three outputs into Montgomery form; tr = H(pk, 64).
 * Asynchronous on `stream`.  Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set,
 *   n_keys > MLDSA_SEED_MAX_KEYS, a NULL xi or output other than pk, an int32 output that is not 16-byte aligned, a NULL or
 *   misaligned scratch; MLDSA_ERR_NOMEM for a scratch below mldsa_seed_expand_scratch_bytes(set, min(n_keys, 64)).  n_keys = 0
 *   returns MLDSA_OK. */
int mldsa_seed_expand(mldsa_ctx *ctx, int set, const uint8_t *xi, uint8_t *rho, uint8_t *cap_k, uint8_t *tr, int32_t *s_1_hat_mont,
                      int32_t *s_2_hat_mont, int32_t *t_0_hat_mont, uint8_t *pk /* may be NULL */, size_t n_keys, void *scratch,
                      size_t scratch_bytes, void *stream);

/* The consistency check of a private key that arrives as seed AND expanded key: match[i] = 1 iff sk[i] (wire format,
 * sk[n_keys][SK_LEN]) is byte for byte ML-DSA.KeyGen_internal(xi[i]).sk, else 0.  The wire key of the seed is generated by
 * mldsa_keygen into the scratch and compared by one wave per key: 16-byte loads of both keys, the differences ORed across the wave,
 * no data-dependent branch and no data-dependent address -- both operands are secret.
 * Asynchronous on `stream`.  Argument errors as for mldsa_seed_expand, with a NULL xi / sk / match. */
int mldsa_seed_check(mldsa_ctx *ctx, int set, const uint8_t *xi, const uint8_t *sk, uint8_t *match /* [n_keys] */, size_t n_keys,
                     void *scratch, size_t scratch_bytes, void *stream);

/* mldsa_sign with the key table given as seeds: xi[n_keys][32] is expanded ONCE per call into the scratch (mldsa_seed_expand's
 * passes), then the core's mldsa_sign runs on those fields.  mode, key_idx, msgs / msg_off, ctxs / ctx_off, rnd, sigs, status, the
 * per-op refusals and the all-zero signature of a refused op are exactly mldsa_sign's; the signatures are byte for byte those of
 * mldsa_keygen -> mldsa_sk_expand -> mldsa_sign.  Blocks like mldsa_sign: every op is signed when the call returns.
 * Before the call returns -- also after an error that came up once work was launched -- the whole scratch is zeroed.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set or mode, n_keys > MLDSA_SEED_MAX_KEYS,
 *   n_keys = 0 with n_ops > 0, key_idx = NULL with n_keys < n_ops, a NULL xi / msg_off / rnd / sigs, a NULL or misaligned scratch;
 *   MLDSA_ERR_NOMEM for a scratch below the table plus the smallest expansion pass.  n_ops = 0 returns MLDSA_OK and launches
 *   nothing. */
int mldsa_sign_seed(mldsa_ctx *ctx, int set, int mode, const uint8_t *xi, size_t n_keys, const uint32_t *key_idx, const uint8_t *msgs,
                    const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sigs,
                    int32_t *status /* may be NULL */, size_t n_ops, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_SEED_H */
