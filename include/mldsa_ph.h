/* mldsa_ph.h -- HashML-DSA with the pre-hash on the GPU (libmldsa_ph.so).
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h.  It computes PH(M) -- SHA-256, SHA-512 or
 * SHAKE128 of each raw message, the reference's hash_message (src/hashing.rs:316-354), or one of the nine other
 * functions of the NIST hash OID arc (MLDSA_PH_* below) -- in one kernel, one
 * message per lane, writes OID || PH(M) for every operation into caller-provided device scratch, and then calls
 * mldsa_verify / mldsa_verify_pk / mldsa_sign with MLDSA_MODE_PREHASH on the same stream.  It reaches the core
 * only through the core's public entry points, so every core call's behaviour is the core's.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are device pointers, `stream` is a
 * hipStream_t (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort.
 *
 * Argument errors: an unknown `ph`, a NULL pointer the call needs while n_ops > 0, or `scratch` that is NULL,
 *   not 8-byte aligned or smaller than mldsa_ph_scratch_bytes(ph, n_ops) return MLDSA_ERR_PARAM before anything
 *   is launched.  n_ops = 0 returns MLDSA_OK.  Errors of the core call pass through with their code, and
 *   mldsa_ph_last_error() then carries the core's message.
 * Offsets are untrusted, with the rule of mldsa_verify: an op whose message pair is not in order inside
 *   [msg_off[0], msg_off[n_ops]], or that names bytes of a NULL `msgs`, is refused on its own -- ok = 0, status
 *   MLDSA_ERR_PARAM and an all-zero signature -- and no byte of its message is read.  An op whose ctx pair is
 *   malformed or whose ctx is longer than 255 bytes is not hashed either (no byte of its message is read) and
 *   gets the core's result: ok = 0 / MLDSA_ERR_CTX_LEN (lib.rs:274, 368).  A malformed message pair takes
 *   precedence over |ctx| > 255, as in the core.  Other ops are unaffected.
 * Device and stream: every call launches on mldsa_ctx_device(ctx) and restores the caller's current device.
 *   mldsa_prehash and the verify calls are asynchronous on `stream` and never synchronise the host;
 *   mldsa_hash_sign is synchronous like mldsa_sign: signatures and statuses are final when it returns.
 *   Scratch is used in stream order on `stream`: it may be reused by the next call on the same stream.
 *
 * Messages that arrive in pieces, or that are too large to hold on the device at once, go through the incremental
 *   pre-hash (mldsa_ph_init / _update / _final below); messages, keys and signatures that lie in HOST memory go through
 *   mldsa_hash_verify_host / mldsa_hash_sign_host, which stream the message bytes through a bounded staging buffer.
 */
#ifndef MLDSA_PH_H
#define MLDSA_PH_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_PH_ABI_VERSION 1
#define MLDSA_PH_SHA256 0   /* OID 2.16.840.1.101.3.4.2.1,  32-byte digest (hashing.rs:319-329) */
#define MLDSA_PH_SHA512 1   /* OID 2.16.840.1.101.3.4.2.3,  64-byte digest (hashing.rs:330-340) */
#define MLDSA_PH_SHAKE128 2 /* OID 2.16.840.1.101.3.4.2.11, 32 bytes of output (hashing.rs:341-352) */
/* The other functions of the NIST arc 2.16.840.1.101.3.4.2.* (FIPS 204 §5.4 allows any approved hash or XOF): code = 16 + the
 * last OID arc.  0, 1, 2 keep their meaning; 3-15 and every other value are unknown.  The library does not police FIPS 204's
 * strength recommendation (e.g. SHA-224 with ML-DSA-87), as the reference does not for SHA-256. */
#define MLDSA_PH_SHA384 18     /* ...4.2.2,  48-byte digest */
#define MLDSA_PH_SHA224 20     /* ...4.2.4,  28-byte digest */
#define MLDSA_PH_SHA512_224 21 /* ...4.2.5,  28-byte digest */
#define MLDSA_PH_SHA512_256 22 /* ...4.2.6,  32-byte digest */
#define MLDSA_PH_SHA3_224 23   /* ...4.2.7,  28-byte digest */
#define MLDSA_PH_SHA3_256 24   /* ...4.2.8,  32-byte digest */
#define MLDSA_PH_SHA3_384 25   /* ...4.2.9,  48-byte digest */
#define MLDSA_PH_SHA3_512 26   /* ...4.2.10, 64-byte digest */
#define MLDSA_PH_SHAKE256 28   /* ...4.2.12, 64 bytes of output (FIPS 204: 512 bits) */

/* One-shot calls (mldsa_prehash, mldsa_hash_verify, mldsa_hash_verify_pk, mldsa_hash_sign) of at most this many operations
 * run the six Keccak-family functions one message per WAVE on the core's cooperative sponge instead of one per lane; rows,
 * refusals and the offset table are the same bytes in either form.  A compile-time constant of the library (0: never).
 * Measured (profiles/prehash_fips_list_bench.jsonl, "prehash_small_call", SHAKE256 / SHA3-512 / SHAKE128 at 1 KiB and 16 KiB,
 * n = 1 ... 4096): the wave form's median latency of mldsa_prehash and of mldsa_hash_verify is below the lane form's by more
 * than the lane form's p10-p90 spread at every n measured; 4096 is the largest of them (there: 68 against 94 us at 1 KiB). */
#ifndef MLDSA_PH_COOP_MAX_OPS
#define MLDSA_PH_COOP_MAX_OPS 4096
#endif

int mldsa_ph_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_ph_last_error(void);
/* 11-byte DER OID + digest: 43 / 75 / 43 for the codes 0 / 1 / 2, 39 / 43 / 59 / 75 for 28- / 32- / 48- / 64-byte digests;
 * negative for an unknown ph */
int mldsa_ph_row_len(int ph);
/* device scratch the op-level calls need for n_ops operations: 8 (n_ops + 1) + n_ops row_len + n_ops bytes;
 * 0 for an unknown ph (or a size that does not fit a size_t) */
size_t mldsa_ph_scratch_bytes(int ph, size_t n_ops);

/* The seam: out[n_ops][row_len] = OID || PH(M_i) for the messages msgs[msg_off[i], msg_off[i + 1]).  An op with a
 * malformed pair gets an all-zero row and bad[i] = 1 (else bad[i] = 0); bad may be NULL.  Asynchronous on stream. */
int mldsa_prehash(mldsa_ctx *ctx, int ph, const uint8_t *msgs, const uint64_t *msg_off, uint8_t *out, uint8_t *bad,
                  size_t n_ops, void *stream);

/* HashML-DSA.Verify / .Sign (src/lib.rs:391-411, 310-342) on RAW messages: arguments, refusal rules and results are
 * those of mldsa_verify / mldsa_verify_pk / mldsa_sign with mode = MLDSA_MODE_PREHASH and msg_i = OID || PH(M_i),
 * plus ph and a caller-owned device scratch of >= mldsa_ph_scratch_bytes(ph, n_ops) bytes. */
int mldsa_hash_verify(mldsa_ctx *ctx, int set, int ph, const uint8_t *rho, const uint8_t *tr, const int32_t *t1_d2_hat_mont,
                      size_t n_keys, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off,
                      const uint8_t *ctxs, const uint64_t *ctx_off, const uint8_t *sigs, uint8_t *ok, size_t n_ops,
                      void *scratch, size_t scratch_bytes, void *stream);
int mldsa_hash_verify_pk(mldsa_ctx *ctx, int set, int ph, const uint8_t *pk, size_t n_keys, const uint32_t *key_idx,
                         const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off,
                         const uint8_t *sigs, uint8_t *ok, size_t n_ops, void *scratch, size_t scratch_bytes, void *stream);
int mldsa_hash_sign(mldsa_ctx *ctx, int set, int ph, const uint8_t *rho, const uint8_t *cap_k, const uint8_t *tr,
                    const int32_t *s_1_hat_mont, const int32_t *s_2_hat_mont, const int32_t *t_0_hat_mont, size_t n_keys,
                    const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs,
                    const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sigs, int32_t *status, size_t n_ops,
                    void *scratch, size_t scratch_bytes, void *stream);

/* ---- incremental pre-hash: init / update / final ------------------------------------------------------------
 * PH(M) of n_ops messages that arrive in pieces, one operation per lane.  The hash states of the operations live in
 * caller-owned device memory between the calls: `state`, at least mldsa_ph_state_bytes(ph, n_ops) bytes, 8-byte aligned,
 * opaque (its layout depends on n_ops: a state belongs to the (ph, n_ops) it was initialised with, and every call on it
 * passes the same two values).  The length of a message is a 64-bit byte count.
 *   mldsa_ph_init    fresh states: the empty message, not bad.
 *   mldsa_ph_update  op i absorbs the piece pieces[piece_off[i], piece_off[i + 1]); n_ops + 1 offsets on the device.  An
 *                    empty piece is a no-op.  Pieces may be cut at any byte position and lie at any byte alignment.
 *   mldsa_ph_final   pads and finishes: out[n_ops][row_len] = OID || PH(M_i), the row format of mldsa_prehash; bad[i]
 *                    (bad may be NULL); and, when out_off != NULL, the n_ops + 1 offsets i row_len that the core's
 *                    MLDSA_MODE_PREHASH call reads.  The states are not changed: init starts the next messages.
 * For every way of cutting the messages into pieces the rows are those of mldsa_prehash on the whole messages.
 * Offsets are untrusted, with the rule of mldsa_prehash: a piece pair that is not in order inside
 *   [piece_off[0], piece_off[n_ops]], or that names bytes of a NULL `pieces`, reads nothing and marks its op bad.  Bad is
 *   sticky across later updates (no further byte of that op is read); final gives such an op an all-zero row and
 *   bad[i] = 1.  Other ops are unaffected.  Nothing outside [piece_off[0], piece_off[n_ops]) is read and nothing outside
 *   the first mldsa_ph_state_bytes(ph, n_ops) bytes of `state` is touched.
 * Argument errors: unknown ph, NULL ctx, a NULL or misaligned `state`, state_bytes < mldsa_ph_state_bytes(ph, n_ops), a
 *   NULL piece_off / out return MLDSA_ERR_PARAM before anything is launched; n_ops = 0 returns MLDSA_OK.
 * All three calls are asynchronous on `stream`, never synchronise the host, launch on mldsa_ctx_device(ctx) and restore
 *   the caller's current device.  The state is used in stream order. */
/* bytes of device memory for the states of n_ops operations; 0 for an unknown ph or a size that does not fit */
size_t mldsa_ph_state_bytes(int ph, size_t n_ops);
int mldsa_ph_init(mldsa_ctx *ctx, int ph, void *state, size_t state_bytes, size_t n_ops, void *stream);
int mldsa_ph_update(mldsa_ctx *ctx, int ph, void *state, size_t state_bytes, const uint8_t *pieces, const uint64_t *piece_off,
                    size_t n_ops, void *stream);
int mldsa_ph_final(mldsa_ctx *ctx, int ph, void *state, size_t state_bytes, uint8_t *out, uint64_t *out_off, uint8_t *bad,
                   size_t n_ops, void *stream);

/* ---- HashML-DSA from host memory ----------------------------------------------------------------------------
 * Raw messages, wire-format keys, signatures and results in HOST memory: arguments and results are those of
 * mldsa_verify_host / mldsa_sign_host with `ph` in place of `mode`.  A mldsa_ph_host owns what the calls need besides the
 * context: two staging chunks of `staging_bytes` each on the device, two page-locked ones on the host, a copy and a
 * compute stream, and the per-batch buffers (offsets, hash states, rows), which grow with the largest n_ops seen.
 *   The message bytes [msg_off[0], msg_off[n_ops]) are cut into chunks of at most staging_bytes at arbitrary byte
 *   positions -- a message may span any number of chunks, a chunk may hold thousands of messages -- and chunk i + 1 is
 *   uploaded while mldsa_ph_update runs on chunk i, for the ops that have bytes in it.  The device memory of a call is
 *   2 staging_bytes + states + rows + one offset table, whatever the size of the messages.  After mldsa_ph_final the rows
 *   (39 ... 75 bytes per op) are brought to the host and mldsa_verify_host / mldsa_sign_host run in MLDSA_MODE_PREHASH:
 *   verdicts, signatures, statuses and per-op refusals are the core's.
 * Refusal rules are those of the core's *_host calls: both offset tables are checked first (mldsa_check_offsets) and a
 *   malformed table, or a msg_off that names bytes of a NULL msgs, fails the whole call with MLDSA_ERR_PARAM before a
 *   message byte is read; an op whose ctx is longer than 255 bytes gets ok = 0 / MLDSA_ERR_CTX_LEN from the core.
 * Page-locked caller memory (mldsa_host_alloc) is copied by DMA where it lies, pageable memory goes through the
 *   page-locked chunks.  A call returns when the results are in the caller's buffers.  One call at a time per
 *   mldsa_ph_host (the calls take its mutex); objects on different contexts are independent.  No call may be made on
 *   an object whose context has been destroyed; mldsa_ph_host_destroy itself does not need the context. */
typedef struct mldsa_ph_host mldsa_ph_host;
/* staging_bytes: size of ONE message staging chunk (two are kept, device + page-locked); 0 = the library's default */
int mldsa_ph_host_create(mldsa_ctx *ctx, size_t staging_bytes, mldsa_ph_host **out);
void mldsa_ph_host_destroy(mldsa_ph_host *h); /* NULL: no-op */
int mldsa_hash_verify_host(mldsa_ph_host *h, int set, int ph, const uint8_t *pk, size_t n_keys, const uint32_t *key_idx,
                           const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off,
                           const uint8_t *sigs, uint8_t *ok, size_t n_ops);
int mldsa_hash_sign_host(mldsa_ph_host *h, int set, int ph, const uint8_t *sk, size_t n_keys, const uint32_t *key_idx,
                         const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off,
                         const uint8_t *rnd, uint8_t *sigs, int32_t *status, size_t n_ops);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_PH_H */
