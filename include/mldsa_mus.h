/* mldsa_mus.h -- the message representative mu of messages that arrive in pieces, on the device (libmldsa_mus.so; mus = mu stream).
 *
 * FIPS 204 allows mu = H(BytesToBits(tr) || M', 64) (Algorithm 7 line 6, Algorithm 8 line 7) to be computed outside the signer and the
 * verifier so that a message can be hashed as it arrives, without ever being held whole.  mldsa_mu_compute (mldsa_mu.h) needs every
 * message whole in device memory.  This library computes the same mu incrementally -- init / update / final on a SHAKE256 sponge per
 * operation kept in caller-owned device memory -- and, on top of that, from raw messages of any size in HOST memory through two bounded
 * staging chunks (mldsa_mus_host_compute).  The rows (mu, mu_flag) are byte for byte those of mldsa_mu_compute on the whole messages and
 * are what mldsa_verify_mu / mldsa_sign_mu take as they stand.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h, like libmldsa_mu.so: it links the core only.
 *
 * Conventions are those of mldsa_mu.h: pointers to operation data are DEVICE pointers (the host-memory call below says which of its
 * pointers are HOST pointers), key_idx[op] < n_keys selects the key of an op (NULL: op i uses key i), `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.
 *
 * State: caller-owned device memory, 8-byte aligned, opaque, mldsa_mus_state_bytes(n_ops) bytes, tied to the n_ops it was initialised
 * with, used in stream order.  Layout (for the record; both kernel forms read and write it): 52 32-bit words per op, word-major --
 * word w of op i at state[w * n_ops + i] --: word 0 the bytes in the current rate block (0 ... 135), word 1 the op's flag, words
 * 2 ... 51 the 25 lanes of the sponge as (lo, hi) pairs.  A partial block is XORed straight into the sponge: SHAKE needs no total length.
 */
#ifndef MLDSA_MUS_H
#define MLDSA_MUS_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_MUS_ABI_VERSION 1
/* most operations of one call */
#define MLDSA_MUS_MAX_OPS ((size_t)1 << 30)
/* Calls of at most this many ops run one op per WAVE on the core's cooperative sponge instead of one op per lane: a call of few ops
 * is a serial chain of permutations, and the cooperative permutation is the shorter one.  0 = never.  Both forms give the same bytes.
 * The value is the largest measured n (of 1, 64, 1024, 4096, 16384) at which the wave form's median is below the lane form's by more
 * than the lane form's p10 to p90 spread, for 1 KiB and for 16 KiB messages (tools/bench_mus.py --forms-dir, profiles/mu_stream_bench.jsonl:
 * init + update + final of 4096 x 1 KiB 75 against 108 us, of 16384 x 1 KiB 240 against 115 us). */
#ifndef MLDSA_MUS_WAVE_MAX_OPS
#define MLDSA_MUS_WAVE_MAX_OPS 4096
#endif

int mldsa_mus_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_mus_last_error(void);

/* bytes of the state of n_ops operations: 208 n_ops; 0 for n_ops > MLDSA_MUS_MAX_OPS */
size_t mldsa_mus_state_bytes(size_t n_ops);

/* Fresh states that have absorbed what precedes the message: tr (MLDSA_MODE_INTERNAL), tr | 0x00 | len(ctx) | ctx (MLDSA_MODE_PURE,
 * Algorithm 2 line 10) or tr | 0x01 | len(ctx) | ctx (MLDSA_MODE_PREHASH, Algorithm 4 line 23; the caller then streams OID | PH(M) as
 * the message): 64 to 321 bytes, at most two permutations.
 *   tr[n_keys][64], key_idx, ctxs / ctx_off (n_ops + 1 offsets; ctx_off NULL = every ctx empty) as for mldsa_mu_compute, untrusted
 *   alike: the call vouches for [ctx_off[0], ctx_off[n_ops]) and reads nothing else.
 *   The op's flag, with the precedence of mldsa_mu_compute: 2 = its ctx offset pair is not in order inside the call's range or names
 *   bytes of a NULL ctxs; then 1 = its ctx is longer than 255 bytes; then 2 = its key index is not below n_keys.  Nothing of a
 *   flagged op is read, now or later.
 * Asynchronous on `stream`.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown mode, a NULL tr / state, a misaligned state,
 *   state_bytes < mldsa_mus_state_bytes(n_ops), n_keys = 0, n_ops > MLDSA_MUS_MAX_OPS.  n_ops = 0 returns MLDSA_OK. */
int mldsa_mus_init(mldsa_ctx *ctx, int mode, const uint8_t *tr /* [n_keys][64] */, size_t n_keys, const uint32_t *key_idx,
                   const uint8_t *ctxs, const uint64_t *ctx_off /* NULL: every ctx empty */, void *state, size_t state_bytes,
                   size_t n_ops, void *stream);

/* Op i absorbs pieces[piece_off[i], piece_off[i + 1]) (n_ops + 1 offsets).  Pieces may be cut at any byte and lie at any alignment; an
 * empty piece is a no-op.  Offsets are untrusted, by the rule of mldsa_ph_update: a pair that is not in order inside
 * [piece_off[0], piece_off[n_ops]], or one that names bytes of a NULL `pieces`, reads nothing and sets flag 2 on the op unless the op
 * already carries a flag (the first flag stays).  Flags are sticky: a flagged op reads no further byte.  Other ops are unaffected.
 * Nothing outside [piece_off[0], piece_off[n_ops]) is read and nothing outside the first mldsa_mus_state_bytes(n_ops) bytes of `state`
 * is touched.  n_ops is the one the state was initialised with.  Asynchronous on `stream`.
 * Argument errors: as for mldsa_mus_init, with a NULL piece_off. */
int mldsa_mus_update(mldsa_ctx *ctx, void *state, size_t state_bytes, const uint8_t *pieces, const uint64_t *piece_off, size_t n_ops,
                     void *stream);

/* mu[op] = the 64 bytes squeezed from a padded COPY of the op's state (held in registers), mu_flag[op] = the op's flag.  A flagged
 * op's row is all zero.  The state itself is not changed: a later update + final gives the mu of the longer message, so a prefix can
 * be snapshotted.  Asynchronous on `stream`.
 * Argument errors: as for mldsa_mus_init, with a NULL mu. */
int mldsa_mus_final(mldsa_ctx *ctx, const void *state, size_t state_bytes, uint8_t *mu /* [n_ops][64] */,
                    int32_t *mu_flag /* [n_ops], may be NULL */, size_t n_ops, void *stream);

/* ---- raw messages of any size in host memory -> mu rows on the device ----
 * An mldsa_mus_host owns two device and two page-locked staging chunks of `staging_bytes` (0 = the library's default), a copy stream
 * and a compute stream, and the per-batch buffers (offset tables, ctxs, state), which grow with the largest n_ops seen. */
typedef struct mldsa_mus_host mldsa_mus_host;
int mldsa_mus_host_create(mldsa_ctx *ctx, size_t staging_bytes /* 0 = default */, mldsa_mus_host **out);
/* NULL: no-op.  Does not need the context. */
void mldsa_mus_host_destroy(mldsa_mus_host *h);

/* mu rows of n_ops messages that lie in HOST memory.
 *   HOST pointers: msgs / msg_off, ctxs / ctx_off (n_ops + 1 offsets each; ctx_off NULL = every ctx empty) -- the bulk.
 *   DEVICE pointers: tr[n_keys][64] and key_idx (may be NULL) -- mldsa_pk_expand / mldsa_sk_expand leave tr on the device --, and the
 *   results mu[n_ops][64] and mu_flag[n_ops] (may be NULL): the next call, mldsa_verify_mu / mldsa_sign_mu, reads them there.
 * The ctx table and the ctxs are uploaded whole (at most 255 useful bytes per op) and mldsa_mus_init runs; the bytes
 * [msg_off[0], msg_off[n_ops]) are cut into chunks of at most staging_bytes at arbitrary byte positions -- a message may span any
 * number of chunks, a chunk may hold thousands of messages --; chunk i + 1 is uploaded while the update runs on chunk i, for the ops
 * that have bytes in it only; then mldsa_mus_final runs.  Page-locked caller memory is copied by DMA where it lies, pageable memory
 * goes through the page-locked chunks.  Device memory per call: 2 staging_bytes + the state + the offset tables and ctxs, whatever the
 * message sizes.  Blocks: mu is complete when the call returns.  One call at a time per object (a mutex).  The work runs on the
 * object's own streams: tr and key_idx must be complete, and mu / mu_flag free of pending work, when the call is made.
 * Both offset tables are checked first (mldsa_check_offsets): a malformed table, or a msg_off that names bytes of a NULL msgs, fails
 * the whole call with MLDSA_ERR_PARAM before a byte is read and leaves mu untouched.  A ctx longer than 255 bytes gives flag 1 on
 * that op; a key index not below n_keys flag 2.
 * Argument errors: MLDSA_ERR_PARAM for a NULL object, unknown mode, a NULL tr / msg_off / mu, n_keys = 0, n_ops > MLDSA_MUS_MAX_OPS.
 *   n_ops = 0 returns MLDSA_OK. */
int mldsa_mus_host_compute(mldsa_mus_host *h, int mode, const uint8_t *tr /* DEVICE [n_keys][64] */, size_t n_keys,
                           const uint32_t *key_idx /* DEVICE, may be NULL */, const uint8_t *msgs, const uint64_t *msg_off,
                           const uint8_t *ctxs, const uint64_t *ctx_off /* HOST */, uint8_t *mu /* DEVICE [n_ops][64] */,
                           int32_t *mu_flag /* DEVICE, may be NULL */, size_t n_ops);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_MUS_H */
