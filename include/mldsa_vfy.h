/* mldsa_vfy.h -- the large-batch, device-resident verify pass as a layered library (libmldsa_vfy.so).
 *
 * mldsa_vfy_verify is mldsa_verify (mldsa_hip.h) for calls of many ops: same arguments, same verdicts, same refusal rules, ordered on
 * the caller's stream.  It differs in how the pass is run:
 *   - ExpandA, which is 70 % of such a call and bound by its own instruction count, runs on a Keccak round of 180 instead of 190
 *     vector instructions (fips204_amd/vfy/keccak180.h);
 *   - the call is cut into parts of MLDSA_VFY_PART_OPS ops.  A call of one part -- every call up to that size -- is one chain on the
 *     caller's stream (ExpandA, the arithmetic, the c~ hash) with the key-index check, mu and SampleInBall on one library-owned stream
 *     beside ExpandA.  In a call of several parts ExpandA of part p + 1 runs on one library-owned stream while the arithmetic and the c~
 *     hash of part p run on another, and the A_hat scratch is a ring of two parts instead of one row set per op.  Stream events alone
 *     order the streams, and the caller's stream ends behind all of the call either way;
 *   - the scratch is the caller's.
 * A_hat is derived again for every op, key table or not, as mldsa_verify does.
 * The formats are the core's: A_hat in the packed 24-bit form (768 bytes per polynomial), c as one byte per coefficient, rows of
 * mu | w1.  This pass folds back into the core library when the core's profile set is next collected.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers, key_idx[op] < n_keys selects the key of an op
 * (NULL: op i uses key i), `stream` is a hipStream_t (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and
 * never abort, every call launches on mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported
 * before anything is launched.
 */
#ifndef MLDSA_VFY_H
#define MLDSA_VFY_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_VFY_ABI_VERSION 1
/* most operations of one call */
#define MLDSA_VFY_MAX_OPS ((size_t)1 << 22)
/* Ops of one part.  A call of at most this many ops is one part, and runs as one chain on the caller's stream
 * (profiles/vfy_chain_ab.jsonl).  Measured among call / {1, 2, 4, 8} at 65 536 and 131 072 ops (profiles/vfy_layer_ab.jsonl, DESIGN.md
 * section 6). */
#ifndef MLDSA_VFY_PART_OPS
#define MLDSA_VFY_PART_OPS 65536
#endif

int mldsa_vfy_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_vfy_last_error(void);

/* Bytes of the scratch of a call of n_ops ops at the current part size: the A_hat ring (one or two parts of min(n_ops, part) x k x l
 * rows of 768 bytes) and 276 + 64 + w1_len bytes per op, every array rounded up to 256 bytes.  0 for an unknown set and for
 * n_ops > MLDSA_VFY_MAX_OPS. */
size_t mldsa_vfy_scratch_bytes(int set, size_t n_ops);

/* mldsa_verify on the caller's scratch.  ok[op] = 1 for a valid signature, 0 otherwise; an op with a key index outside the table, a
 * ctx longer than 255 bytes or a malformed offset pair is refused alone (ok = 0), as by mldsa_verify.  Asynchronous: the work is
 * ordered behind what `stream` holds at the call and `stream` is ordered behind all of it; the scratch is used in that order and holds
 * nothing secret.  One call at a time enqueues per process (a mutex); the library's two streams and its events live as long as the
 * process.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set or mode, a NULL rho / tr / t1_d2_hat_mont /
 *   msg_off / sigs / ok, n_keys that does not cover the batch (key_idx ? n_keys > 0 : n_keys >= n_ops; above 2^32 - 1 it is read as
 *   2^32 - 1, as by mldsa_verify), n_ops > MLDSA_VFY_MAX_OPS, a
 *   NULL or not 256-byte aligned scratch.  MLDSA_ERR_NOMEM: scratch_bytes < mldsa_vfy_scratch_bytes(set, n_ops).  n_ops = 0 returns
 *   MLDSA_OK. */
int mldsa_vfy_verify(mldsa_ctx *ctx, int set, int mode, const uint8_t *rho, const uint8_t *tr, const int32_t *t1_d2_hat_mont,
                     size_t n_keys, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs,
                     const uint64_t *ctx_off, const uint8_t *sigs, uint8_t *ok, size_t n_ops, void *scratch, size_t scratch_bytes,
                     void *stream);

/* Test seam: the library's ExpandA kernel on rho[n_ops][32], then its packed rows unpacked to the int32 rows of mldsa_expand_a
 * (a_hat[n_ops][k][l][256]).  Allocates and frees its packed rows itself and waits for the stream. */
int mldsa_vfy_expand_a(mldsa_ctx *ctx, int set, const uint8_t *rho, int32_t *a_hat, size_t n_ops, void *stream);

/* Test and measurement knob, NOT for production use: ops per part of the calls that follow, process-wide (0 = MLDSA_VFY_PART_OPS
 * again).  Returns the value in force before.  It changes what mldsa_vfy_scratch_bytes returns: a scratch sized before a change may be
 * too small after it, which mldsa_vfy_verify answers with MLDSA_ERR_NOMEM before anything is launched. */
size_t mldsa_vfy_set_part_ops(size_t part_ops);

/* Per-stage timing as mldsa_profile_enable / mldsa_profile_report give it for the core: event pairs around the launches of the calls
 * made on the context's device while enabled, resolved by the report, which waits for the device and starts the record afresh.  The
 * report is a JSON object {"stage": {"ms": total, "calls": launches}}; the stages carry the core's names: expand_a, verify_main,
 * ctilde_hash, mu, sample_in_ball (one launch of each per part).  At most 4 096 launches are kept between two reports. */
int mldsa_vfy_profile_enable(mldsa_ctx *ctx, int on);
int mldsa_vfy_profile_report(mldsa_ctx *ctx, char *buf, size_t buf_len);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_VFY_H */
