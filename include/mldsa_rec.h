/* mldsa_rec.h -- batched verification straight from serialized records on the device (libmldsa_rec.so).
 *
 * A verification service holds a buffer of wire records -- transactions, log entries, certificates -- in which each record carries its
 * public key, its signature and its message at positions the parser knows, at arbitrary alignment, under a parameter set that differs
 * from record to record.  Every verify entry point of mldsa_hip.h wants one set per call, pk[n][PK_LEN] dense and 16-byte aligned,
 * sigs[n][SIG_LEN] dense and the messages concatenated behind n + 1 offsets.  This library does that split where the bytes already
 * lie: it takes the buffer (the blob) and one descriptor per op, any mix of ML-DSA-44 / 65 / 87, sorts the ops by parameter set,
 * packs each set's dense arrays on the device and returns one verdict per op.  The verdicts are mldsa_verify_pk's.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only and reaches it only through
 * mldsa_verify_pk and the public helpers, so every verdict, refusal rule and precedence is the core's.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.
 *
 * Public data only: keys, signatures, messages and contexts of verification.  The scratch holds nothing else and is not cleared.
 */
#ifndef MLDSA_REC_H
#define MLDSA_REC_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_REC_ABI_VERSION 1
/* most ops of one call: a slot is 30 bits of a class_slot word */
#define MLDSA_REC_MAX_OPS ((size_t)1 << 30)
/* ops per workgroup of the classify and apply passes (one op per thread): the unit of the scan */
#define MLDSA_REC_SCAN_BLOCK 256

/* ---- the descriptor: one per op, a device array, 8-byte aligned, 40 bytes each -------------------------------------------------------
 * The four offsets are byte offsets into the blob, uint8[blob_len] in device memory with NO alignment requirement.  The key is PK_LEN
 * and the signature SIG_LEN bytes of the op's set.  Ranges of different ops, and of one op, may overlap or coincide (several records
 * signing one message, one key under many signatures).  In MLDSA_MODE_PREHASH the message field is OID | PH(M), as in the core.
 *
 * Descriptor and blob are untrusted.  An op is REFUSED alone -- ok = 0, and not one byte of the blob is read for it -- when
 *   its set is none of MLDSA_44 / MLDSA_65 / MLDSA_87, its reserved byte is nonzero, its ctx_len exceeds 255 (the core's rule), or
 *   any of its four ranges [off, off + len) does not lie inside [0, blob_len): the test is off <= blob_len && len <= blob_len - off,
 *   which no 64-bit wrap gets past.  (An empty range is accepted wherever off <= blob_len.)
 * No byte outside [blob, blob + blob_len) is ever read, the aligned wide loads at a field's ends included. */
typedef struct {
    uint64_t pk_off, sig_off, msg_off, ctx_off;
    uint32_t msg_len;
    uint16_t ctx_len;
    uint8_t set;      /* MLDSA_44, MLDSA_65 or MLDSA_87 */
    uint8_t reserved; /* must be 0 */
} mldsa_rec_op;

/* classes of a class_slot word: (class << 30) | slot */
#define MLDSA_REC_CLASS_44 0
#define MLDSA_REC_CLASS_65 1
#define MLDSA_REC_CLASS_87 2
#define MLDSA_REC_CLASS_REFUSED 3

/* what the plan counts, one struct in device memory (8-byte aligned): ops per class (44, 65, 87, refused) and, per accepted class, the
 * message and context bytes of its ops as 64-bit sums (a message shared by several ops counts once per op: the sums may exceed blob_len) */
typedef struct {
    uint64_t n[4];
    uint64_t msg_bytes[3];
    uint64_t ctx_bytes[3];
} mldsa_rec_totals;

int mldsa_rec_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_rec_last_error(void);

/* ---- 1. the plan: class and slot of every op ------------------------------------------------------------------------------------------
 *   class_slot[i]  (class << 30) | slot: the op's class and its row among the ops of that class.  Slots are given by a stable exclusive
 *                  scan over the ops in input order -- op i's slot is the number of ops j < i of the same class -- not by arrival
 *                  counters, so the result does not depend on how the waves were scheduled.  Refused ops are numbered likewise.
 *   totals         see mldsa_rec_totals.
 *   plan           the plan's working memory, mldsa_rec_plan_bytes(n_ops) bytes, 256-byte aligned.  mldsa_rec_pack reads it: besides
 *                  the per-block sums of the scan it holds, for every op, where its message and its context begin among the
 *                  concatenated messages and contexts of its class (the same scan, over msg_len and ctx_len).
 * Asynchronous on `stream`, never waits for the host: three launches ordered by the kernel boundaries.  k_classify (one op per thread,
 *   MLDSA_REC_SCAN_BLOCK per workgroup) checks each descriptor and writes ten sums per workgroup; k_offsets (one wave per sum) turns
 *   them into exclusive prefixes and the totals; k_apply scans inside each workgroup and writes class_slot and the two positions.  No kernel
 *   waits on another workgroup and every loop runs to a count the host passed.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, blob (with blob_len > 0), ops, class_slot, totals or plan, ops or totals not 8-byte
 *   aligned, class_slot not 4-byte aligned, plan not 256-byte aligned or smaller than mldsa_rec_plan_bytes, n_ops > MLDSA_REC_MAX_OPS.
 *   n_ops = 0 returns MLDSA_OK and writes nothing. */
int mldsa_rec_plan(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_rec_op *ops, size_t n_ops, uint32_t *class_slot,
                   mldsa_rec_totals *totals, void *plan, size_t plan_bytes, void *stream);
/* With R(x) = x rounded up to a multiple of 256 and B = ceil(n_ops / MLDSA_REC_SCAN_BLOCK) workgroups:
 *   R(80 B) + 2 R(8 n_ops)            ten 64-bit sums per workgroup; message and context position of every op
 * 0 for n_ops > MLDSA_REC_MAX_OPS. */
size_t mldsa_rec_plan_bytes(size_t n_ops);

/* ---- 2. the pack: each class's dense arrays -------------------------------------------------------------------------------------------
 * Given the totals as the HOST read them, carves `arena` and fills, for each class c with n_c ops,
 *   pk[n_c][PK_LEN]            256-byte (so 16-byte) aligned
 *   sigs[n_c][SIG_LEN]         packed
 *   msgs, msg_off[n_c + 1]     the class's messages in slot order behind their offsets; likewise ctxs, ctx_off[n_c + 1]
 *   ok[n_c]                    room for the class's verdicts (not written here)
 * exactly as mldsa_verify_pk, mldsa_verify_pk_dedup (mldsa_keys.h) or mldsa_hash_verify_pk (mldsa_ph.h) take them: `out` (host memory)
 * receives the device pointers and counts, and is the seam a caller feeds to those calls itself.  Refused ops are skipped.
 * One launch, one wave per op.  Each of the op's four fields is copied by the plan of fips204_amd/rec/rec_plan.h: bytes one by one up
 *   to the destination's first 16-byte boundary, then 16-byte chunks -- aligned 16-byte loads, funnel-shifted in registers by the
 *   difference between source and destination alignment (one load per chunk when the two agree), aligned 16-byte stores --, then the
 *   rest one by one.  The kernel checks every descriptor again and drops an op whose class, slot or positions disagree with the counts
 *   the host passed, so a plan that was tampered with writes nothing outside the arena and reads nothing outside the blob.
 * Argument errors (MLDSA_ERR_PARAM): NULL pointers as for the plan, a NULL totals or out, counts that do not add up to n_ops, arena
 *   NULL or not 256-byte aligned; MLDSA_ERR_NOMEM: arena_bytes < mldsa_rec_scratch_bytes of the totals.  n_ops = 0 returns MLDSA_OK
 *   with an all-zero *out. */
typedef struct {
    size_t n; /* ops of the class; the pointers are valid, and the offset tables hold n + 1 entries, also when n = 0 */
    uint8_t *pk, *sigs, *msgs, *ctxs, *ok;
    uint64_t *msg_off, *ctx_off;
} mldsa_rec_class;
typedef struct {
    mldsa_rec_class c[3]; /* MLDSA_REC_CLASS_44, _65, _87 */
} mldsa_rec_packed;
int mldsa_rec_pack(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, const mldsa_rec_op *ops, size_t n_ops,
                   const uint32_t *class_slot, const void *plan, size_t plan_bytes, const mldsa_rec_totals *totals /* host */,
                   void *arena, size_t arena_bytes, mldsa_rec_packed *out /* host */, void *stream);
/* The arena of a known mix, exactly.  With R as above, PK_c / SIG_c the lengths of class c and n_c its ops:
 *   sum over c = 44, 65, 87 of  R(n_c PK_c) + R(n_c SIG_c) + 2 R(8 (n_c + 1)) + R(n_c)      pk, sigs, two offset tables, ok
 *   + R(msg_bytes) + R(ctx_bytes)                  the three classes' messages, then their contexts, back to back in class order
 * msg_bytes and ctx_bytes are the sums over the three classes.  0 when a count exceeds MLDSA_REC_MAX_OPS or the size does not fit. */
size_t mldsa_rec_scratch_bytes(size_t n44, size_t n65, size_t n87, uint64_t msg_bytes, uint64_t ctx_bytes);
/* A bound for an unknown mix of n_ops ops: at least mldsa_rec_scratch_bytes of every mix with n44 + n65 + n87 <= n_ops.
 *   R(2592 n_ops) + R(4627 n_ops) + 2 R(8 n_ops + 24) + R(n_ops) + 5 * 512 + R(msg_bytes) + R(ctx_bytes)
 * (every op sized as ML-DSA-87; 512 bytes per array for the rounding of the two other classes).  0 as above. */
size_t mldsa_rec_scratch_bytes_max(size_t n_ops, uint64_t msg_bytes, uint64_t ctx_bytes);

/* ---- 3. the whole pass ------------------------------------------------------------------------------------------------------------------
 * ok[i] = the verdict mldsa_verify_pk gives op i's key, message, context and signature under the op's set and `mode` (MLDSA_MODE_*, one
 * per call); 0 for a refused op.
 *   1. mldsa_rec_plan on `stream`.
 *   2. The call WAITS for `stream` once, to read the totals.  This is its only host synchronisation; a caller that wants none, or that
 *      wants another verify call behind the seam, drives mldsa_rec_plan and mldsa_rec_pack itself.
 *   3. If scratch_bytes is less than the mix needs, the call returns MLDSA_ERR_NOMEM before anything more is launched: ok is not
 *      written and info->scratch_needed names the need.
 *   4. mldsa_rec_pack, then one mldsa_verify_pk(set_c, mode, pk_c, n_c, NULL, ...) per non-empty class on `stream`, then one launch
 *      that scatters ok[i] = ok_c[slot] (0 for a refused op).
 * scratch (256-byte aligned): mldsa_rec_front_bytes(n_ops) + mldsa_rec_scratch_bytes(the mix) bytes; with
 *   mldsa_rec_scratch_bytes_max in place of the latter the call cannot run out.  Used in stream order: the next call on the same stream
 *   may reuse it.
 * info (host memory, may be NULL) receives the totals and the scratch the call needs; it is filled whenever step 2 was reached.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, blob (with blob_len > 0), ops, ok or scratch, unknown mode, ops not 8-byte or scratch
 *   not 256-byte aligned, scratch_bytes < mldsa_rec_front_bytes(n_ops), n_ops > MLDSA_REC_MAX_OPS.  n_ops = 0 returns MLDSA_OK.  Errors of
 *   a core call pass through with their code, and mldsa_rec_last_error() then carries the core's message.
 *
 * Cost, from byte counts (an expectation): the pack reads and writes PK_LEN + SIG_LEN + |M| once each per op, about 0.7 GB for
 *   65 536 ML-DSA-65 ops.
 * Measured on an MI355X, 65 536 ops of 32-byte messages, records 5 mod 16 bytes apart (profiles/rec_bench.jsonl; medians of
 *   alternating runs; "copy" is a device-to-device copy of the bytes the pack moves, in the same run):
 *                                               ML-DSA-44   ML-DSA-65   ML-DSA-87   even three-way mix
 *     this call / mldsa_verify_pk on arrays
 *       packed beforehand                       1.157       1.100       1.068       1.091     (1.57 / 2.35 / 3.76 / 2.88 ms)
 *     plan + pack alone                         0.185 ms    0.210 ms    0.245 ms    0.233 ms
 *     plan + pack / copy                        2.05        1.64        1.41        1.81
 *     numpy repack + upload + mldsa_verify_pk
 *       on the host / this call                 32          27          23          30        (51 ... 87 ms)
 *   The seam moves 2.7 ... 3.9 TB/s read + written where the copy reaches 5.4 ... 5.5; what the call adds to mldsa_verify_pk is the
 *   seam plus at most 30 us for the wait and the scatter. */
typedef struct {
    uint64_t n[4];           /* ops per class: 44, 65, 87, refused */
    uint64_t msg_bytes;      /* message bytes of the accepted ops */
    uint64_t ctx_bytes;      /* context bytes of the accepted ops */
    uint64_t scratch_needed; /* mldsa_rec_front_bytes(n_ops) + mldsa_rec_scratch_bytes of this mix */
} mldsa_rec_info;
int mldsa_rec_verify(mldsa_ctx *ctx, int mode, const uint8_t *blob, uint64_t blob_len, const mldsa_rec_op *ops, size_t n_ops, uint8_t *ok,
                     void *scratch, size_t scratch_bytes, mldsa_rec_info *info /* host */, void *stream);
/* What mldsa_rec_verify keeps in front of the arena:  R(4 n_ops) + 256 + mldsa_rec_plan_bytes(n_ops)    class_slot, totals, plan.
 * 0 for n_ops > MLDSA_REC_MAX_OPS. */
size_t mldsa_rec_front_bytes(size_t n_ops);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_REC_H */
