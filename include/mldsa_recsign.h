/* mldsa_recsign.h -- batched signing of serialized request records on the device (libmldsa_recsign.so).
 *
 * A signing service holds a buffer of requests -- transactions, log entries, to-be-signed certificates -- under keys of different
 * parameter sets, with messages and contexts at arbitrary offsets, and each signature must end up in a hole inside its record, at an
 * odd offset.  mldsa_sign of mldsa_hip.h and every route on top of it want one set per call and dense arrays: msgs behind n + 1
 * offsets, rnd[n][32], key_idx[n], and they return sigs[n][SIG_LEN] dense.  This library does that split, and the way back, where the
 * bytes already lie: it takes the buffer (the blob) and one descriptor per op, any mix of ML-DSA-44 / 65 / 87, sorts the ops by
 * parameter set, packs what mldsa_sign wants on the device, signs each set from a device-resident key table and writes every signature
 * to its byte offset in an output buffer, which may be the blob itself.  It is the signing counterpart of mldsa_rec.h.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h: it links the core only and reaches it only through mldsa_sign and
 * the public helpers, so every signature byte and every per-op status of an accepted op is the core's.  No key material is copied: the
 * key tables stay where the caller put them and are handed to mldsa_sign as they are.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are DEVICE pointers unless marked host, `stream` is a hipStream_t
 * (NULL = the default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on
 * mldsa_ctx_device(ctx) and restores the caller's current device.  Argument errors are reported before anything is launched.
 *
 * Secrets: the per-signature randomness rnd is the ONLY secret the scratch ever holds (messages, contexts, key indices, signatures and
 * status words are public; the keys are never copied).  mldsa_recsign_sign zeroes the arena's rnd rows in stream order before it
 * returns, whatever its return code; a caller that drives the seam itself clears mldsa_recsign_packed.rnd_region likewise.
 */
#ifndef MLDSA_RECSIGN_H
#define MLDSA_RECSIGN_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_RECSIGN_ABI_VERSION 1
/* most ops of one call: a slot is 30 bits of a class_slot word */
#define MLDSA_RECSIGN_MAX_OPS ((size_t)1 << 30)
/* ops per workgroup of the classify and apply passes (one op per thread): the unit of the scan */
#define MLDSA_RECSIGN_SCAN_BLOCK 256
/* flags bit 0: the op's 32 bytes of randomness lie at rnd_off in the blob */
#define MLDSA_RECSIGN_RND 1

/* ---- the descriptor: one per op, a device array, 8-byte aligned, 48 bytes each -------------------------------------------------------
 * msg_off, ctx_off and rnd_off are byte offsets into the blob, uint8[blob_len] in device memory; sig_off is a byte offset into the
 * output buffer, uint8[out_len].  Neither buffer has an alignment requirement.  The signature written is SIG_LEN bytes of the op's set.
 * With MLDSA_RECSIGN_RND clear, rnd is all zero (the deterministic variant) and rnd_off is neither followed nor checked.  Message,
 * context and rnd ranges of different ops may overlap or coincide.  In MLDSA_MODE_PREHASH the message field is OID | PH(M), as in the
 * core.  `key` is the row of the op's set's key table.
 *
 * Descriptor and blob are untrusted.  An op is REFUSED alone; for a refused op not one byte of the blob is read and not one byte of
 * `out` is written, and its status is the code of the first rule it breaks, tested in this order:
 *   1. its set is none of MLDSA_44 / MLDSA_65 / MLDSA_87, a flag bit other than bit 0 is set, or reserved is nonzero: MLDSA_ERR_PARAM
 *   2. ctx_len > 255: MLDSA_ERR_CTX_LEN (the core's code for it)
 *   3. key >= n_keys of its set (a set with n_keys = 0 is not served: all its ops are refused): MLDSA_ERR_PARAM
 *   4. its message, context or (with the flag) rnd range [off, off + len) does not lie inside [0, blob_len): MLDSA_ERR_PARAM
 *   5. [sig_off, sig_off + SIG_LEN) does not lie inside [0, out_len): MLDSA_ERR_PARAM
 * The range test is off <= size && len <= size - off, which no 64-bit wrap gets past (an empty range is accepted wherever
 * off <= size).  The rules are one function, check_op of fips204_amd/recsign/recsign_plan.h.
 * No byte outside [blob, blob + blob_len) is ever read and none outside the accepted ops' signature ranges is ever written, the
 * aligned wide accesses at a field's ends included. */
typedef struct {
    uint64_t msg_off, ctx_off, rnd_off; /* byte offsets into blob[blob_len] */
    uint64_t sig_off;                   /* byte offset into out[out_len] */
    uint32_t msg_len, key;              /* key = row of the op's set's key table */
    uint16_t ctx_len;
    uint8_t set;                        /* MLDSA_44, MLDSA_65 or MLDSA_87 */
    uint8_t flags;
    uint32_t reserved;                  /* must be 0 */
} mldsa_recsign_op;

/* classes of a class_slot word: (class << 30) | slot */
#define MLDSA_RECSIGN_CLASS_44 0
#define MLDSA_RECSIGN_CLASS_65 1
#define MLDSA_RECSIGN_CLASS_87 2
#define MLDSA_RECSIGN_CLASS_REFUSED 3

/* ---- the key tables: a HOST array of three, class order 44 / 65 / 87 --------------------------------------------------------------
 * n_keys expanded private keys, field by field, exactly the six device pointers mldsa_sign takes (from mldsa_sk_expand).  A set with
 * n_keys = 0 is not served and its pointers are not looked at; a served set with a NULL pointer is an argument error.  n_keys above
 * UINT32_MAX is an argument error (a descriptor's key is 32 bits). */
typedef struct {
    size_t n_keys;
    const uint8_t *rho, *cap_k, *tr;
    const int32_t *s_1_hat_mont, *s_2_hat_mont, *t_0_hat_mont;
} mldsa_recsign_keys;

/* what the plan counts, one struct in device memory (8-byte aligned): ops per class (44, 65, 87, refused) and, per accepted class, the
 * message and context bytes of its ops as 64-bit sums (a message shared by several ops counts once per op) */
typedef struct {
    uint64_t n[4];
    uint64_t msg_bytes[3];
    uint64_t ctx_bytes[3];
} mldsa_recsign_totals;

int mldsa_recsign_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_recsign_last_error(void);

/* ---- 1. the plan: class and slot of every op ------------------------------------------------------------------------------------------
 *   n_keys         HOST array of three: the rows of the key tables in class order (rule 3).
 *   class_slot[i]  (class << 30) | slot: the op's class and its row among the ops of that class.  Slots are given by a stable exclusive
 *                  scan over the ops in input order -- op i's slot is the number of ops j < i of the same class.  Refused ops are
 *                  numbered likewise.
 *   totals         see mldsa_recsign_totals.
 *   plan           the plan's working memory, mldsa_recsign_plan_bytes(n_ops) bytes, 256-byte aligned.  mldsa_recsign_pack reads it:
 *                  besides the per-block sums of the scan it holds, for every op, where its message and its context begin among the
 *                  concatenated messages and contexts of its class.
 * Asynchronous on `stream`, never waits for the host: three launches ordered by the kernel boundaries.  k_classify (one op per thread,
 *   MLDSA_RECSIGN_SCAN_BLOCK per workgroup) checks each descriptor and writes ten sums per workgroup; k_offsets (one wave per sum)
 *   turns them into exclusive prefixes and the totals; k_apply scans inside each workgroup and writes class_slot and the two
 *   positions.  No kernel waits on another workgroup and every loop runs to a count the host passed.  The blob is not read.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, ops, n_keys, class_slot, totals or plan, ops or totals not 8-byte aligned, class_slot
 *   not 4-byte aligned, plan not 256-byte aligned or smaller than mldsa_recsign_plan_bytes, an n_keys above UINT32_MAX,
 *   n_ops > MLDSA_RECSIGN_MAX_OPS.  n_ops = 0 returns MLDSA_OK and writes nothing. */
int mldsa_recsign_plan(mldsa_ctx *ctx, uint64_t blob_len, uint64_t out_len, const mldsa_recsign_op *ops, size_t n_ops,
                       const size_t *n_keys /* host [3] */, uint32_t *class_slot, mldsa_recsign_totals *totals, void *plan,
                       size_t plan_bytes, void *stream);
/* With R(x) = x rounded up to a multiple of 256 and B = ceil(n_ops / MLDSA_RECSIGN_SCAN_BLOCK) workgroups:
 *   R(80 B) + 2 R(8 n_ops)            ten 64-bit sums per workgroup; message and context position of every op
 * 0 for n_ops > MLDSA_RECSIGN_MAX_OPS. */
size_t mldsa_recsign_plan_bytes(size_t n_ops);

/* ---- 2. the pack: each class's dense arrays -------------------------------------------------------------------------------------------
 * Given the totals as the HOST read them, carves `arena` and fills, for each class c with n_c ops,
 *   key_idx[n_c]               the ops' key rows
 *   msgs, msg_off[n_c + 1]     the class's messages in slot order behind their offsets; likewise ctxs, ctx_off[n_c + 1]
 *   rnd[n_c][32]               the ops' randomness, all zero for an op without MLDSA_RECSIGN_RND
 *   sigs[n_c][SIG_LEN], status[n_c] (int32)    room for the class's signatures and status words (not written here)
 * exactly as mldsa_sign, mldsa_sign_async, mldsa_sign_cached_a or mldsa_hash_sign (mldsa_ph.h) take them: `packed` (host memory)
 * receives the device pointers and counts, and is the seam a caller feeds to those calls itself.  Refused ops are skipped.
 * One launch, one wave per op.  Message, context and rnd are each copied by the plan of fips204_amd/rec/rec_plan.h: bytes one by one
 *   up to the destination's first 16-byte boundary, then 16-byte chunks -- aligned 16-byte loads, funnel-shifted in registers by the
 *   difference between source and destination alignment, aligned 16-byte stores --, then the rest one by one.  The kernel checks every
 *   descriptor again and drops an op whose class, slot or positions disagree with the counts the host passed, so a plan that was
 *   tampered with writes nothing outside the arena and reads nothing outside the blob.
 * Argument errors (MLDSA_ERR_PARAM): NULL pointers as for the plan, blob NULL with blob_len > 0, a NULL totals or packed, counts that
 *   do not add up to n_ops, arena NULL or not 256-byte aligned; MLDSA_ERR_NOMEM: arena_bytes < mldsa_recsign_arena_bytes of the
 *   totals.  n_ops = 0 returns MLDSA_OK with an all-zero *packed. */
typedef struct {
    size_t n; /* ops of the class; the pointers are valid, and the offset tables hold n + 1 entries, also when n = 0 */
    uint32_t *key_idx;
    uint8_t *msgs, *ctxs, *rnd, *sigs;
    uint64_t *msg_off, *ctx_off;
    int32_t *status;
} mldsa_recsign_class;
typedef struct {
    mldsa_recsign_class c[3]; /* MLDSA_RECSIGN_CLASS_44, _65, _87 */
    uint8_t *rnd_region;      /* the three classes' rnd rows back to back: the arena's only secret, to be zeroed after signing */
    size_t rnd_region_bytes;  /* R(32 (n_44 + n_65 + n_87)) */
} mldsa_recsign_packed;
int mldsa_recsign_pack(mldsa_ctx *ctx, const uint8_t *blob, uint64_t blob_len, uint64_t out_len, const mldsa_recsign_op *ops, size_t n_ops,
                       const size_t *n_keys /* host [3] */, const uint32_t *class_slot, const void *plan, size_t plan_bytes,
                       const mldsa_recsign_totals *totals /* host */, void *arena, size_t arena_bytes,
                       mldsa_recsign_packed *packed /* host, out */, void *stream);
/* The arena of a known mix, exactly.  With R as above, SIG_c the signature length of class c and n_c its ops:
 *   sum over c = 44, 65, 87 of  R(4 n_c) + 2 R(8 (n_c + 1)) + R(n_c SIG_c) + R(4 n_c)     key_idx, two offset tables, sigs, status
 *   + R(32 (n_44 + n_65 + n_87))                   the three classes' rnd rows back to back, one region that one memset clears
 *   + R(msg_bytes) + R(ctx_bytes)                  the three classes' messages, then their contexts, back to back in class order
 * msg_bytes and ctx_bytes are the sums over the three classes.  0 when a count exceeds MLDSA_RECSIGN_MAX_OPS or the size does not fit. */
size_t mldsa_recsign_arena_bytes(size_t n44, size_t n65, size_t n87, uint64_t msg_bytes, uint64_t ctx_bytes);
/* A bound for an unknown mix of n_ops ops: at least mldsa_recsign_arena_bytes of every mix with n44 + n65 + n87 <= n_ops.
 *   2 R(4 n_ops) + 2 R(8 n_ops + 24) + R(4627 n_ops) + 5 * 512 + R(32 n_ops) + R(msg_bytes) + R(ctx_bytes)
 * (every op sized as ML-DSA-87; 512 bytes per array for the rounding of the two other classes): within 4 KiB of the all-87 mix.
 * 0 as above. */
size_t mldsa_recsign_arena_bytes_max(size_t n_ops, uint64_t msg_bytes, uint64_t ctx_bytes);

/* ---- 3. the scatter: every signature to its hole ----------------------------------------------------------------------------------------
 * Behind the signing calls on `stream`.  For an accepted op the SIG_LEN bytes of its row of the class's sigs go to out + sig_off -- what
 * mldsa_sign wrote there, all zero when its status is not MLDSA_OK -- and status[i] (int32, one per op) is the class's status[slot].
 * For a refused op only status[i] is written: the refusal's code.
 * One launch, one wave per op.  The copy is the same copy plan in the other direction: the source window is the class's sigs array,
 *   whose rows lie at slot * SIG_LEN (not 16-byte aligned for ML-DSA-65 / 87); the destination residue is (out + sig_off) & 15; the
 *   body's 16-byte stores lie wholly inside the op's range; head and tail go byte by byte, so no byte next to a signature is ever read
 *   or rewritten.  The kernel checks every descriptor again, as the pack does.
 * Signature ranges of two accepted ops that overlap are the caller's error: the overlap then holds bytes of one or the other, and
 *   nothing outside the union is written.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, ops, n_keys, out, class_slot, packed or status, misaligned ops / class_slot / status, a
 *   packed whose counts exceed n_ops or whose class with n > 0 has a NULL sigs or status.  n_ops = 0 returns MLDSA_OK. */
int mldsa_recsign_scatter(mldsa_ctx *ctx, const mldsa_recsign_op *ops, size_t n_ops, uint64_t blob_len, uint8_t *out, uint64_t out_len,
                          const size_t *n_keys /* host [3] */, const uint32_t *class_slot, const mldsa_recsign_packed *packed /* host */,
                          int32_t *status, void *stream);

/* ---- 4. the whole pass ------------------------------------------------------------------------------------------------------------------
 * Signs op i's message under its context with key `key` of keys[class of its set] and `mode` (MLDSA_MODE_*, one per call), writes the
 * signature to out + sig_off and status[i] = mldsa_sign's status of the op; a refused op gets its refusal's code and nothing else.
 *   1. mldsa_recsign_plan on `stream`.
 *   2. The call WAITS for `stream` once, to read the totals.  A caller that wants another signing call behind the seam
 *      (mldsa_sign_async, mldsa_sign_cached_a, mldsa_hash_sign) drives plan, pack and scatter itself.
 *   3. If scratch_bytes is less than the mix needs, the call returns MLDSA_ERR_NOMEM before anything more is launched: out and status
 *      are not written and info->scratch_needed names the need.
 *   4. mldsa_recsign_pack.
 *   5. One mldsa_sign(set_c, mode, keys[c] ..., key_idx_c, ..., rnd_c, sigs_c, status_c, n_c, stream) per non-empty class.  mldsa_sign
 *      waits for the stream itself, so the call is complete when it returns: every accepted op is signed.
 *   6. mldsa_recsign_scatter.
 *   7. The arena's rnd rows are zeroed in stream order, whatever the return code says.
 * out == blob is allowed and defined, and so are overlapping buffers: everything is read from the blob (steps 1 to 5) before the first
 *   signature byte is written (step 6).
 * scratch (256-byte aligned): mldsa_recsign_front_bytes(n_ops) + mldsa_recsign_arena_bytes(the mix) bytes; with
 *   mldsa_recsign_arena_bytes_max in place of the latter the call cannot run out.  Used in stream order.  rnd is the only secret the
 *   scratch ever holds, and step 7 clears it.
 * info (host memory, may be NULL) receives the totals and the scratch the call needs; it is filled whenever step 2 was reached.
 * Argument errors (MLDSA_ERR_PARAM): NULL ctx, ops, keys, out, status or scratch, blob NULL with blob_len > 0, unknown mode, ops not
 *   8-byte, status not 4-byte or scratch not 256-byte aligned, scratch_bytes < mldsa_recsign_front_bytes(n_ops), a served set with a
 *   NULL table pointer, an n_keys above UINT32_MAX, n_ops > MLDSA_RECSIGN_MAX_OPS.  n_ops = 0 returns MLDSA_OK and touches nothing,
 *   without a context.  Errors of a core call pass through with their code, and mldsa_recsign_last_error() then carries the core's
 *   message.
 *
 * Cost, from byte counts (an expectation): the seam -- plan, pack and scatter -- reads and writes about |M| + |ctx| + 32 + SIG_LEN bytes
 *   per op, 0.22 GB for 65 536 ML-DSA-65 ops of 32-byte messages.
 * Measured on an MI355X, 65 536 ops of 32-byte messages with rnd, 1 024 keys per set, signed in place, records 5 mod 16 bytes apart
 *   (profiles/recsign_bench.jsonl; medians of alternating runs; "copy" is a device-to-device copy of the bytes the seam moves, in the
 *   same run):
 *                                               ML-DSA-44   ML-DSA-65   ML-DSA-87   even three-way mix
 *     this call / mldsa_sign on arrays packed
 *       beforehand, signatures left dense       1.098       1.075       1.051       1.050     (5.33 / 7.57 / 9.58 / 9.54 ms)
 *     plan + pack + scatter alone               0.193 ms    0.219 ms    0.246 ms    0.217 ms
 *     plan + pack + scatter / copy              3.01        2.56        2.13        2.47
 *     numpy split + upload + mldsa_sign +
 *       download + host scatter / this call     8.0         8.3         9.1         7.7       (43 ... 87 ms)
 *   The seam moves 1.7 ... 2.5 TB/s read + written where the copy reaches 5.1 ... 5.3: five launches on 0.16 ... 0.31 GB.  The call adds
 *   0.46 ... 0.53 ms to mldsa_sign: the seam, and about 0.3 ms that were not broken down further (the wait for the totals, which drains
 *   the stream in front of the core's call, and the clearing of rnd behind it). */
typedef struct {
    uint64_t n[4];           /* ops per class: 44, 65, 87, refused */
    uint64_t msg_bytes;      /* message bytes of the accepted ops */
    uint64_t ctx_bytes;      /* context bytes of the accepted ops */
    uint64_t scratch_needed; /* mldsa_recsign_front_bytes(n_ops) + mldsa_recsign_arena_bytes of this mix */
} mldsa_recsign_info;
int mldsa_recsign_sign(mldsa_ctx *ctx, int mode, const mldsa_recsign_keys *keys /* host [3] */, const uint8_t *blob, uint64_t blob_len,
                       const mldsa_recsign_op *ops, size_t n_ops, uint8_t *out, uint64_t out_len, int32_t *status, void *scratch,
                       size_t scratch_bytes, mldsa_recsign_info *info /* host */, void *stream);
/* What mldsa_recsign_sign keeps in front of the arena:  R(4 n_ops) + 256 + mldsa_recsign_plan_bytes(n_ops)    class_slot, totals, plan.
 * 0 for n_ops > MLDSA_RECSIGN_MAX_OPS. */
size_t mldsa_recsign_front_bytes(size_t n_ops);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_RECSIGN_H */
