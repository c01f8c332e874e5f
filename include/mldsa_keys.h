/* mldsa_keys.h -- wire-format public keys deduplicated on the device in front of batched verification (libmldsa_keys.so).
 *
 * A verification service receives (pk, message, signature) triples whose keys repeat heavily.  ExpandA bounds verification:
 * mldsa_verify_pk re-derives A_hat for every op, mldsa_verify_cached_a on a table of distinct keys does not.  This library finds
 * the repeats where the keys already lie -- in device memory -- and runs the batch on the table of distinct keys.
 *
 * A front-end library layered on the C ABI of include/mldsa_hip.h, like libmldsa_ph.so: it reaches the core only through the
 * core's public entry points, so every verdict, refusal rule and precedence is the core's.
 *
 * Conventions are those of mldsa_hip.h: pointers to operation data are device pointers, `stream` is a hipStream_t (NULL = the
 * default stream), calls return MLDSA_OK or a negative MLDSA_ERR_* and never abort, every call launches on mldsa_ctx_device(ctx)
 * and restores the caller's current device.  Randomness -- the hash seed -- is the caller's.
 *
 * Public keys only.  Hashing and probing on key bytes is memory access that depends on them: signers pass key_idx themselves.
 */
#ifndef MLDSA_KEYS_H
#define MLDSA_KEYS_H

#include <stddef.h>
#include <stdint.h>

#include "mldsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLDSA_KEYS_ABI_VERSION 1
/* most keys one call dedupes (key indices and slots are 32-bit words) and most rows of a cached table */
#define MLDSA_KEYS_MAX_KEYS ((size_t)1 << 30)
#define MLDSA_KEYS_MAX_CACHED ((size_t)1 << 24)
/* Slots the claim phase looks at before a key gives up and owns a row by itself.  The slot table holds at most one slot per
 * distinct hash value and at least 2 n_keys slots, so its load never exceeds 1/2; a run of k occupied slots under linear
 * probing at load 1/2 has probability about exp(-0.19 k) per slot: 256 puts an exhausted probe below 1e-15 per call for every
 * n_keys the library takes, and a key that does exhaust it costs one surplus row, never a wrong one.  Which key of a cluster runs
 * out of slots depends on the order in which the other hashes of the cluster arrived: this is the one case in which the rows
 * depend on how the waves were scheduled. */
#define MLDSA_KEYS_PROBE_MAX 256

int mldsa_keys_abi_version(void);
/* message of the last failed call of this thread; carries the core's message when a core call failed */
const char *mldsa_keys_last_error(void);

/* ---- the seam: first-occurrence deduplication of n_keys wire-format keys ------------------------------------------------------
 *   row_of[i]  the row of the table that holds key i's bytes
 *   *n_rows    the number of rows (one device word); row_of[i] < n_rows <= n_keys
 *   table      rows with number < table_rows receive their key's bytes: table[row_of[i]] == pk[i] byte for byte.  table may be
 *              NULL with table_rows = 0; n_rows is the true count either way, rows >= table_rows are not written.
 * Rows are numbered in order of FIRST OCCURRENCE in pk: row r is the r-th key that has no equal key before it (an exclusive scan
 *   over "owns a row" flags, not an arrival counter), so the result does not depend on the order the waves ran in (but for an
 *   exhausted probe: see MLDSA_KEYS_PROBE_MAX).
 * The hash is a keyed hash of the key bytes under `seed` (16 bytes of HOST memory, read during the call) with a 64-bit value: an
 *   NH sum of 32 x 32 -> 64-bit products, finalised to 64 bits.  Correctness never depends on it: two keys share a row only after a
 *   full byte comparison.  The seed only stops someone who chooses the keys from forcing long probe chains or shared slots; NH's
 *   bound is that of its 32-bit words, so such a person makes a chosen pair of keys share a slot with probability 2^-32, not 2^-64,
 *   and the price of success is a surplus row.  Draw the seed from the system's generator.
 * hash_bits (1 ... 64; 64 is the normal value) keeps only that many bits of the hash, so that tests can force collisions.  Keys with
 *   the same (truncated) hash share one slot whose owner is the lowest key index among them; a key whose bytes differ from its
 *   slot owner's, or whose probe ran MLDSA_KEYS_PROBE_MAX slots, gets a row of its own even if an equal key exists.  n_rows is then
 *   larger than the number of distinct keys; everything above still holds.  At 64 bits that takes a collision of the hash under
 *   an unknown seed.
 * Nothing outside the n_keys input rows is read; nothing outside row_of, the first min(n_rows, table_rows) table rows, n_rows and
 *   the first mldsa_keys_dedup_scratch_bytes(set, n_keys) bytes of scratch is written.
 * Asynchronous on `stream`, never synchronises the host: seven launches (clear the slots; hash + claim; confirm; three for the
 *   scan; gather + row_of), ordered by the kernel boundaries.  Scratch is used in stream order and may be reused by the next call on
 *   the same stream.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set, hash_bits outside 1 ... 64, n_keys >
 *   MLDSA_KEYS_MAX_KEYS, a NULL pk / seed / row_of / n_rows, a NULL table with table_rows > 0, pk, table or scratch not 16-byte
 *   aligned, scratch NULL or smaller than mldsa_keys_dedup_scratch_bytes.  n_keys = 0 writes *n_rows = 0 (when n_rows and ctx are
 *   given) and returns MLDSA_OK. */
int mldsa_keys_dedup(mldsa_ctx *ctx, int set, const uint8_t *pk /* [n_keys][PK_LEN], 16-byte aligned */, size_t n_keys,
                     const uint8_t seed[16], int hash_bits, uint32_t *row_of /* [n_keys] */,
                     uint8_t *table /* [table_rows][PK_LEN], 16-byte aligned */, size_t table_rows, uint32_t *n_rows /* one device word */,
                     void *scratch, size_t scratch_bytes, void *stream);
/* 12 cap + 12 n_pad + 16 ceil(n_pad / 4096) bytes, with cap = the smallest power of two >= max(2 n_keys, 64) (slots: an 8-byte tag
 * and a 4-byte owner each) and n_pad = n_keys rounded up to a multiple of 1024 (slot, representative and rank of every key; one
 * count per 1024 keys for the scan).  0 for an unknown set or n_keys > MLDSA_KEYS_MAX_KEYS. */
size_t mldsa_keys_dedup_scratch_bytes(int set, size_t n_keys);

/* ---- the op-level call: mldsa_verify_pk behind the seam ---------------------------------------------------------------------
 * Arguments, verdicts, refusal rules and precedence are those of mldsa_verify_pk on the same arguments, byte for byte.
 *   1. The keys the call uses are deduplicated: the first n_ops rows of pk when key_idx is NULL, else the n_keys rows of the table,
 *      and the per-op index is composed, idx[op] = row_of[key_idx[op]]; an out-of-range key_idx[op] becomes 0xFFFFFFFF, so the
 *      core refuses that op by its own rule (ok = 0).
 *   2. The call WAITS for `stream` once, to read the one word n_rows.  This is its only host synchronisation; a caller that wants
 *      none drives the seam and mldsa_verify_cached_a itself.
 *   3. Cached route, n_rows <= max_cached_keys: mldsa_pk_expand and mldsa_expand_a on the gathered table in scratch, then
 *      mldsa_verify_cached_a with the composed index.  Plain route, otherwise: mldsa_verify_pk on the caller's original arrays.
 * max_cached_keys bounds the scratch (PK_LEN + 96 + 1024 K (1 + L) bytes per row: 17 / 36 / 67 KiB for ML-DSA-44 / 65 / 87) and
 *   the work spent on the table before it pays; see the note at the end of this comment.
 * info (may be NULL; host memory) receives n_rows and the route taken.
 * Argument errors (MLDSA_ERR_PARAM before anything is launched): NULL ctx, unknown set or mode, hash_bits outside 1 ... 64, a NULL pk /
 *   msg_off / sigs / ok / seed, n_keys that does not cover the batch (0 with key_idx, < n_ops without), more than
 *   MLDSA_KEYS_MAX_KEYS keys or ops, max_cached_keys > MLDSA_KEYS_MAX_CACHED, pk not 16-byte aligned, scratch NULL, not 256-byte
 *   aligned or smaller than mldsa_keys_verify_scratch_bytes.  n_ops = 0 returns MLDSA_OK.  Errors of a core call pass through with
 *   their code, and mldsa_keys_last_error() then carries the core's message.
 *
 * Measured on an MI355X, 65 536 ops per call, one wire key per op, D distinct keys (profiles/keys_dedup_bench.jsonl; medians of
 *   alternating runs, time of this call over mldsa_verify_pk's):
 *     D            1      64     1 024  8 192  65 536 (cached route forced)   65 536 (max_cached_keys = 8 192: plain route)
 *     ML-DSA-44    0.48   0.42   0.42   0.52   1.12                            1.04
 *     ML-DSA-65    0.36   0.32   0.32   0.47   1.14                            1.03
 *     ML-DSA-87    0.26   0.24   0.25   0.42   1.11                            1.03
 *   ML-DSA-65 at D = 1 024: 0.69 ms = 95 M verifies/s against 30.6 M/s for mldsa_verify_pk and 140 M/s for mldsa_verify_cached_a on
 *   a table built beforehand (this call takes 1.35 ... 1.9 times that bound up to D = 8 192).  The seam alone takes 64 ... 123 us (149 ... 183 us when all keys are equal).
 *   Recommendation: max_cached_keys = 8 192, the largest D measured at which the cached route wins (by more than mldsa_verify_pk's
 *   own p10-p90 spread, on every set); it is the Python default.  When every key is distinct the cached route LOSES 11 ... 14 %; with
 *   max_cached_keys = 8 192 such a batch takes the plain route and loses 3 ... 4 % (the seam and the wait).  The crossover lies between
 *   8 192 and 65 536 distinct keys and has not been located more finely. */
#define MLDSA_KEYS_ROUTE_PLAIN 0
#define MLDSA_KEYS_ROUTE_CACHED 1
typedef struct {
    uint32_t n_rows; /* rows the deduplication found */
    int route;       /* MLDSA_KEYS_ROUTE_* */
} mldsa_keys_info;
int mldsa_verify_pk_dedup(mldsa_ctx *ctx, int set, int mode, const uint8_t *pk, size_t n_keys, const uint32_t *key_idx,
                          const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *ctxs, const uint64_t *ctx_off,
                          const uint8_t *sigs, uint8_t *ok, size_t n_ops, const uint8_t seed[16], int hash_bits,
                          size_t max_cached_keys, void *scratch, size_t scratch_bytes, mldsa_keys_info *info, void *stream);
/* n_keys: the larger of n_ops and the number of keys the call dedupes (n_keys of the call when key_idx is given, else n_ops).
 * With R(x) = x rounded up to a multiple of 256:
 *   R(mldsa_keys_dedup_scratch_bytes(set, n_keys)) + 2 R(4 n_keys) + 256                     row_of, composed index, n_rows
 *   + R(m PK_LEN) + R(32 m) + R(64 m) + R(1024 K m) + R(1024 K L m),  m = max_cached_keys    table, rho, tr, t1, A_hat
 * 0 for an unknown set, n_keys > MLDSA_KEYS_MAX_KEYS or max_cached_keys > MLDSA_KEYS_MAX_CACHED. */
size_t mldsa_keys_verify_scratch_bytes(int set, size_t n_keys, size_t max_cached_keys);

#ifdef __cplusplus
}
#endif

#endif /* MLDSA_KEYS_H */
