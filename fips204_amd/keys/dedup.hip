// libmldsa_keys.so (include/mldsa_keys.h): wire-format public keys deduplicated on the device, and mldsa_verify_pk behind that seam.
//
// One wave per key for everything that touches key bytes: PK_LEN is 82 / 122 / 162 sixteen-byte chunks, lane l holds the chunks
// l, l + 64 (, l + 128) in registers, and hash and comparison are reduced across the wave with shuffles -- no LDS anywhere.
// The phases are separate launches and the kernel boundaries do all the ordering: no wave waits for another wave, and inside a
// launch other waves' words are touched by relaxed atomics only.
//   k_claim    keyed 64-bit hash of key i; linear probing in an open-addressing table of (tag, owner) slots: the first slot on
//              the key's path that is empty (atomicCAS claims it with the hash as its tag) or already carries the hash takes the
//              key, and owner = atomicMin over the indices of the keys it took.  Keys with equal bytes have equal hashes, walk the
//              same path and meet in the same slot whichever came first, so when the launch ends that slot's owner is the first
//              occurrence -- whatever the order the waves ran in.
//   k_confirm  key i against its slot's owner, byte for byte: equal -> rep[i] = owner; different (two keys under one hash), or no
//              slot within the probe bound -> rep[i] = i, the key owns a row.  Owners own theirs (rep[o] = o).
//   k_count, k_offsets, k_rank   exclusive scan over the flags rep[i] == i: rank[i] = owning keys before i; the total is n_rows.
//   k_gather   row_of[i] = rank[rep[i]]; an owner whose row lies below table_rows copies its bytes into the table.
// What bounds them: k_claim and k_confirm each read every key once, and k_confirm reads the owner's row as well for every key that is
// not its slot's owner (up to a third pass over the key bytes; with few distinct keys those rows come from L2 / the last-level cache);
// a batch of repeats adds one atomicMin per key only while the owner word it read is still above its own index.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_keys.h"
#include "../layer/layer_host.h"

namespace {

using namespace mldsa_layer;

constexpr uint32_t NONE = 0xFFFFFFFFu;       // no slot / empty owner
constexpr uint64_t EMPTY = ~(uint64_t)0;     // empty tag: what the clearing memset (0xFF) leaves
constexpr int WAVES = 4;                     // keys per workgroup in the one-wave-per-key kernels
constexpr int SCAN_PER_LANE = 16, SCAN_PER_WAVE = 64 * SCAN_PER_LANE;  // the scan: 1024 flags per wave

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

template <typename T>
__device__ __forceinline__ T relaxed_load(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The chunks of one key in registers: chunk c of the key is v[c / 64] of lane c % 64.
template <int CH>
struct KeyRegs {
    static constexpr int STEPS = (CH + 63) / 64;
    uint4 v[STEPS];
    __device__ __forceinline__ void load(const uint4* __restrict__ row, int lane) {
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int c = s * 64 + lane;
            v[s] = c < CH ? row[c] : make_uint4(0, 0, 0, 0);
        }
    }
};

// Keyed hash, the same value in every lane.  NH-style: every 16-byte chunk contributes (m0 + k0)(m1 + k1) + (m2 + k2)(m3 + k3) in
// 64-bit arithmetic with four 32-bit key words of its own, drawn from the seed by splitmix64 at the chunk's position; the sum over
// the chunks (any order: the position is in the key words) is finalised under the second seed word.  A 64-bit value, but NH's bound
// is that of its 32-bit words: two chosen keys that differ in one word collide when the partner word plus its key word is 0 mod 2^32,
// so someone who picks the keys without knowing the seed makes a given pair collide with probability 2^-32, not 2^-64.  Not a MAC and
// not asked to be one: a collision costs surplus rows, never a wrong one.
template <int CH>
__device__ __forceinline__ uint64_t key_hash(const KeyRegs<CH>& k, int lane, uint64_t s0, uint64_t s1, int hash_bits) {
    uint64_t acc = 0;
#pragma unroll
    for (int s = 0; s < KeyRegs<CH>::STEPS; ++s) {
        const int c = s * 64 + lane;
        if (c < CH) {
            const uint64_t ka = mix64(s0 + (uint64_t)(2 * c + 1) * 0x9E3779B97F4A7C15ull);
            const uint64_t kb = mix64(s1 + (uint64_t)(2 * c + 2) * 0x9E3779B97F4A7C15ull);
            const uint4 m = k.v[s];
            acc += (uint64_t)(m.x + (uint32_t)ka) * (uint64_t)(m.y + (uint32_t)(ka >> 32));
            acc += (uint64_t)(m.z + (uint32_t)kb) * (uint64_t)(m.w + (uint32_t)(kb >> 32));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor((unsigned long long)acc, d, 64);
    uint64_t h = mix64(acc + s1);
    if (hash_bits < 64) h &= ((uint64_t)1 << hash_bits) - 1;
    return h == EMPTY ? h - 1 : h;  // the all-ones word marks an empty slot
}

template <int CH>
__global__ __launch_bounds__(64 * WAVES) void k_claim(const uint4* __restrict__ pk, uint32_t n, uint64_t s0, uint64_t s1, int hash_bits,
                                                       unsigned long long* tags, uint32_t* owners, uint32_t slot_mask,
                                                       uint32_t* __restrict__ slot_of) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    KeyRegs<CH> k;
    k.load(pk + (size_t)i * CH, lane);
    const uint64_t h = key_hash<CH>(k, lane, s0, s1, hash_bits);
    if (lane != 0) return;
    uint32_t s = (uint32_t)h & slot_mask, got = NONE;
    for (int p = 0; p < MLDSA_KEYS_PROBE_MAX; ++p, s = (s + 1) & slot_mask) {
        // a look first: in a batch of repeats nearly every key finds its hash already there, and a load does not serialise
        unsigned long long t = relaxed_load(&tags[s]);
        if (t == EMPTY) t = atomicCAS(&tags[s], (unsigned long long)EMPTY, (unsigned long long)h);
        if (t == EMPTY || t == h) {
            got = s;
            break;
        }
    }
    // owner = the lowest index the slot took; keys are dispatched roughly in index order, so most find a lower owner and add nothing
    if (got != NONE && relaxed_load(&owners[got]) > i) atomicMin(&owners[got], i);
    slot_of[i] = got;
}

template <int CH>
__global__ __launch_bounds__(64 * WAVES) void k_confirm(const uint4* __restrict__ pk, uint32_t n, const uint32_t* __restrict__ owners,
                                                         const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ rep) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    const uint32_t o = s == NONE ? i : owners[s];  // o <= i: key i itself lowered the owner to at most i
    uint32_t r = i;
    if (o < i) {
        KeyRegs<CH> a, b;
        a.load(pk + (size_t)i * CH, lane);
        b.load(pk + (size_t)o * CH, lane);
        uint32_t diff = 0;
#pragma unroll
        for (int t = 0; t < KeyRegs<CH>::STEPS; ++t)
            diff |= (a.v[t].x ^ b.v[t].x) | (a.v[t].y ^ b.v[t].y) | (a.v[t].z ^ b.v[t].z) | (a.v[t].w ^ b.v[t].w);
        if (!__any(diff != 0)) r = o;
    }
    if (lane == 0) rep[i] = r;
}

// ---- exclusive scan over the flags rep[j] == j, 1024 flags per wave.  rep and rank are padded to a multiple of 1024 entries, so
// the 16-byte accesses stay inside them; entries from n on are never counted.
__device__ __forceinline__ uint32_t lane_flags(const uint32_t* __restrict__ rep, uint32_t n, uint32_t base, uint32_t (&f)[SCAN_PER_LANE]) {
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER_LANE / 4; ++q) {
        const uint4 v = *reinterpret_cast<const uint4*>(rep + base + 4 * q);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t j = base + 4 * q + e;
            f[4 * q + e] = (j < n && w[e] == j) ? 1u : 0u;
            cnt += f[4 * q + e];
        }
    }
    return cnt;
}

__global__ __launch_bounds__(64) void k_count(const uint32_t* __restrict__ rep, uint32_t n, uint32_t* __restrict__ counts) {
    uint32_t f[SCAN_PER_LANE];
    uint32_t cnt = lane_flags(rep, n, blockIdx.x * SCAN_PER_WAVE + threadIdx.x * SCAN_PER_LANE, f);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
}

// inclusive scan of one value per lane across the wave
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// one wave: counts[b] -> rows owned before block b (in place); the total is n_rows
__global__ __launch_bounds__(64) void k_offsets(uint32_t* __restrict__ counts, uint32_t n_blocks, uint32_t* __restrict__ n_rows) {
    const int lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 64) {
        const uint32_t b = base + lane;
        const uint32_t v = b < n_blocks ? counts[b] : 0;
        const uint32_t inc = wave_inclusive(v, lane);
        if (b < n_blocks) counts[b] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) *n_rows = carry;
}

__global__ __launch_bounds__(64) void k_rank(const uint32_t* __restrict__ rep, uint32_t n, const uint32_t* __restrict__ offsets,
                                            uint32_t* __restrict__ rank) {
    const int lane = threadIdx.x;
    const uint32_t base = blockIdx.x * SCAN_PER_WAVE + lane * SCAN_PER_LANE;
    uint32_t f[SCAN_PER_LANE];
    const uint32_t cnt = lane_flags(rep, n, base, f);
    uint32_t run = offsets[blockIdx.x] + wave_inclusive(cnt, lane) - cnt;
#pragma unroll
    for (int q = 0; q < SCAN_PER_LANE / 4; ++q) {
        uint4 o;
        o.x = run; run += f[4 * q];
        o.y = run; run += f[4 * q + 1];
        o.z = run; run += f[4 * q + 2];
        o.w = run; run += f[4 * q + 3];
        *reinterpret_cast<uint4*>(rank + base + 4 * q) = o;
    }
}

template <int CH>
__global__ __launch_bounds__(64 * WAVES) void k_gather(const uint4* __restrict__ pk, uint32_t n, const uint32_t* __restrict__ rep,
                                                        const uint32_t* __restrict__ rank, uint32_t* __restrict__ row_of,
                                                        uint4* __restrict__ table, uint32_t table_rows) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t r = rep[i];     // r <= i < n
    const uint32_t row = rank[r];  // < n_rows
    if (lane == 0) row_of[i] = row;
    if (r != i || row >= table_rows) return;
    KeyRegs<CH> k;
    k.load(pk + (size_t)i * CH, lane);
    uint4* dst = table + (size_t)row * CH;
#pragma unroll
    for (int s = 0; s < KeyRegs<CH>::STEPS; ++s) {
        const int c = s * 64 + lane;
        if (c < CH) dst[c] = k.v[s];
    }
}

// idx[op] = row_of[key_idx[op]], 0xFFFFFFFF for an index outside the n_keys rows: the core refuses that op by its own rule
__global__ __launch_bounds__(256) void k_compose(const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ row_of, uint32_t n_keys,
                                               uint32_t* __restrict__ idx, uint32_t n_ops) {
    const uint32_t op = blockIdx.x * 256 + threadIdx.x;
    if (op >= n_ops) return;
    const uint32_t k = key_idx[op];
    idx[op] = k < n_keys ? row_of[k] : NONE;
}

// ------------------------------------------------------------------------------------------------------------ host side
size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// scratch of the seam: [tags: 8 cap] [owners: 4 cap] [slot_of: 4 n_pad] [rep: 4 n_pad] [rank: 4 n_pad] [counts: 16 ceil(n_pad / 4096)]
struct DedupLayout {
    size_t cap, n_pad, n_blocks, bytes;
};

bool dedup_layout(int set, size_t n, DedupLayout* o) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_KEYS_MAX_KEYS) return false;
    size_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    o->cap = cap;
    o->n_pad = round_up(n, SCAN_PER_WAVE);
    o->n_blocks = o->n_pad / SCAN_PER_WAVE;
    o->bytes = 12 * cap + 12 * o->n_pad + 16 * ((o->n_blocks + 3) / 4);
    return true;
}

template <int CH>
void launch_keyed(const uint8_t* pk, uint32_t n, uint64_t s0, uint64_t s1, int hash_bits, unsigned long long* tags, uint32_t* owners,
                  uint32_t slot_mask, uint32_t* slot_of, uint32_t* rep, hipStream_t s) {
    const dim3 grid((n + WAVES - 1) / WAVES), block(64 * WAVES);
    const uint4* k = reinterpret_cast<const uint4*>(pk);
    hipLaunchKernelGGL((k_claim<CH>), grid, block, 0, s, k, n, s0, s1, hash_bits, tags, owners, slot_mask, slot_of);
    hipLaunchKernelGGL((k_confirm<CH>), grid, block, 0, s, k, n, owners, slot_of, rep);
}

template <int CH>
void launch_gather(const uint8_t* pk, uint32_t n, const uint32_t* rep, const uint32_t* rank, uint32_t* row_of, uint8_t* table,
                   uint32_t table_rows, hipStream_t s) {
    hipLaunchKernelGGL((k_gather<CH>), dim3((n + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, s, reinterpret_cast<const uint4*>(pk), n, rep,
                       rank, row_of, reinterpret_cast<uint4*>(table), table_rows);
}

// every check is the caller's: n >= 1, the current device is the context's
int launch_dedup(const char* fn, int set, const uint8_t* pk, size_t n_keys, const uint8_t* seed, int hash_bits, uint32_t* row_of,
                 uint8_t* table, size_t table_rows, uint32_t* n_rows, void* scratch, const DedupLayout& L, hipStream_t s) {
    uint8_t* base = static_cast<uint8_t*>(scratch);
    unsigned long long* tags = reinterpret_cast<unsigned long long*>(base);
    uint32_t* owners = reinterpret_cast<uint32_t*>(base + 8 * L.cap);
    uint32_t* slot_of = owners + L.cap;
    uint32_t* rep = slot_of + L.n_pad;
    uint32_t* rank = rep + L.n_pad;
    uint32_t* counts = rank + L.n_pad;
    uint64_t s0, s1;
    memcpy(&s0, seed, 8);
    memcpy(&s1, seed + 8, 8);
    const uint32_t n = (uint32_t)n_keys, mask = (uint32_t)(L.cap - 1);
    const uint32_t rows = (uint32_t)(table_rows < n_keys ? table_rows : n_keys);
    hipError_t e = hipMemsetAsync(base, 0xFF, 12 * L.cap, s);  // every tag EMPTY, every owner NONE
    if (e != hipSuccess) return hip_failed(fn, "clearing the slots", e);
    if (set == MLDSA_44) launch_keyed<82>(pk, n, s0, s1, hash_bits, tags, owners, mask, slot_of, rep, s);
    else if (set == MLDSA_65) launch_keyed<122>(pk, n, s0, s1, hash_bits, tags, owners, mask, slot_of, rep, s);
    else launch_keyed<162>(pk, n, s0, s1, hash_bits, tags, owners, mask, slot_of, rep, s);
    const uint32_t nb = (uint32_t)L.n_blocks;
    hipLaunchKernelGGL(k_count, dim3(nb), dim3(64), 0, s, rep, n, counts);
    hipLaunchKernelGGL(k_offsets, dim3(1), dim3(64), 0, s, counts, nb, n_rows);
    hipLaunchKernelGGL(k_rank, dim3(nb), dim3(64), 0, s, rep, n, counts, rank);
    if (set == MLDSA_44) launch_gather<82>(pk, n, rep, rank, row_of, table, rows, s);
    else if (set == MLDSA_65) launch_gather<122>(pk, n, rep, rank, row_of, table, rows, s);
    else launch_gather<162>(pk, n, rep, rank, row_of, table, rows, s);
    LAYER_LAUNCHED("kernel launch");
    return MLDSA_OK;
}

// scratch of the op-level call, every part rounded up to 256 bytes
struct VerifyLayout {
    size_t dedup, row_of, idx, n_rows, table, rho, tr, t1, a_hat, bytes;
};

bool verify_layout(int set, size_t n, size_t m, VerifyLayout* o) {
    mldsa_params p;
    DedupLayout d;
    if (mldsa_get_params(set, &p) != MLDSA_OK || !dedup_layout(set, n, &d) || m > MLDSA_KEYS_MAX_CACHED) return false;
    Taker t;
    t.round = 256;
    o->dedup = t.take(d.bytes);
    o->row_of = t.take(4 * n);
    o->idx = t.take(4 * n);
    o->n_rows = t.take(256);
    o->table = t.take(m * (size_t)p.pk_len);
    o->rho = t.take(32 * m);
    o->tr = t.take(64 * m);
    o->t1 = t.take(1024 * (size_t)p.k * m);
    o->a_hat = t.take(1024 * (size_t)p.k * (size_t)p.l * m);
    o->bytes = t.at;
    return true;
}

}  // namespace

extern "C" {

int mldsa_keys_abi_version(void) { return MLDSA_KEYS_ABI_VERSION; }

const char* mldsa_keys_last_error(void) { return g_err.c_str(); }

size_t mldsa_keys_dedup_scratch_bytes(int set, size_t n_keys) {
    DedupLayout L;
    return dedup_layout(set, n_keys, &L) ? L.bytes : 0;
}

size_t mldsa_keys_verify_scratch_bytes(int set, size_t n_keys, size_t max_cached_keys) {
    VerifyLayout L;
    return verify_layout(set, n_keys, max_cached_keys, &L) ? L.bytes : 0;
}

int mldsa_keys_dedup(mldsa_ctx* ctx, int set, const uint8_t* pk, size_t n_keys, const uint8_t seed[16], int hash_bits, uint32_t* row_of,
                     uint8_t* table, size_t table_rows, uint32_t* n_rows, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_keys_dedup";
    DedupLayout L;
    if (!dedup_layout(set, n_keys, &L)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set or too many keys");
    if (hash_bits < 1 || hash_bits > 64) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": hash_bits outside 1 ... 64");
    if (n_keys == 0 && (!ctx || !n_rows)) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (n_keys != 0) {
        if (!pk || !seed || !row_of || !n_rows || (!table && table_rows != 0)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
        if (!aligned(pk, 16) || !aligned(table, 16) || !aligned(row_of, 4) || !aligned(n_rows, 4))
            return fail(MLDSA_ERR_PARAM, std::string(fn) + ": pk and table must be 16-byte aligned, row_of and n_rows 4-byte aligned");
        if (!scratch || !aligned(scratch, 16) || scratch_bytes < L.bytes)
            return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, misaligned or smaller than mldsa_keys_dedup_scratch_bytes");
    }
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (n_keys == 0) {
        const hipError_t e = hipMemsetAsync(n_rows, 0, 4, s);
        return e == hipSuccess ? MLDSA_OK : hip_failed(fn, "clearing n_rows", e);
    }
    return launch_dedup(fn, set, pk, n_keys, seed, hash_bits, row_of, table, table_rows, n_rows, scratch, L, s);
}

int mldsa_verify_pk_dedup(mldsa_ctx* ctx, int set, int mode, const uint8_t* pk, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                          const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, const uint8_t* sigs, uint8_t* ok,
                          size_t n_ops, const uint8_t seed[16], int hash_bits, size_t max_cached_keys, void* scratch, size_t scratch_bytes,
                          mldsa_keys_info* info, void* stream) {
    const char* fn = "mldsa_verify_pk_dedup";
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (hash_bits < 1 || hash_bits > 64) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": hash_bits outside 1 ... 64");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    // the core refuses an unknown mode before it launches anything; so does this call, which would otherwise find out after its wait
    if (mode != MLDSA_MODE_PURE && mode != MLDSA_MODE_INTERNAL && mode != MLDSA_MODE_PREHASH)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (!pk || !msg_off || !sigs || !ok || !seed) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (key_idx ? n_keys == 0 : n_keys < n_ops) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys does not cover the batch");
    const size_t n_dedup = key_idx ? n_keys : n_ops;  // the keys the call uses
    const size_t n_max = n_dedup > n_ops ? n_dedup : n_ops;
    VerifyLayout V;
    DedupLayout D;
    if (n_ops > MLDSA_KEYS_MAX_KEYS || !verify_layout(set, n_max, max_cached_keys, &V) || !dedup_layout(set, n_dedup, &D))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_KEYS_MAX_KEYS keys or ops, or max_cached_keys > MLDSA_KEYS_MAX_CACHED");
    if (!aligned(pk, 16)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": pk must be 16-byte aligned");
    if (!scratch || !aligned(scratch, 256) || scratch_bytes < V.bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_keys_verify_scratch_bytes");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint32_t* row_of = reinterpret_cast<uint32_t*>(base + V.row_of);
    uint32_t* idx = reinterpret_cast<uint32_t*>(base + V.idx);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(base + V.n_rows);
    uint8_t* table = base + V.table;
    const size_t cap = max_cached_keys < n_dedup ? max_cached_keys : n_dedup;

    int rc = launch_dedup(fn, set, pk, n_dedup, seed, hash_bits, row_of, cap ? table : nullptr, cap, d_rows, base + V.dedup, D, s);
    if (rc != MLDSA_OK) return rc;
    const uint32_t* use_idx = row_of;  // key_idx NULL: op i uses key i, so its row is row_of[i]
    if (key_idx) {
        hipLaunchKernelGGL(k_compose, dim3((unsigned)((n_ops + 255) / 256)), dim3(256), 0, s, key_idx, row_of, (uint32_t)n_keys, idx,
                           (uint32_t)n_ops);
        LAYER_LAUNCHED("k_compose launch");
        use_idx = idx;
    }
    // the call's one host wait: the route depends on n_rows
    uint32_t rows = 0;
    hipError_t e = hipMemcpyAsync(&rows, d_rows, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_failed(fn, "reading n_rows", e);
    const bool cached = rows <= cap;
    if (info) {
        info->n_rows = rows;
        info->route = cached ? MLDSA_KEYS_ROUTE_CACHED : MLDSA_KEYS_ROUTE_PLAIN;
    }
    if (!cached) {
        rc = mldsa_verify_pk(ctx, set, mode, pk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, stream);
        return rc == MLDSA_OK ? rc : core_failed(fn, "mldsa_verify_pk", rc);
    }
    uint8_t* rho = base + V.rho;
    uint8_t* tr = base + V.tr;
    int32_t* t1 = reinterpret_cast<int32_t*>(base + V.t1);
    int32_t* a_hat = reinterpret_cast<int32_t*>(base + V.a_hat);
    LAYER_CORE(mldsa_pk_expand(ctx, set, table, rho, tr, t1, rows, stream), "mldsa_pk_expand");
    LAYER_CORE(mldsa_expand_a(ctx, set, rho, a_hat, rows, stream), "mldsa_expand_a");
    rc = mldsa_verify_cached_a(ctx, set, mode, a_hat, tr, t1, rows, use_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, stream);
    return rc == MLDSA_OK ? rc : core_failed(fn, "mldsa_verify_cached_a", rc);
}

}  // extern "C"
