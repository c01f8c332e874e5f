// libmldsa_seed.so (include/mldsa_seed.h): private keys in seed form -- ML-DSA.KeyGen_internal (FIPS 204 Algorithm 6) delivered as the
// expanded private key mldsa_sign takes, the seed / expanded-key consistency check, and signing from a table of seeds -- layered on
// the core's C ABI.  The core does the sampling and the arithmetic on int32 polynomials (mldsa_expand_a, mldsa_expand_s, mldsa_ntt,
// mldsa_mat_vec_mul, mldsa_inv_ntt, mldsa_to_mont) and whole operations (mldsa_keygen for the check, mldsa_sign); the kernels here
// are the steps between them:
//   k_seed_h     (rho, rho', K) = H(xi | K | L, 128): one seed per lane, one permutation (34 bytes in, 128 out, one rate block).
//   k_seed_rows  s1 | s2 as ExpandS leaves them ([key][L + K] rows) -> the s1 and s2 output rows, where the NTT then runs in place:
//                the core's NTT and matrix-vector product want each vector contiguous over the keys.
//   k_seed_t     one wave per row (key, i), four consecutive coefficients per lane: t = A s1 + s2 mod q, Power2Round, t0 (centred)
//                as int32 for the NTT that follows, t1 packed into the key's pk row -- SimpleBitPack, 10 bits: a lane's 40 bits are
//                spread over the row's 80 dwords with lane shuffles, so the stores are whole, consecutive dwords.
//   k_seed_tr    tr = H(pk, 64): one key per lane on the lane-per-state Keccak, the 10 / 15 / 20 rate blocks staged cooperatively
//                into an LDS tile (the layout layer/layer_dev.h describes).
//   k_seed_cmp   one wave per key: 16-byte loads of the generated and the presented wire key, differences ORed across the wave.
//                The trip count depends on the parameter set only and every address on the key's number only: both keys are secret.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_seed.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"

namespace {

using namespace mldsa_layer;
using mldsa::SHAKE256_RATE;
using mldsa::load_le32;

// ------------------------------------------------------------------------------------------------------------- seed hash
// xi [n][32] -> rho [n][32], rho' [n][64], K [n][32]; rho also opens the key's wire public key (pk_rows, pk_len bytes apart)
__global__ __launch_bounds__(64) void k_seed_h(const uint8_t* __restrict__ xi, uint32_t kl /* K | L << 8 */, uint8_t* __restrict__ rho,
                                              uint8_t* __restrict__ rho_prime, uint8_t* __restrict__ cap_k, uint8_t* __restrict__ pk_rows,
                                              size_t pk_len, size_t n) {
    const size_t key = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (key >= n) return;
    KeccakState st;
    mldsa::keccak_zero(st);
    mldsa::absorb_words<4>(st, xi + key * 32);
    st.lo[4] = kl | (0x1Fu << 16);  // bytes 32, 33 and the pad at byte 34
    st.hi[SHAKE256_RATE / 8 - 1] = 0x80000000u;
    mldsa::keccak_f1600(st);
    u32_any* r = reinterpret_cast<u32_any*>(rho + key * 32);
    u32_any* pr = reinterpret_cast<u32_any*>(pk_rows + key * pk_len);
    u32_any* k = reinterpret_cast<u32_any*>(cap_k + key * 32);
    uint32_t* rp = reinterpret_cast<uint32_t*>(rho_prime + key * 64);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        r[2 * w] = st.lo[w];
        r[2 * w + 1] = st.hi[w];
        pr[2 * w] = st.lo[w];
        pr[2 * w + 1] = st.hi[w];
        k[2 * w] = st.lo[12 + w];
        k[2 * w + 1] = st.hi[12 + w];
    }
#pragma unroll
    for (int w = 0; w < 8; w++) {
        rp[2 * w] = st.lo[4 + w];
        rp[2 * w + 1] = st.hi[4 + w];
    }
}

// ----------------------------------------------------------------------------------------------------- s1 | s2 -> two vectors
// s1s2 [n][L + K][256] -> s1 [n][L][256], s2 [n][K][256]; one workgroup per key, 16 bytes per thread and step
__global__ __launch_bounds__(256) void k_seed_rows(const int32_t* __restrict__ s1s2, int32_t* __restrict__ s1, int32_t* __restrict__ s2,
                                                  int k_polys, int l_polys) {
    const size_t key = blockIdx.x;
    const int4* src = reinterpret_cast<const int4*>(s1s2) + key * (size_t)(l_polys + k_polys) * 64;
    int4* d1 = reinterpret_cast<int4*>(s1) + key * (size_t)l_polys * 64;
    int4* d2 = reinterpret_cast<int4*>(s2) + key * (size_t)k_polys * 64;
    for (int c = threadIdx.x; c < l_polys * 64; c += 256) d1[c] = src[c];
    for (int c = threadIdx.x; c < k_polys * 64; c += 256) d2[c] = src[l_polys * 64 + c];
}

// ------------------------------------------------------------------------------------------- t = A s1 + s2, Power2Round, pk
// w [n][K][256] canonical (mldsa_inv_ntt's output); s1s2 [n][L + K][256]; t0 [n][K][256]; pk_rows: the keys' wire public keys,
// pk_len bytes apart (rho | K rows of 320 bytes).  Workgroup = 4 waves = 4 rows.
__global__ __launch_bounds__(256) void k_seed_t(const int32_t* __restrict__ w, const int32_t* __restrict__ s1s2, int32_t* __restrict__ t0,
                                               uint8_t* __restrict__ pk_rows, size_t pk_len, int k_polys, int l_polys, size_t n_rows) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // the same for the whole wave
    const size_t key = row / (size_t)k_polys;
    const int i = (int)(row - key * (size_t)k_polys);
    const int4 wv = reinterpret_cast<const int4*>(w + row * 256)[lane];
    const int4 sv = reinterpret_cast<const int4*>(s1s2 + (key * (size_t)(l_polys + k_polys) + l_polys + i) * 256)[lane];
    const int32_t t[4] = {canon(wv.x + sv.x), canon(wv.y + sv.y), canon(wv.z + sv.z), canon(wv.w + sv.w)};
    int32_t r1[4], r0[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        r1[c] = (t[c] + (1 << 12) - 1) >> 13;  // Power2Round (Algorithm 35): t = r1 2^13 + r0, r0 in (-2^12, 2^12]
        r0[c] = t[c] - (r1[c] << 13);
    }
    reinterpret_cast<int4*>(t0 + row * 256)[lane] = make_int4(r0[0], r0[1], r0[2], r0[3]);
    // the lane's 40 bits are bits 40 lane ... 40 lane + 39 of the row; dword d = bits 32 d ... 32 d + 31 starts inside lane 4 d / 5
    const uint64_t v = (uint64_t)(uint32_t)r1[0] | ((uint64_t)(uint32_t)r1[1] << 10) | ((uint64_t)(uint32_t)r1[2] << 20) |
                       ((uint64_t)(uint32_t)r1[3] << 30);
    u32_any* out = reinterpret_cast<u32_any*>(pk_rows + key * pk_len + 32 + (size_t)i * (T1_ROW_DW * 4));
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int d = half * 64 + lane;          // the second step has dwords 64 ... 79 in lanes 0 ... 15
        const int la = (4 * d) / 5 & 63, lb = (la + 1) & 63;
        const int sh = (32 * d) % 40;            // 0, 32, 24, 16, 8
        const uint64_t a = (uint64_t)__shfl((unsigned long long)v, la, 64);
        const uint64_t b = (uint64_t)__shfl((unsigned long long)v, lb, 64);
        const uint32_t dw = (uint32_t)(a >> sh) | (uint32_t)(sh > 8 ? b << (40 - sh) : 0);  // sh <= 8: the dword lies inside one lane's bits
        if (d < T1_ROW_DW) out[d] = dw;
    }
}

// ------------------------------------------------------------------------------------------------------------ tr = H(pk, 64)
template <int K>
__global__ __launch_bounds__(64) void k_seed_tr(const uint8_t* __restrict__ pk_rows, uint8_t* __restrict__ tr, size_t n) {
    constexpr int PK_DW = 8 + K * T1_ROW_DW;     // 328 / 488 / 648 dwords; the pad byte opens dword PK_DW
    constexpr int BLOCKS = PK_DW / RATE_DW + 1;  // 10 / 15 / 20: the pad always fits in the last block
    __shared__ uint32_t tile[64 * TILE_STRIDE];
    const int lane = threadIdx.x;
    const size_t base_key = (size_t)blockIdx.x * 64;
    KeccakState st;
    mldsa::keccak_zero(st);
#pragma unroll 1
    for (int b = 0; b < BLOCKS; b++) {
#pragma unroll 2
        for (int t = 0; t < RATE_DW; t++) {
            const int item = t * 64 + lane, o = item / RATE_DW, j = item - o * RATE_DW;
            const int d = b * RATE_DW + j;
            const size_t key = base_key + o;
            uint32_t v = 0;
            if (key < n) {
                if (d < PK_DW) v = load_le32(pk_rows + key * (size_t)(PK_DW * 4) + 4 * d);
                else if (d == PK_DW) v = 0x1Fu;
                if (d == BLOCKS * RATE_DW - 1) v |= 0x80000000u;
            }
            tile[o * TILE_STRIDE + j] = v;
        }
        __syncthreads();
        const uint32_t* row = tile + lane * TILE_STRIDE;
#pragma unroll
        for (int i = 0; i < RATE_DW / 2; i++) {
            st.lo[i] ^= row[2 * i];
            st.hi[i] ^= row[2 * i + 1];
        }
        mldsa::keccak_f1600(st);
        __syncthreads();
    }
    const size_t key = base_key + lane;
    if (key >= n) return;
    u32_any* out = reinterpret_cast<u32_any*>(tr + key * 64);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        out[2 * i] = st.lo[i];
        out[2 * i + 1] = st.hi[i];
    }
}

// ------------------------------------------------------------------------------------------------------------- comparison
// a, b [n][sk_len] (sk_len a multiple of 16) -> match [n]; workgroup = 4 waves = 4 keys
__global__ __launch_bounds__(256) void k_seed_cmp(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ match,
                                                 int sk_vec /* sk_len / 16 */, size_t n) {
    const int lane = threadIdx.x & 63;
    const size_t key = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (key >= n) return;  // the same for the whole wave
    const u32x4_any* pa = reinterpret_cast<const u32x4_any*>(a + key * (size_t)sk_vec * 16);
    const u32x4_any* pb = reinterpret_cast<const u32x4_any*>(b + key * (size_t)sk_vec * 16);
    uint32_t diff = 0;
    for (int c = lane; c < sk_vec; c += 64) {
        const u32x4_any x = pa[c], y = pb[c];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) diff |= (uint32_t)__shfl_xor((int)diff, m, 64);  // wave_or, written out
    if (lane == 0) match[key] = (uint8_t)(diff == 0);
}

// ------------------------------------------------------------------------------------------------------------ host side
// Scratch layout of one expansion pass.  Every part is a multiple of 16 bytes per key, so every array starts 16-byte aligned.
struct ExpandLayout {
    size_t a_hat, s1s2, w, rho_prime, pk, bytes;
};

bool expand_layout(int set, size_t n, ExpandLayout* o) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_SEED_MAX_KEYS) return false;
    const size_t K = (size_t)p.k, L = (size_t)p.l;
    Taker t;
    o->a_hat = t.take(n * 1024 * K * L);
    o->s1s2 = t.take(n * 1024 * (L + K));
    o->w = t.take(n * 1024 * K);
    o->rho_prime = t.take(n * 64);
    o->pk = t.take(n * (size_t)p.pk_len);
    o->bytes = t.at;
    return true;
}

size_t expand_bytes(int set, size_t n) {
    ExpandLayout E;
    return expand_layout(set, n, &E) ? E.bytes : 0;
}

size_t check_bytes(int set, size_t n) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_SEED_MAX_KEYS) return 0;
    return n * (size_t)(p.pk_len + p.sk_len);
}

size_t table_bytes(const mldsa_params& p, size_t n) { return n * (1024 * (size_t)(p.l + 2 * p.k) + 128); }

struct ExpandOut {
    uint8_t *rho, *cap_k, *tr;
    int32_t *s1, *s2, *t0;
    uint8_t* pk;  // may be nullptr
};

// keys key0 ... key0 + n - 1 of the call: `base` holds one pass (expand_layout(set, n))
int expand_pass(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* xi, const ExpandOut& out, size_t key0, size_t n,
                uint8_t* base, hipStream_t s) {
    ExpandLayout E;
    expand_layout(set, n, &E);
    const size_t K = (size_t)p.k, L = (size_t)p.l, pkl = (size_t)p.pk_len;
    int32_t* a_hat = reinterpret_cast<int32_t*>(base + E.a_hat);
    int32_t* s1s2 = reinterpret_cast<int32_t*>(base + E.s1s2);
    int32_t* w = reinterpret_cast<int32_t*>(base + E.w);
    uint8_t* rho_prime = base + E.rho_prime;
    uint8_t* rho = out.rho + key0 * 32;
    uint8_t* pk_rows = out.pk ? out.pk + key0 * pkl : base + E.pk;
    int32_t* s1 = out.s1 + key0 * L * 256;
    int32_t* s2 = out.s2 + key0 * K * 256;
    int32_t* t0 = out.t0 + key0 * K * 256;
    void* st = (void*)s;

    hipLaunchKernelGGL(k_seed_h, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, xi + key0 * 32, (uint32_t)p.k | ((uint32_t)p.l << 8), rho,
                       rho_prime, out.cap_k + key0 * 32, pk_rows, pkl, n);
    LAYER_LAUNCHED("k_seed_h launch");
    LAYER_CORE(mldsa_expand_a(ctx, set, rho, a_hat, n, st), "mldsa_expand_a");
    LAYER_CORE(mldsa_expand_s(ctx, set, rho_prime, s1s2, n, st), "mldsa_expand_s");
    hipLaunchKernelGGL(k_seed_rows, dim3((unsigned)n), dim3(256), 0, s, s1s2, s1, s2, p.k, p.l);
    LAYER_LAUNCHED("k_seed_rows launch");
    LAYER_CORE(mldsa_ntt(ctx, s1, s1, n * L, st), "mldsa_ntt");
    LAYER_CORE(mldsa_ntt(ctx, s2, s2, n * K, st), "mldsa_ntt");
    LAYER_CORE(mldsa_mat_vec_mul(ctx, set, a_hat, s1, w, n, st), "mldsa_mat_vec_mul");
    LAYER_CORE(mldsa_inv_ntt(ctx, w, w, n * K, st), "mldsa_inv_ntt");
    hipLaunchKernelGGL(k_seed_t, dim3((unsigned)((n * K + 3) / 4)), dim3(256), 0, s, w, s1s2, t0, pk_rows, pkl, p.k, p.l, n * K);
    LAYER_LAUNCHED("k_seed_t launch");
    LAYER_CORE(mldsa_ntt(ctx, t0, t0, n * K, st), "mldsa_ntt");
    LAYER_CORE(mldsa_to_mont(ctx, s1, s1, n * L, st), "mldsa_to_mont");
    LAYER_CORE(mldsa_to_mont(ctx, s2, s2, n * K, st), "mldsa_to_mont");
    LAYER_CORE(mldsa_to_mont(ctx, t0, t0, n * K, st), "mldsa_to_mont");
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    uint8_t* tr = out.tr + key0 * 64;
    if (p.k == 4) hipLaunchKernelGGL(k_seed_tr<4>, grid, block, 0, s, pk_rows, tr, n);
    else if (p.k == 6) hipLaunchKernelGGL(k_seed_tr<6>, grid, block, 0, s, pk_rows, tr, n);
    else hipLaunchKernelGGL(k_seed_tr<8>, grid, block, 0, s, pk_rows, tr, n);
    LAYER_LAUNCHED("k_seed_tr launch");
    return MLDSA_OK;
}

// all the keys of a call, in passes of `pass` keys through `base`
int expand_all(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* xi, const ExpandOut& out, size_t n_keys,
               size_t pass, uint8_t* base, hipStream_t s) {
    for (size_t key0 = 0; key0 < n_keys; key0 += pass) {
        const size_t n = n_keys - key0 < pass ? n_keys - key0 : pass;
        const int rc = expand_pass(fn, ctx, set, p, xi, out, key0, n, base, s);
        if (rc != MLDSA_OK) return rc;
    }
    return MLDSA_OK;
}

int check_all(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* xi, const uint8_t* sk, uint8_t* match,
              size_t n_keys, size_t pass, uint8_t* base, hipStream_t s) {
    const size_t skl = (size_t)p.sk_len;
    for (size_t key0 = 0; key0 < n_keys; key0 += pass) {
        const size_t n = n_keys - key0 < pass ? n_keys - key0 : pass;
        uint8_t* sk_gen = base;            // [n][SK_LEN]: a multiple of 16 bytes per key
        uint8_t* pk_gen = base + n * skl;  // [n][PK_LEN]
        LAYER_CORE(mldsa_keygen(ctx, set, xi + key0 * 32, pk_gen, sk_gen, n, (void*)s), "mldsa_keygen");
        hipLaunchKernelGGL(k_seed_cmp, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, sk_gen, sk + key0 * skl, match + key0, (int)(skl / 16), n);
        LAYER_LAUNCHED("k_seed_cmp launch");
    }
    return MLDSA_OK;
}

bool mode_ok(int mode) { return mode == MLDSA_MODE_PURE || mode == MLDSA_MODE_INTERNAL || mode == MLDSA_MODE_PREHASH; }

}  // namespace

extern "C" {

int mldsa_seed_abi_version(void) { return MLDSA_SEED_ABI_VERSION; }

const char* mldsa_seed_last_error(void) { return g_err.c_str(); }

size_t mldsa_seed_expand_scratch_bytes(int set, size_t n_keys) { return expand_bytes(set, n_keys); }

size_t mldsa_seed_check_scratch_bytes(int set, size_t n_keys) { return check_bytes(set, n_keys); }

size_t mldsa_seed_sign_scratch_bytes(int set, size_t n_keys) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n_keys > MLDSA_SEED_MAX_KEYS) return 0;
    return table_bytes(p, n_keys) + expand_bytes(set, n_keys);
}

int mldsa_seed_expand(mldsa_ctx* ctx, int set, const uint8_t* xi, uint8_t* rho, uint8_t* cap_k, uint8_t* tr, int32_t* s_1_hat_mont,
                      int32_t* s_2_hat_mont, int32_t* t_0_hat_mont, uint8_t* pk, size_t n_keys, void* scratch, size_t scratch_bytes,
                      void* stream) {
    const char* fn = "mldsa_seed_expand";
    mldsa_params p;
    const int arc = check_common(fn, ctx, set, n_keys, MLDSA_SEED_MAX_KEYS, "MLDSA_SEED_MAX_KEYS keys", &p);
    if (arc != MLDSA_OK) return arc;
    if (n_keys == 0) return MLDSA_OK;
    if (!xi || !rho || !cap_k || !tr || !s_1_hat_mont || !s_2_hat_mont || !t_0_hat_mont)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(s_1_hat_mont, 16) || !aligned(s_2_hat_mont, 16) || !aligned(t_0_hat_mont, 16))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": the key polynomials must be 16-byte aligned");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    const size_t pass = largest_pass(n_keys, scratch_bytes, [set](size_t n) { return expand_bytes(set, n); });
    if (pass == 0) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_seed_expand_scratch_bytes(set, min(n_keys, 64))");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const ExpandOut out = {rho, cap_k, tr, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont, pk};
    const int rc = expand_all(fn, ctx, set, p, xi, out, n_keys, pass, static_cast<uint8_t*>(scratch), s);
    // the scratch held rho', s1, s2, A s1 and t: cleared whatever happened above
    return cleared(fn, rc, scratch, scratch_bytes, s, false, "mldsa_memset");
}

int mldsa_seed_check(mldsa_ctx* ctx, int set, const uint8_t* xi, const uint8_t* sk, uint8_t* match, size_t n_keys, void* scratch,
                     size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_seed_check";
    mldsa_params p;
    const int arc = check_common(fn, ctx, set, n_keys, MLDSA_SEED_MAX_KEYS, "MLDSA_SEED_MAX_KEYS keys", &p);
    if (arc != MLDSA_OK) return arc;
    if (n_keys == 0) return MLDSA_OK;
    if (!xi || !sk || !match) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    const size_t pass = largest_pass(n_keys, scratch_bytes, [set](size_t n) { return check_bytes(set, n); });
    if (pass == 0) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_seed_check_scratch_bytes(set, min(n_keys, 64))");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const int rc = check_all(fn, ctx, set, p, xi, sk, match, n_keys, pass, static_cast<uint8_t*>(scratch), s);
    // the scratch held the seeds' wire private keys: cleared whatever happened above
    return cleared(fn, rc, scratch, scratch_bytes, s, false, "mldsa_memset");
}

int mldsa_sign_seed(mldsa_ctx* ctx, int set, int mode, const uint8_t* xi, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                    const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, const uint8_t* rnd, uint8_t* sigs, int32_t* status,
                    size_t n_ops, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_sign_seed";
    mldsa_params p;
    // check_common's checks, written out: the mode is refused before the key count
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (mldsa_get_params(set, &p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (!mode_ok(mode)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (n_keys > MLDSA_SEED_MAX_KEYS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_SEED_MAX_KEYS keys");
    if (n_ops == 0) return MLDSA_OK;
    if (n_keys == 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0");
    if (!key_idx && n_keys < n_ops) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys does not cover the batch");
    if (!xi || !msg_off || !rnd || !sigs) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    const size_t table = table_bytes(p, n_keys);
    const size_t pass = scratch_bytes < table ? 0 : largest_pass(n_keys, scratch_bytes - table, [set](size_t n) { return expand_bytes(set, n); });
    if (pass == 0)
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below the key table plus mldsa_seed_expand_scratch_bytes(set, min(n_keys, 64))");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    // the table: the int32 rows first (every array 16-byte aligned), then rho, K, tr
    uint8_t* base = static_cast<uint8_t*>(scratch);
    const size_t K = (size_t)p.k, L = (size_t)p.l;
    ExpandOut t;
    t.s1 = reinterpret_cast<int32_t*>(base);
    t.s2 = t.s1 + n_keys * L * 256;
    t.t0 = t.s2 + n_keys * K * 256;
    t.rho = reinterpret_cast<uint8_t*>(t.t0 + n_keys * K * 256);
    t.cap_k = t.rho + n_keys * 32;
    t.tr = t.cap_k + n_keys * 32;
    t.pk = nullptr;
    int rc = expand_all(fn, ctx, set, p, xi, t, n_keys, pass, base + table, s);
    if (rc == MLDSA_OK) {
        rc = mldsa_sign(ctx, set, mode, t.rho, t.cap_k, t.tr, t.s1, t.s2, t.t0, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, rnd, sigs, status,
                        n_ops, (void*)s);
        if (rc != MLDSA_OK) rc = core_failed(fn, "mldsa_sign", rc);
    }
    // the scratch held the expanded keys and what their expansion left: cleared whatever happened above
    return cleared(fn, rc, scratch, scratch_bytes, s, true, "clearing the scratch");
}

}  // extern "C"
