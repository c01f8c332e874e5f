// libmldsa_keycheck.so (include/mldsa_keycheck.h): strict import of wire-format private keys -- the range check FIPS 204 Algorithm 25
// (skDecode) leaves to the importer, and the pairwise consistency of a key: its t0 and tr fields against its rho, s1, s2, and the key
// against the public key delivered with it -- layered on the core's C ABI.  The core samples A_hat (mldsa_expand_a), computes A s1 in
// one fused kernel (mldsa_verify_arith with z = s1 and all-zero c and t1) and does the import itself (mldsa_sk_expand); the kernels
// here are the steps between them:
//   k_kc_range   one wave per key over the s1 | s2 region in units of 32 coefficients (three dwords of 3-bit fields, four of 4-bit
//                fields per lane): every field of a dword tested at once (field > 2 eta), ORed per vector and across the wave.
//   k_kc_s1      one wave per polynomial of s1: four consecutive fields per lane -> eta - v as int32, the row mldsa_verify_arith reads.
//   k_kc_row     one wave per row (key, i < K), four consecutive coefficients per lane: s2_i and the 13-bit t0_i fields from the wire
//                key, t = A s1 + s2 mod q, Power2Round, r0 against the t0 field, t1 packed into the pk' row with lane shuffles (a
//                lane's 40 bits spread over the row's 80 dwords: whole, consecutive dword stores) and compared with pk; row 0 also
//                carries rho into pk' and compares it.
//   k_kc_tr      tr' = H(pk', 64): one key per lane, rate blocks staged through an LDS tile (the layout layer/layer_dev.h describes;
//                here the loads are unconditional and in flight twelve per lane at a time), compared with bytes 64 ... 127 of the key
//                in registers: tr' is never stored.
//   k_kc_merge   the partial verdicts of a key -> its flag, the consistency bits masked where a range bit is set.
//   k_kc_wipe    mldsa_sk_import: every output row of a flagged key -> zero (the flag is public by then).
// s1, s2, t0 and every comparison against them are secret: no branch, trip count or address depends on them; the differences are
// carried as ORed words and turned into verdict bits by compares the compiler lowers to selects.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_keycheck.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"

namespace {

using namespace mldsa_layer;
using mldsa::load_le32;

constexpr int STAGE_CHUNK = 12;             // loads of k_kc_tr in flight per lane: 34 = 12 + 12 + 10
constexpr int T0_ROW_BYTES = 416;           // 256 coefficients of 13 bits
constexpr int SK_HEAD = 128;                // rho 32 | K 32 | tr 64
constexpr int PART = 16;                    // partial verdict bytes per key: rows 0 ... K - 1, tr at 8, ranges at 9
constexpr int PART_TR = 8, PART_RANGE = 9;

// --------------------------------------------------------------------------------------------------------------- ranges
// 4-bit fields, v > 8: bit 3 set and any of bits 2 ... 0 (adding 7 to them carries into bit 3, never into the next field)
__device__ __forceinline__ uint32_t over8_nibbles(uint32_t x) {
    return x & (((x & 0x77777777u) + 0x77777777u) & 0x88888888u);
}

// 3-bit fields of a 96-bit unit (32 coefficients; field k = bits 3 k ... 3 k + 2), v > 4: bit 2 set and bit 1 or bit 0.  The lower
// bits are moved up to bit 2's place across the dword borders; bit 2 of the fields sits at bits 2, 5 ... of dword 0, 0, 3 ... of
// dword 1 and 1, 4 ... of dword 2.
__device__ __forceinline__ uint32_t over4_triples(uint32_t x0, uint32_t x1, uint32_t x2) {
    const uint32_t lo0 = (x0 << 1) | (x0 << 2);
    const uint32_t lo1 = (x1 << 1) | (x1 << 2) | (x0 >> 31) | (x0 >> 30);
    const uint32_t lo2 = (x2 << 1) | (x2 << 2) | (x1 >> 31) | (x1 >> 30);
    return (x0 & lo0 & 0x24924924u) | (x1 & lo1 & 0x49249249u) | (x2 & lo2 & 0x92492492u);
}

// sk [n][sk_len] -> out[key * out_stride] = MLDSA_KEY_S1_RANGE | MLDSA_KEY_S2_RANGE.  B = bits per field (3: eta = 2, 4: eta = 4); a
// unit is 4 B bytes = 32 coefficients, a polynomial 8 units; units 0 ... s1_units - 1 are s1's.  Workgroup = 4 waves = 4 keys.
template <int B>
__global__ __launch_bounds__(256) void k_kc_range(const uint8_t* __restrict__ sk, size_t sk_len, int s1_units, int n_units,
                                                 uint8_t* __restrict__ out, size_t out_stride, size_t n) {
    const int lane = threadIdx.x & 63;
    const size_t key = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (key >= n) return;  // the same for the whole wave
    const uint8_t* region = sk + key * sk_len + SK_HEAD;
    uint32_t bad1 = 0, bad2 = 0;
    for (int u = lane; u < n_units; u += 64) {  // the bound is the parameter set's
        uint32_t bad;
        if constexpr (B == 4) {
            const u32x4_any x = reinterpret_cast<const u32x4_any*>(region)[u];
            bad = over8_nibbles(x.x) | over8_nibbles(x.y) | over8_nibbles(x.z) | over8_nibbles(x.w);
        } else {
            const u32_any* p = reinterpret_cast<const u32_any*>(region) + 3 * u;
            bad = over4_triples(p[0], p[1], p[2]);
        }
        const uint32_t is_s1 = u < s1_units ? 0xFFFFFFFFu : 0u;  // the unit's number: public
        bad1 |= bad & is_s1;
        bad2 |= bad & ~is_s1;
    }
    bad1 = wave_or(bad1);
    bad2 = wave_or(bad2);
    if (lane == 0) out[key * out_stride] = (uint8_t)((bad1 != 0 ? MLDSA_KEY_S1_RANGE : 0) | (bad2 != 0 ? MLDSA_KEY_S2_RANGE : 0));
}

// ------------------------------------------------------------------------------------------------- fields of s1, s2 and t0
// four consecutive fields of `bits` bits (3 or 4), the lane's, of a packed polynomial: eta - v each.  The lane's 4 * bits bits start at
// bit 4 * bits * lane, inside two bytes.
__device__ __forceinline__ void eta_fields(const uint8_t* poly, int bits, int eta, int lane, int32_t out[4]) {
    const int at = 4 * bits * lane;
    const uint32_t w = ((uint32_t)poly[at >> 3] | ((uint32_t)poly[(at >> 3) + 1] << 8)) >> (at & 7);
    const uint32_t mask = (1u << bits) - 1;
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = eta - (int32_t)((w >> (bits * c)) & mask);
}

// sk [n][sk_len] -> s1 [n][L][256], and the keys' rho 32 bytes apart (rho [n][32]) as mldsa_expand_a reads them; workgroup = 4 waves =
// 4 polynomials
__global__ __launch_bounds__(256) void k_kc_s1(const uint8_t* __restrict__ sk, size_t sk_len, int32_t* __restrict__ s1, uint8_t* __restrict__ rho,
                                              int l_polys, int bits, int eta, size_t n_polys) {
    const int lane = threadIdx.x & 63;
    const size_t poly = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (poly >= n_polys) return;  // the same for the whole wave
    const size_t key = poly / (size_t)l_polys;
    const int j = (int)(poly - key * (size_t)l_polys);
    if (j == 0 && lane < 8) reinterpret_cast<u32_any*>(rho + key * 32)[lane] = load_le32(sk + key * sk_len + 4 * lane);
    int32_t f[4];
    eta_fields(sk + key * sk_len + SK_HEAD + (size_t)j * (32 * bits), bits, eta, lane, f);
    reinterpret_cast<int4*>(s1 + poly * 256)[lane] = make_int4(f[0], f[1], f[2], f[3]);
}

// ------------------------------------------------------------------------------------- t = A s1 + s2, Power2Round, t0, pk'
// w [n][K][256] canonical (mldsa_verify_arith's output); sk [n][sk_len]; pk [n][pk_len] or nullptr; pk_rows: pk', pk_len bytes apart
// (rho | K rows of 320 bytes); part [n][PART].  Workgroup = 4 waves = 4 rows.
__global__ __launch_bounds__(256) void k_kc_row(const int32_t* __restrict__ w, const uint8_t* __restrict__ sk, size_t sk_len,
                                               const uint8_t* __restrict__ pk, uint8_t* __restrict__ pk_rows, size_t pk_len,
                                               uint8_t* __restrict__ part, int k_polys, int l_polys, int bits, int eta, size_t n_rows) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // the same for the whole wave
    const size_t key = row / (size_t)k_polys;
    const int i = (int)(row - key * (size_t)k_polys);
    const uint8_t* key_sk = sk + key * sk_len;
    const uint8_t* key_pk = pk ? pk + key * pk_len : nullptr;
    uint32_t diff_pk = 0;
    if (i == 0 && lane < 8) {  // rho opens pk' (the row's number and the lane: public)
        const uint32_t r = load_le32(key_sk + 4 * lane);
        reinterpret_cast<u32_any*>(pk_rows + key * pk_len)[lane] = r;
        if (key_pk) diff_pk = r ^ load_le32(key_pk + 4 * lane);
    }
    const int4 wv = reinterpret_cast<const int4*>(w + row * 256)[lane];
    int32_t s2[4];
    eta_fields(key_sk + SK_HEAD + (size_t)(l_polys + i) * (32 * bits), bits, eta, lane, s2);
    const int32_t t[4] = {canon(wv.x + s2[0]), canon(wv.y + s2[1]), canon(wv.z + s2[2]), canon(wv.w + s2[3])};
    // the lane's four t0 fields: 52 bits from bit 52 lane of the row, inside seven bytes (two dwords three bytes apart; the last
    // lane's end with the row)
    const uint8_t* t0_row = key_sk + SK_HEAD + (size_t)(l_polys + k_polys) * (32 * bits) + (size_t)i * T0_ROW_BYTES;
    const int at = 52 * lane;
    const uint64_t t0_bits = ((uint64_t)load_le32(t0_row + (at >> 3)) | ((uint64_t)load_le32(t0_row + (at >> 3) + 3) << 24)) >> (at & 7);
    int32_t r1[4];
    uint32_t diff_t0 = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        r1[c] = (t[c] + (1 << 12) - 1) >> 13;  // Power2Round (Algorithm 35): t = r1 2^13 + r0, r0 in (-2^12, 2^12]
        const int32_t r0 = t[c] - (r1[c] << 13);
        diff_t0 |= (uint32_t)((1 << 12) - r0) ^ (uint32_t)((t0_bits >> (13 * c)) & 0x1FFF);  // BitPack(t0, 2^12 - 1, 2^12): field = 2^12 - r0
    }
    // the lane's 40 bits are bits 40 lane ... 40 lane + 39 of the row; dword d = bits 32 d ... 32 d + 31 starts inside lane 4 d / 5
    const uint64_t v = (uint64_t)(uint32_t)r1[0] | ((uint64_t)(uint32_t)r1[1] << 10) | ((uint64_t)(uint32_t)r1[2] << 20) |
                       ((uint64_t)(uint32_t)r1[3] << 30);
    const size_t t1_at = 32 + (size_t)i * (T1_ROW_DW * 4);
    u32_any* out = reinterpret_cast<u32_any*>(pk_rows + key * pk_len + t1_at);
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int d = half * 64 + lane;          // the second step has dwords 64 ... 79 in lanes 0 ... 15
        const int la = (4 * d) / 5 & 63, lb = (la + 1) & 63;
        const int sh = (32 * d) % 40;            // 0, 32, 24, 16, 8
        const uint64_t a = (uint64_t)__shfl((unsigned long long)v, la, 64);
        const uint64_t b = (uint64_t)__shfl((unsigned long long)v, lb, 64);
        const uint32_t dw = (uint32_t)(a >> sh) | (uint32_t)(sh > 8 ? b << (40 - sh) : 0);  // sh <= 8: the dword lies inside one lane's bits
        if (d < T1_ROW_DW) {
            out[d] = dw;
            if (key_pk) diff_pk |= dw ^ load_le32(key_pk + t1_at + 4 * d);
        }
    }
    diff_t0 = wave_or(diff_t0);
    diff_pk = wave_or(diff_pk);
    if (lane == 0) part[key * PART + i] = (uint8_t)((diff_t0 != 0 ? MLDSA_KEY_T0 : 0) | (diff_pk != 0 ? MLDSA_KEY_PK : 0));
}

// -------------------------------------------------------------------------------------- tr' = H(pk', 64) against the tr field
template <int K>
__global__ __launch_bounds__(64) void k_kc_tr(const uint8_t* __restrict__ pk_rows, const uint8_t* __restrict__ sk, size_t sk_len,
                                             uint8_t* __restrict__ part, size_t n) {
    constexpr int PK_DW = 8 + K * T1_ROW_DW;     // 328 / 488 / 648 dwords; the pad byte opens dword PK_DW
    constexpr int BLOCKS = PK_DW / RATE_DW + 1;  // 10 / 15 / 20: the pad always fits in the last block
    __shared__ uint32_t tile[64 * TILE_STRIDE];
    const int lane = threadIdx.x;
    const size_t base_key = (size_t)blockIdx.x * 64;
    KeccakState st;
    mldsa::keccak_zero(st);
    const uint8_t* first_row = pk_rows + base_key * (size_t)(PK_DW * 4);
#pragma unroll 1
    for (int b = 0; b < BLOCKS; b++) {
        // the lanes' words of rate block b (consecutive lanes on consecutive dwords of one key), padding included, STAGE_CHUNK per lane
        // at a time.  Every load of a chunk is issued whatever the item -- an item without a dword of pk' (past the key, past the
        // batch) reads the block's first dword and drops it --, so that they are in flight together and none waits behind a branch
#pragma unroll 1
        for (int t0 = 0; t0 < RATE_DW; t0 += STAGE_CHUNK) {
            uint32_t staged[STAGE_CHUNK];
#pragma unroll
            for (int u = 0; u < STAGE_CHUNK; u++) {
                const int item = (t0 + u) * 64 + lane, o = item / RATE_DW, j = item - o * RATE_DW;
                const int d = b * RATE_DW + j;
                const bool has = d < PK_DW && base_key + o < n && t0 + u < RATE_DW;
                const uint32_t v = load_le32(first_row + (has ? (uint32_t)(o * (PK_DW * 4) + 4 * d) : 0u));  // (32-bit offsets from a wave-uniform base)
                staged[u] = (has ? v : (d == PK_DW ? 0x1Fu : 0u)) | (d == BLOCKS * RATE_DW - 1 ? 0x80000000u : 0u);
            }
#pragma unroll
            for (int u = 0; u < STAGE_CHUNK; u++) {
                const int item = (t0 + u) * 64 + lane, o = item / RATE_DW, j = item - o * RATE_DW;
                if (t0 + u < RATE_DW) tile[o * TILE_STRIDE + j] = staged[u];
            }
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
    const uint8_t* tr = sk + key * sk_len + 64;
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= (st.lo[i] ^ load_le32(tr + 8 * i)) | (st.hi[i] ^ load_le32(tr + 8 * i + 4));
    part[key * PART + PART_TR] = (uint8_t)(diff != 0 ? MLDSA_KEY_TR : 0);
}

// ------------------------------------------------------------------------------------------------------------ the verdict
// part [n][PART] -> flag [n]: a range bit hides the consistency bits
__global__ __launch_bounds__(256) void k_kc_merge(const uint8_t* __restrict__ part, uint8_t* __restrict__ flag, int k_polys, size_t n) {
    const size_t key = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (key >= n) return;
    const uint4 p = reinterpret_cast<const uint4*>(part)[key];
    const uint32_t rows_lo = p.x, rows_hi = k_polys > 4 ? p.y & (k_polys > 6 ? 0xFFFFFFFFu : 0x0000FFFFu) : 0u;
    uint32_t cons = rows_lo | rows_hi;
    cons |= cons >> 16;
    cons = (cons | (cons >> 8) | p.z) & (MLDSA_KEY_T0 | MLDSA_KEY_TR | MLDSA_KEY_PK);  // p.z: byte 8 = tr
    const uint32_t range = (p.z >> 8) & (MLDSA_KEY_S1_RANGE | MLDSA_KEY_S2_RANGE);
    const uint32_t keep = range != 0 ? 0u : 0xFFu;
    flag[key] = (uint8_t)(range | (cons & keep));
}

// every output row of a flagged key -> zero; one workgroup per key
__global__ __launch_bounds__(256) void k_kc_wipe(const uint8_t* __restrict__ flag, uint8_t* __restrict__ rho, uint8_t* __restrict__ cap_k,
                                                uint8_t* __restrict__ tr, int32_t* __restrict__ s1, int32_t* __restrict__ s2,
                                                int32_t* __restrict__ t0, int k_polys, int l_polys) {
    const size_t key = blockIdx.x;
    if (flag[key] == 0) return;  // public
    const int t = threadIdx.x;
    if (t < 8) reinterpret_cast<u32_any*>(rho + key * 32)[t] = 0;
    else if (t < 16) reinterpret_cast<u32_any*>(cap_k + key * 32)[t - 8] = 0;
    else if (t < 32) reinterpret_cast<u32_any*>(tr + key * 64)[t - 16] = 0;
    const int4 zero = make_int4(0, 0, 0, 0);
    int4* d1 = reinterpret_cast<int4*>(s1) + key * (size_t)l_polys * 64;
    int4* d2 = reinterpret_cast<int4*>(s2) + key * (size_t)k_polys * 64;
    int4* d0 = reinterpret_cast<int4*>(t0) + key * (size_t)k_polys * 64;
    for (int c = t; c < l_polys * 64; c += 256) d1[c] = zero;
    for (int c = t; c < k_polys * 64; c += 256) {
        d2[c] = zero;
        d0[c] = zero;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// Scratch layout of passes of up to n keys.  Every part is a multiple of 16 bytes per key, so every array starts 16-byte aligned.
struct Layout {
    size_t a_hat, s1, w, zero, pk, part, bytes;
};

bool layout(int set, size_t n, Layout* o) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_KEYCHECK_MAX_KEYS) return false;
    const size_t K = (size_t)p.k, L = (size_t)p.l;
    Taker t;
    o->a_hat = t.take(n * 1024 * K * L);
    o->s1 = t.take(n * 1024 * L);
    o->w = t.take(n * 1024 * K);
    o->zero = t.take(n * 1024 * (K + 1));  // c [n][256], then t1 [n][K][256]
    o->pk = t.take(n * (size_t)p.pk_len);
    o->part = t.take(n * PART);
    o->bytes = t.at;
    return true;
}

size_t pass_bytes(int set, size_t n) {
    Layout Y;
    return layout(set, n, &Y) ? Y.bytes : 0;
}

int field_bits(const mldsa_params& p) { return p.eta == 2 ? 3 : 4; }

// the range bits of n keys -> out[key * out_stride]
int launch_range(const char* fn, const mldsa_params& p, const uint8_t* sk, uint8_t* out, size_t out_stride, size_t n, hipStream_t s) {
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const int s1_units = p.l * 8, n_units = (p.l + p.k) * 8;
    if (field_bits(p) == 3) hipLaunchKernelGGL(k_kc_range<3>, grid, block, 0, s, sk, (size_t)p.sk_len, s1_units, n_units, out, out_stride, n);
    else hipLaunchKernelGGL(k_kc_range<4>, grid, block, 0, s, sk, (size_t)p.sk_len, s1_units, n_units, out, out_stride, n);
    LAYER_LAUNCHED("k_kc_range launch");
    return MLDSA_OK;
}

// all the keys of a call, in passes of `pass` keys through `base` (layout(set, pass))
int pair_all(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* sk, const uint8_t* pk, uint8_t* flag, size_t n_keys,
             size_t pass, uint8_t* base, hipStream_t s) {
    Layout Y;
    layout(set, pass, &Y);
    const size_t K = (size_t)p.k, L = (size_t)p.l, pkl = (size_t)p.pk_len, skl = (size_t)p.sk_len;
    const int bits = field_bits(p);
    int32_t* a_hat = reinterpret_cast<int32_t*>(base + Y.a_hat);
    int32_t* s1 = reinterpret_cast<int32_t*>(base + Y.s1);
    int32_t* w = reinterpret_cast<int32_t*>(base + Y.w);
    int32_t* zero_c = reinterpret_cast<int32_t*>(base + Y.zero);
    int32_t* zero_t1 = zero_c + pass * 256;
    uint8_t* pk_rows = base + Y.pk;
    uint8_t* part = base + Y.part;
    void* st = (void*)s;
    // nothing below writes the c and t1 rows: cleared once for every pass
    LAYER_CORE(mldsa_memset(base + Y.zero, 0, pass * 1024 * (K + 1), st), "mldsa_memset");
    for (size_t key0 = 0; key0 < n_keys; key0 += pass) {
        const size_t n = n_keys - key0 < pass ? n_keys - key0 : pass;
        const uint8_t* sk0 = sk + key0 * skl;
        const uint8_t* pk0 = pk ? pk + key0 * pkl : nullptr;
        const int rc = launch_range(fn, p, sk0, part + PART_RANGE, PART, n, s);
        if (rc != MLDSA_OK) return rc;
        // rho [n][32] lies at the head of the rows A s1 is written to afterwards: mldsa_expand_a has read it by then (stream order)
        uint8_t* rho = reinterpret_cast<uint8_t*>(w);
        hipLaunchKernelGGL(k_kc_s1, dim3((unsigned)((n * L + 3) / 4)), dim3(256), 0, s, sk0, skl, s1, rho, p.l, bits, p.eta, n * L);
        LAYER_LAUNCHED("k_kc_s1 launch");
        LAYER_CORE(mldsa_expand_a(ctx, set, rho, a_hat, n, st), "mldsa_expand_a");
        LAYER_CORE(mldsa_verify_arith(ctx, set, a_hat, s1, zero_c, zero_t1, w, n, st), "mldsa_verify_arith");
        hipLaunchKernelGGL(k_kc_row, dim3((unsigned)((n * K + 3) / 4)), dim3(256), 0, s, w, sk0, skl, pk0, pk_rows, pkl, part, p.k, p.l, bits,
                           p.eta, n * K);
        LAYER_LAUNCHED("k_kc_row launch");
        const dim3 grid((unsigned)((n + 63) / 64)), block(64);
        if (p.k == 4) hipLaunchKernelGGL(k_kc_tr<4>, grid, block, 0, s, pk_rows, sk0, skl, part, n);
        else if (p.k == 6) hipLaunchKernelGGL(k_kc_tr<6>, grid, block, 0, s, pk_rows, sk0, skl, part, n);
        else hipLaunchKernelGGL(k_kc_tr<8>, grid, block, 0, s, pk_rows, sk0, skl, part, n);
        LAYER_LAUNCHED("k_kc_tr launch");
        hipLaunchKernelGGL(k_kc_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, flag + key0, p.k, n);
        LAYER_LAUNCHED("k_kc_merge launch");
    }
    return MLDSA_OK;
}

// scratch of a pair check: MLDSA_ERR_PARAM / MLDSA_ERR_NOMEM, or the pass in *pass
int check_scratch(const char* fn, int set, size_t n_keys, const void* scratch, size_t scratch_bytes, size_t* pass) {
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    *pass = largest_pass(n_keys, scratch_bytes, [set](size_t n) { return pass_bytes(set, n); });
    if (*pass == 0) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_keycheck_scratch_bytes(set, min(n_keys, 64))");
    return MLDSA_OK;
}

struct ImportOut {
    uint8_t *rho, *cap_k, *tr;
    int32_t *s1, *s2, *t0;
};

// every output row of a flagged key -> zero
int launch_wipe(const char* fn, const mldsa_params& p, const uint8_t* flag, const ImportOut& o, size_t n_keys, hipStream_t s) {
    hipLaunchKernelGGL(k_kc_wipe, dim3((unsigned)n_keys), dim3(256), 0, s, flag, o.rho, o.cap_k, o.tr, o.s1, o.s2, o.t0, p.k, p.l);
    LAYER_LAUNCHED("k_kc_wipe launch");
    return MLDSA_OK;
}

// the pair check behind its argument checks (wipe: the fields of mldsa_sk_import, or nullptr), the scratch zeroed behind the last
// kernel whatever happened
int pair_checked(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* sk, const uint8_t* pk, uint8_t* flag,
                 size_t n_keys, size_t pass, void* scratch, size_t scratch_bytes, const ImportOut* wipe, hipStream_t s) {
    int rc = pair_all(fn, ctx, set, p, sk, pk, flag, n_keys, pass, static_cast<uint8_t*>(scratch), s);
    if (rc == MLDSA_OK && wipe) rc = launch_wipe(fn, p, flag, *wipe, n_keys, s);
    // the scratch held s1 and A s1: cleared whatever happened above
    return cleared(fn, rc, scratch, scratch_bytes, s, false, "mldsa_memset");
}

}  // namespace

extern "C" {

int mldsa_keycheck_abi_version(void) { return MLDSA_KEYCHECK_ABI_VERSION; }

const char* mldsa_keycheck_last_error(void) { return g_err.c_str(); }

size_t mldsa_keycheck_scratch_bytes(int set, size_t n_keys) { return pass_bytes(set, n_keys); }

int mldsa_sk_range_check(mldsa_ctx* ctx, int set, const uint8_t* sk, uint8_t* flag, size_t n_keys, void* stream) {
    const char* fn = "mldsa_sk_range_check";
    mldsa_params p;
    const int arc = check_common(fn, ctx, set, n_keys, MLDSA_KEYCHECK_MAX_KEYS, "MLDSA_KEYCHECK_MAX_KEYS keys", &p);
    if (arc != MLDSA_OK) return arc;
    if (n_keys == 0) return MLDSA_OK;
    if (!sk || !flag) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    LAYER_ON_DEVICE(ctx);
    return launch_range(fn, p, sk, flag, 1, n_keys, (hipStream_t)stream);
}

int mldsa_keypair_check(mldsa_ctx* ctx, int set, const uint8_t* sk, const uint8_t* pk, uint8_t* flag, size_t n_keys, void* scratch,
                        size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_keypair_check";
    mldsa_params p;
    const int arc = check_common(fn, ctx, set, n_keys, MLDSA_KEYCHECK_MAX_KEYS, "MLDSA_KEYCHECK_MAX_KEYS keys", &p);
    if (arc != MLDSA_OK) return arc;
    if (n_keys == 0) return MLDSA_OK;
    if (!sk || !flag) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    size_t pass = 0;
    const int src = check_scratch(fn, set, n_keys, scratch, scratch_bytes, &pass);
    if (src != MLDSA_OK) return src;
    LAYER_ON_DEVICE(ctx);
    return pair_checked(fn, ctx, set, p, sk, pk, flag, n_keys, pass, scratch, scratch_bytes, nullptr, (hipStream_t)stream);
}

int mldsa_sk_import(mldsa_ctx* ctx, int set, int level, const uint8_t* sk, const uint8_t* pk, uint8_t* rho, uint8_t* cap_k, uint8_t* tr,
                    int32_t* s_1_hat_mont, int32_t* s_2_hat_mont, int32_t* t_0_hat_mont, uint8_t* flag, size_t n_keys, void* scratch,
                    size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_sk_import";
    mldsa_params p;
    const int arc = check_common(fn, ctx, set, n_keys, MLDSA_KEYCHECK_MAX_KEYS, "MLDSA_KEYCHECK_MAX_KEYS keys", &p);
    if (arc != MLDSA_OK) return arc;
    if (level != MLDSA_KEYCHECK_RANGE && level != MLDSA_KEYCHECK_PAIR) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown level");
    if (n_keys == 0) return MLDSA_OK;
    if (!sk || !flag || !rho || !cap_k || !tr || !s_1_hat_mont || !s_2_hat_mont || !t_0_hat_mont)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(s_1_hat_mont, 16) || !aligned(s_2_hat_mont, 16) || !aligned(t_0_hat_mont, 16))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": the key polynomials must be 16-byte aligned");
    size_t pass = 0;
    if (level == MLDSA_KEYCHECK_PAIR) {
        const int src = check_scratch(fn, set, n_keys, scratch, scratch_bytes, &pass);
        if (src != MLDSA_OK) return src;
    }
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const ImportOut out = {rho, cap_k, tr, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont};
    const int xrc = mldsa_sk_expand(ctx, set, sk, rho, cap_k, tr, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont, n_keys, stream);
    if (xrc != MLDSA_OK) return core_failed(fn, "mldsa_sk_expand", xrc);  // (nothing has touched the scratch)
    if (level == MLDSA_KEYCHECK_PAIR) return pair_checked(fn, ctx, set, p, sk, pk, flag, n_keys, pass, scratch, scratch_bytes, &out, s);
    const int rc = launch_range(fn, p, sk, flag, 1, n_keys, s);
    return rc == MLDSA_OK ? launch_wipe(fn, p, flag, out, n_keys, s) : rc;
}

}  // extern "C"
