// libmldsa_mu.so (include/mldsa_mu.h): ML-DSA.Sign_internal / Verify_internal from an externally computed mu (FIPS 204 Algorithms 7
// and 8), layered on the core's seam-level C ABI.  The core does all the arithmetic and every codec on int32 polynomials
// (mldsa_sig_decode, mldsa_sample_in_ball, mldsa_expand_a, mldsa_verify_arith, mldsa_infinity_norm, mldsa_expand_mask, mldsa_ntt,
// mldsa_inv_ntt, mldsa_mat_vec_mul, mldsa_pointwise_mont, mldsa_sig_encode); the kernels here are the steps that touch mu or that
// would cost several int32 round trips through HBM as seam calls:
//   k_mu_ext     mu = H(tr | M', 64), one message per lane, every rate block absorbed straight from tr / prefix / message: no LDS.
//   k_commit     the commitment hash of both directions: canonical w -> UseHint(h, w) (verify) or HighBits(w) (sign) -> w1Encode ->
//                c_tilde = H(mu | w1, lambda / 4).  One sponge state per lane; for every rate block the wave packs the 64 ops' 34
//                dwords cooperatively (consecutive lanes on consecutive dwords of one op: coalesced reads of w and h) into an LDS
//                tile (the layout layer/layer_dev.h describes), then each lane absorbs its own row.  Verify compares with the signature's c_tilde and folds in the decode
//                verdict, ||z||inf, mu_flag and the key flag; sign stores c_tilde.
//   k_rhopp      rho'' = H(K[key] | rnd | mu, 64): one block per op, K gathered by the op's key index.
//   k_accept     one signing round's accept step for one row per workgroup (one coefficient per thread): z = y + c s1,
//                r0 = LowBits(w - c s2), ||z||inf < gamma1 - beta, ||r0||inf < gamma2 - beta, ||c t0||inf < gamma2,
//                h = MakeHint(-c t0, w - c s2 + c t0) with weight <= omega; accepted rows write z, h and c_tilde where
//                mldsa_sig_encode finds them, the others advance kappa.
//   k_count, k_offsets, k_compact, k_gather_rows   the unfinished rows are counted every round (the host reads that one word);
//                once at most half of the rows are unfinished, an exclusive scan gives them new, dense row numbers, their state
//                (mu, rho'', kappa, op, key) moves to the other state set, and their A_hat rows to the other A_hat buffer.  A_hat
//                is expanded once per pass; each gather copies at most half of what the one before did.
// The rounds of an op always test kappa = 0, L, 2 L, ... in order, so the signature is the one of the first accepted kappa.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_mu.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"

namespace {

using namespace mldsa_layer;
using mldsa::Q;
using mldsa::SHAKE256_RATE;
using mldsa::load_le32;

constexpr int SCAN_BLOCK = 256;  // rows per workgroup of the scan

// -------------------------------------------------------------------------------------------------------------------- mu
// The checks are k_mu's: the call vouches for [off[0], off[n_ops]); an op whose pair is not in order inside it is refused unread
// (flag 2), then a ctx longer than 255 bytes (flag 1), then a key index outside the table (flag 2).
__global__ __launch_bounds__(64) void k_mu_ext(const uint8_t* __restrict__ tr, uint32_t n_keys, const uint32_t* __restrict__ key_idx, int mode,
                                               const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ msg_off,
                                               const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off,
                                               uint8_t* __restrict__ mu, int32_t* __restrict__ mu_flag, size_t n_ops) {
    const int lane = threadIdx.x;
    const size_t op = (size_t)blockIdx.x * 64 + lane;
    const bool valid = op < n_ops;
    const uint8_t *trp = nullptr, *mp = nullptr, *cp = nullptr;
    size_t mlen = 0, clen = 0;
    bool live = false;
    if (valid) {
        const uint64_t m0 = msg_off[op], m1 = msg_off[op + 1];
        bool bad_off = !(msg_off[0] <= m0 && m0 <= m1 && m1 <= msg_off[n_ops]);
        mp = msgs + m0;
        mlen = (size_t)(m1 - m0);
        bad_off |= mlen != 0 && msgs == nullptr;
        if (ctx_off) {
            const uint64_t c0 = ctx_off[op], c1 = ctx_off[op + 1];
            bad_off |= !(ctx_off[0] <= c0 && c0 <= c1 && c1 <= ctx_off[n_ops]);
            cp = ctxs + c0;
            clen = (size_t)(c1 - c0);
            bad_off |= clen != 0 && ctxs == nullptr;
        }
        const size_t key = key_idx ? (size_t)key_idx[op] : op;
        const int flag = bad_off ? 2 : clen > 255 ? 1 : key >= n_keys ? 2 : 0;
        if (mu_flag) mu_flag[op] = flag;
        live = flag == 0;
        if (live) trp = tr + key * 64;
        else mlen = clen = 0;
    }
    const size_t pre = mode == MLDSA_MODE_INTERNAL ? 0 : 2 + clen;
    const size_t total = live ? 64 + pre + mlen : 0;
    const size_t my_blocks = live ? total / SHAKE256_RATE + 1 : 0;  // the pad always fits in the last block
    size_t max_blocks = my_blocks;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const size_t o = (size_t)__shfl_xor((unsigned long long)max_blocks, m);
        max_blocks = o > max_blocks ? o : max_blocks;
    }
    auto byte_at = [&](size_t pos) -> uint32_t {
        if (pos < total) {
            if (pos < 64) return trp[pos];
            if (pos < 64 + pre) {
                const size_t q = pos - 64;
                return q == 0 ? (mode == MLDSA_MODE_PREHASH ? 1u : 0u) : q == 1 ? (uint32_t)clen : cp[q - 2];
            }
            return mp[pos - 64 - pre];
        }
        return pos == total ? 0x1Fu : 0u;
    };
    // whole dwords of tr and of the message are one byte-granular load each; only a dword that straddles a boundary (prefix,
    // message end, pad) is assembled from bytes
    auto dword_at = [&](size_t pos) -> uint32_t {
        if (pos + 4 <= 64) return load_le32(trp + pos);
        if (pos >= 64 + pre && pos + 4 <= total) return load_le32(mp + (pos - 64 - pre));
        if (pos > total) return 0u;
        return byte_at(pos) | (byte_at(pos + 1) << 8) | (byte_at(pos + 2) << 16) | (byte_at(pos + 3) << 24);
    };
    KeccakState st;
    mldsa::keccak_zero(st);
    for (size_t b = 0; b < max_blocks; b++) {
        if (b < my_blocks) {
            const size_t base = b * SHAKE256_RATE;
#pragma unroll
            for (int w = 0; w < SHAKE256_RATE / 8; w++) {
                st.lo[w] ^= dword_at(base + 8 * w);
                st.hi[w] ^= dword_at(base + 8 * w + 4);
            }
            if (b == my_blocks - 1) st.hi[SHAKE256_RATE / 8 - 1] ^= 0x80000000u;
            mldsa::keccak_f1600(st);
        }
    }
    if (valid) {
        u32_any* out = reinterpret_cast<u32_any*>(mu + op * MLDSA_MU_LEN);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            out[2 * i] = live ? st.lo[i] : 0u;
            out[2 * i + 1] = live ? st.hi[i] : 0u;
        }
    }
}

// -------------------------------------------------------------------------------------------------------- commitment hash
// dword e of w1Encode(UseHint(h, w)) (h = nullptr: HighBits) of one op: BITS-bit fields of the op's K * 256 coefficients
template <bool G2HI>
__device__ __forceinline__ uint32_t w1_dword(const int32_t* __restrict__ w, const int32_t* __restrict__ h, int e) {
    if constexpr (G2HI) {  // 4-bit fields: coefficients 8 e ... 8 e + 7
        const int4* wp = reinterpret_cast<const int4*>(w + 8 * e);
        const int4 a = wp[0], b = wp[1];
        int4 ha = make_int4(0, 0, 0, 0), hb = ha;
        if (h) {
            const int4* hp = reinterpret_cast<const int4*>(h + 8 * e);
            ha = hp[0];
            hb = hp[1];
        }
        const int32_t r[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const int32_t hh[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) v |= (uint32_t)mldsa::use_hint<true>(hh[i] != 0, r[i]) << (4 * i);
        return v;
    } else {  // 6-bit fields: the dword's 32 bits start inside coefficient c0 and end inside c0 + 5
        const int c0 = (32 * e) / 6, sh = 32 * e - 6 * c0;  // sh in {0, 2, 4}
        uint64_t acc = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) acc |= (uint64_t)(uint32_t)mldsa::use_hint<false>(h ? h[c0 + i] != 0 : 0, w[c0 + i]) << (6 * i);
        return (uint32_t)(acc >> sh);
    }
}

struct CommitVerify {
    const uint8_t* sigs;     // the pass's first signature
    size_t sig_len;
    const uint8_t* dec_ok;   // mldsa_sig_decode's verdict
    const int32_t* znorm;
    int32_t zbound;          // gamma1 - beta
    const int32_t* mu_flag;  // may be nullptr
    const int32_t* key_bad;
    uint8_t* ok;
};

// w [n][K][256] canonical, h [n][K][256] of 0 / 1 (VERIFY), mu [n][64]; VERIFY: ok[n]; else c_tilde [n][CT]
template <int K, bool G2HI, int CT, bool VERIFY>
__global__ __launch_bounds__(64) void k_commit(const int32_t* __restrict__ w, const int32_t* __restrict__ h, const uint8_t* __restrict__ mu,
                                               size_t n, uint8_t* __restrict__ c_tilde, CommitVerify vd) {
    constexpr int W1_DW = K * 256 * (G2HI ? 4 : 6) / 32;
    constexpr int TOTAL_DW = 16 + W1_DW;           // mu | w1: 208 or 272 dwords, the pad byte opens dword TOTAL_DW
    constexpr int BLOCKS = TOTAL_DW / RATE_DW + 1;  // the pad always fits in the last block
    __shared__ uint32_t tile[64 * TILE_STRIDE];
    const int lane = threadIdx.x;
    const size_t base_op = (size_t)blockIdx.x * 64;
    KeccakState st;
    mldsa::keccak_zero(st);
#pragma unroll 1
    for (int b = 0; b < BLOCKS; b++) {
#pragma unroll 2
        for (int t = 0; t < RATE_DW; t++) {
            const int item = t * 64 + lane, o = item / RATE_DW, j = item - o * RATE_DW;
            const int d = b * RATE_DW + j;
            const size_t op = base_op + o;
            uint32_t v = 0;
            if (op < n) {
                if (d < 16) v = load_le32(mu + op * MLDSA_MU_LEN + 4 * d);
                else if (d < TOTAL_DW) v = w1_dword<G2HI>(w + op * (K * 256), VERIFY ? h + op * (K * 256) : nullptr, d - 16);
                else if (d == TOTAL_DW) v = 0x1Fu;
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
    const size_t op = base_op + lane;
    if (op >= n) return;
    if constexpr (VERIFY) {
        const uint8_t* c0 = vd.sigs + op * vd.sig_len;  // c_tilde opens the signature (Algorithm 26)
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < CT / 8; i++) diff |= (st.lo[i] ^ load_le32(c0 + 8 * i)) | (st.hi[i] ^ load_le32(c0 + 8 * i + 4));
        const bool flagged = (vd.mu_flag && vd.mu_flag[op] != 0) || vd.key_bad[op] != 0;
        vd.ok[op] = (uint8_t)(diff == 0 && vd.dec_ok[op] != 0 && vd.znorm[op] < vd.zbound && !flagged);
    } else {
        uint32_t* out = reinterpret_cast<uint32_t*>(c_tilde + op * CT);
#pragma unroll
        for (int i = 0; i < CT / 8; i++) {
            out[2 * i] = st.lo[i];
            out[2 * i + 1] = st.hi[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------------- verify: key gather
// rho and t1 of the op's key, one workgroup per op; an index outside the table reads key 0 and raises the op's key flag
__global__ __launch_bounds__(256) void k_gather_pk(const uint8_t* __restrict__ rho, const int32_t* __restrict__ t1, uint32_t n_keys,
                                                  const uint32_t* __restrict__ key_idx, size_t op0, int k_polys,
                                                  uint8_t* __restrict__ rho_op, int32_t* __restrict__ t1_op, int32_t* __restrict__ key_bad) {
    const size_t i = blockIdx.x, g = op0 + i;
    size_t key = key_idx ? (size_t)key_idx[g] : g;
    const bool bad = key >= n_keys;
    if (bad) key = 0;
    const int t = threadIdx.x;
    if (t == 0) key_bad[i] = bad;
    if (t < 8) reinterpret_cast<uint32_t*>(rho_op + i * 32)[t] = load_le32(rho + key * 32 + 4 * t);
    const int4* src = reinterpret_cast<const int4*>(t1 + key * (size_t)k_polys * 256);
    int4* dst = reinterpret_cast<int4*>(t1_op + i * (size_t)k_polys * 256);
    for (int c = t; c < k_polys * 64; c += 256) dst[c] = src[c];
}

// --------------------------------------------------------------------------------------------------------- sign: row state
// One state set of the rows of a pass; the signer keeps two and compaction moves the unfinished rows from one to the other.
struct RowState {
    uint8_t* mu;      // [rows][64]
    uint8_t* rhopp;   // [rows][64]
    uint16_t* kappa;  // [rows]
    uint32_t* op;     // [rows] the pass's op the row signs
    uint32_t* key;    // [rows] its key (0 for a refused op)
    int32_t* done;    // [rows]
};

// row i = op i of the pass: flags -> status, the op's mu, key and rho; a refused op starts finished
__global__ __launch_bounds__(256) void k_sign_init(const uint8_t* __restrict__ rho, uint32_t n_keys, const uint32_t* __restrict__ key_idx,
                                                  const uint8_t* __restrict__ mu, const int32_t* __restrict__ mu_flag, size_t op0, uint32_t n,
                                                  RowState s, uint8_t* __restrict__ rho_op, int32_t* __restrict__ bad, int32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t g = op0 + i;
    const int flag = mu_flag ? mu_flag[g] : 0;
    size_t key = key_idx ? (size_t)key_idx[g] : g;
    const int st = flag == 1 ? MLDSA_ERR_CTX_LEN : (flag != 0 || key >= n_keys) ? MLDSA_ERR_PARAM : MLDSA_OK;
    if (st != MLDSA_OK) key = 0;
    if (status) status[g] = st;
    bad[i] = st != MLDSA_OK;
    s.op[i] = i;
    s.key[i] = (uint32_t)key;
    s.kappa[i] = 0;
    s.done[i] = st != MLDSA_OK;
    uint32_t* m = reinterpret_cast<uint32_t*>(s.mu + (size_t)i * 64);
#pragma unroll
    for (int k = 0; k < 16; k++) m[k] = st == MLDSA_OK ? load_le32(mu + g * 64 + 4 * k) : 0u;
    uint32_t* r = reinterpret_cast<uint32_t*>(rho_op + (size_t)i * 32);
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = load_le32(rho + key * 32 + 4 * k);
}

// rho'' = H(K | rnd | mu, 64) (Algorithm 7 line 7): 128 bytes, one rate block
__global__ __launch_bounds__(64) void k_rhopp(const uint8_t* __restrict__ cap_k, const uint8_t* __restrict__ rnd /* the pass's first row */,
                                             RowState s, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* kp = cap_k + (size_t)s.key[i] * 32;
    const uint8_t* rp = rnd + (size_t)i * 32;
    const uint8_t* mp = s.mu + (size_t)i * 64;
    KeccakState st;
    mldsa::keccak_zero(st);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        st.lo[w] = load_le32(kp + 8 * w);
        st.hi[w] = load_le32(kp + 8 * w + 4);
        st.lo[4 + w] = load_le32(rp + 8 * w);
        st.hi[4 + w] = load_le32(rp + 8 * w + 4);
    }
#pragma unroll
    for (int w = 0; w < 8; w++) {
        st.lo[8 + w] = load_le32(mp + 8 * w);
        st.hi[8 + w] = load_le32(mp + 8 * w + 4);
    }
    mldsa::shake_pad<SHAKE256_RATE, 128>(st);
    mldsa::keccak_f1600(st);
    uint32_t* out = reinterpret_cast<uint32_t*>(s.rhopp + (size_t)i * 64);
#pragma unroll
    for (int w = 0; w < 8; w++) {
        out[2 * w] = st.lo[w];
        out[2 * w + 1] = st.hi[w];
    }
}

// Row j of the current arrangement: its A_hat row from row src_of[j] of the previous arrangement (a_old = nullptr: A_hat was just
// expanded in this order) and s1 | s2 | t0 of its key from the key table.  One workgroup per row.
__global__ __launch_bounds__(256) void k_gather_rows(const int32_t* __restrict__ a_old, int32_t* __restrict__ a_new, const uint32_t* __restrict__ src_of,
                                                    const uint32_t* __restrict__ key, const int32_t* __restrict__ s1, const int32_t* __restrict__ s2,
                                                    const int32_t* __restrict__ t0, int32_t* __restrict__ sec, int k_polys, int l_polys) {
    const size_t j = blockIdx.x;
    const int t = threadIdx.x;
    if (a_old) {
        const size_t row = (size_t)k_polys * l_polys * 64;  // int4s
        const int4* src = reinterpret_cast<const int4*>(a_old) + (size_t)src_of[j] * row;
        int4* dst = reinterpret_cast<int4*>(a_new) + j * row;
        for (size_t c = t; c < row; c += 256) dst[c] = src[c];
    }
    const size_t kk = key[j];
    int4* dst = reinterpret_cast<int4*>(sec) + j * (size_t)(l_polys + 2 * k_polys) * 64;
    const int4* p1 = reinterpret_cast<const int4*>(s1) + kk * (size_t)l_polys * 64;
    const int4* p2 = reinterpret_cast<const int4*>(s2) + kk * (size_t)k_polys * 64;
    const int4* p0 = reinterpret_cast<const int4*>(t0) + kk * (size_t)k_polys * 64;
    for (int c = t; c < l_polys * 64; c += 256) dst[c] = p1[c];
    dst += l_polys * 64;
    for (int c = t; c < k_polys * 64; c += 256) {
        dst[c] = p2[c];
        dst[k_polys * 64 + c] = p0[c];
    }
}

// canonical [0, q) -> (-q/2, q/2]
__device__ __forceinline__ int32_t center_canon(int32_t x) { return x - ((((Q / 2) - x) >> 31) & Q); }
__device__ __forceinline__ int32_t iabs(int32_t x) { return x < 0 ? -x : x; }

// Algorithm 7 lines 18-28 for row blockIdx.x, coefficient threadIdx.x of every polynomial.
//   y [rows][L][256] in [-gamma1 + 1, gamma1]; w [rows][K][256] canonical; cs [rows][L + 2 K][256] = c s1 | c s2 | c t0, canonical
//   c_tilde [rows][CT].  Accepted: z_out / h_out / ct_out of the row's op, done = 1.  Rejected: kappa += L.
template <int K, int L, bool G2HI, int CT>
__global__ __launch_bounds__(256) void k_accept(const int32_t* __restrict__ y, const int32_t* __restrict__ w, const int32_t* __restrict__ cs,
                                               const uint8_t* __restrict__ c_tilde, RowState s, int32_t gamma1_beta, int32_t beta,
                                               int32_t omega, int32_t* __restrict__ z_out, int32_t* __restrict__ h_out,
                                               uint8_t* __restrict__ ct_out) {
    constexpr int32_t GAMMA2 = G2HI ? (Q - 1) / 32 : (Q - 1) / 88;
    const size_t row = blockIdx.x;
    if (s.done[row]) return;  // the same for the whole workgroup
    const int t = threadIdx.x;
    int bad = 0;
    int32_t z[L];
#pragma unroll
    for (int j = 0; j < L; j++) {
        z[j] = y[(row * L + j) * 256 + t] + center_canon(cs[(row * (L + 2 * K) + j) * 256 + t]);
        bad |= iabs(z[j]) >= gamma1_beta;
    }
    uint32_t hbits = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int32_t wv = w[(row * K + i) * 256 + t];
        const int32_t c2 = center_canon(cs[(row * (L + 2 * K) + L + i) * 256 + t]);
        const int32_t c0 = center_canon(cs[(row * (L + 2 * K) + L + K + i) * 256 + t]);
        const int32_t r = canon(wv - c2);  // w - c s2
        int32_t r1, r0, v1, v0;
        mldsa::decompose<G2HI>(r, r1, r0);
        bad |= iabs(r0) >= GAMMA2 - beta;
        bad |= iabs(c0) >= GAMMA2;
        mldsa::decompose<G2HI>(canon(r + c0), v1, v0);  // w - c s2 + c t0
        hbits |= (uint32_t)(r1 != v1) << i;             // MakeHint(-c t0, w - c s2 + c t0)
    }
    const int any_bad = __syncthreads_or(bad);
    int weight = 0;
#pragma unroll
    for (int i = 0; i < K; i++) weight += __syncthreads_count((hbits >> i) & 1u);
    if (any_bad || weight > omega) {
        if (t == 0) s.kappa[row] = (uint16_t)(s.kappa[row] + L);
        return;
    }
    const size_t op = s.op[row];
#pragma unroll
    for (int j = 0; j < L; j++) z_out[(op * L + j) * 256 + t] = z[j];
#pragma unroll
    for (int i = 0; i < K; i++) h_out[(op * K + i) * 256 + t] = (int32_t)((hbits >> i) & 1u);
    if (t < CT / 4) reinterpret_cast<uint32_t*>(ct_out + op * CT)[t] = reinterpret_cast<const uint32_t*>(c_tilde + row * CT)[t];
    if (t == 0) s.done[row] = 1;
}

// ------------------------------------------------------------------------------------------------------ sign: compaction
__global__ __launch_bounds__(SCAN_BLOCK) void k_count(const int32_t* __restrict__ done, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t r = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int c = __syncthreads_count(r < n && !done[r]);
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)c;
}

// one wave: counts[b] -> unfinished rows before block b (in place); the total is the live count the host reads
__global__ __launch_bounds__(64) void k_offsets(uint32_t* __restrict__ counts, uint32_t n_blocks, uint32_t* __restrict__ n_live) {
    const int lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 64) {
        const uint32_t b = base + lane;
        const uint32_t v = b < n_blocks ? counts[b] : 0;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(inc, d, 64);
            if (lane >= d) inc += u;
        }
        if (b < n_blocks) counts[b] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) *n_live = carry;
}

// the unfinished rows of `from`, in order, become rows 0 ... n_live - 1 of `to`; src_of[new row] = old row
__global__ __launch_bounds__(SCAN_BLOCK) void k_compact(RowState from, uint32_t n, const uint32_t* __restrict__ offsets, RowState to,
                                                        uint32_t* __restrict__ src_of) {
    __shared__ uint32_t wave_sum[SCAN_BLOCK / 64];
    const uint32_t r = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = r < n && !from.done[r];
    const unsigned long long m = __ballot(live);
    if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t rank = offsets[blockIdx.x] + (uint32_t)__popcll(m & (((unsigned long long)1 << lane) - 1));
    for (int v = 0; v < wave; v++) rank += wave_sum[v];
    if (!live) return;
    const uint4* ms = reinterpret_cast<const uint4*>(from.mu + (size_t)r * 64);
    const uint4* rs = reinterpret_cast<const uint4*>(from.rhopp + (size_t)r * 64);
    uint4* md = reinterpret_cast<uint4*>(to.mu + (size_t)rank * 64);
    uint4* rd = reinterpret_cast<uint4*>(to.rhopp + (size_t)rank * 64);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        md[i] = ms[i];
        rd[i] = rs[i];
    }
    to.kappa[rank] = from.kappa[r];
    to.op[rank] = from.op[r];
    to.key[rank] = from.key[r];
    to.done[rank] = 0;
    src_of[rank] = r;
}

// the signature of a refused op is all zero; one wave per op
__global__ __launch_bounds__(64) void k_zero_refused(uint8_t* __restrict__ sigs, size_t sig_len, const int32_t* __restrict__ bad) {
    if (!bad[blockIdx.x]) return;
    uint8_t* p = sigs + (size_t)blockIdx.x * sig_len;
    for (size_t c = threadIdx.x; c < sig_len; c += 64) p[c] = 0;
}

// ------------------------------------------------------------------------------------------------------------ host side
// Scratch layouts.  Every part is a multiple of 16 bytes per op, so every array starts 16-byte aligned in a 256-byte aligned scratch.
struct VerifyLayout {
    size_t a_hat, t1, h, w, z, c, rho, c_tilde, dec_ok, znorm, bytes;
};

bool verify_layout(int set, size_t n, VerifyLayout* o) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_MU_MAX_OPS) return false;
    const size_t K = (size_t)p.k, L = (size_t)p.l;
    Taker t;
    o->a_hat = t.take(n * 1024 * K * L);
    o->t1 = t.take(n * 1024 * K);
    o->h = t.take(n * 1024 * K);
    o->w = t.take(n * 1024 * K);
    o->z = t.take(n * 1024 * L);
    o->c = t.take(n * 1024);
    o->rho = t.take(n * 32);
    o->c_tilde = t.take(n * 64);
    o->dec_ok = t.take(n * 16);
    o->znorm = t.take(n * 16);  // ||z||inf [n], then the key flags [n]
    o->bytes = t.at;
    return true;
}

struct StateOff {
    size_t mu, rhopp, kappa, op, key, done;
};

struct SignLayout {
    size_t counters, a_hat[2], sec, cs, y, y_hat, z_out, w, h_out, c, ct_out, ct_row, bad, rho_op, src_of, counts, bytes;
    StateOff st[2];
};

void take_state(Taker& t, size_t rows, StateOff* s) {
    s->mu = t.take(rows * 64);
    s->rhopp = t.take(rows * 64);
    s->kappa = t.take(rows * 16);
    s->op = t.take(rows * 16);
    s->key = t.take(rows * 16);
    s->done = t.take(rows * 16);
}

bool sign_layout(int set, size_t n, SignLayout* o) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n > MLDSA_MU_MAX_OPS) return false;
    const size_t K = (size_t)p.k, L = (size_t)p.l, half = (n + 1) / 2;
    Taker t;
    o->counters = t.take(256);
    o->a_hat[0] = t.take(n * 1024 * K * L);
    o->sec = t.take(n * 1024 * (L + 2 * K));
    o->cs = t.take(n * 1024 * (L + 2 * K));
    o->y = t.take(n * 1024 * L);
    o->y_hat = t.take(n * 1024 * L);
    o->z_out = t.take(n * 1024 * L);
    o->w = t.take(n * 1024 * K);
    o->h_out = t.take(n * 1024 * K);
    o->c = t.take(n * 1024);
    o->ct_out = t.take(n * 64);
    o->ct_row = t.take(n * 64);
    o->bad = t.take(n * 16);
    o->rho_op = t.take(n * 32);
    o->src_of = t.take(n * 16);
    o->counts = t.take(n * 16);
    take_state(t, n, &o->st[0]);
    o->a_hat[1] = t.take(half * 1024 * K * L);
    take_state(t, half, &o->st[1]);
    o->bytes = t.at;
    return true;
}

RowState row_state(uint8_t* base, const StateOff& s) {
    RowState r;
    r.mu = base + s.mu;
    r.rhopp = base + s.rhopp;
    r.kappa = reinterpret_cast<uint16_t*>(base + s.kappa);
    r.op = reinterpret_cast<uint32_t*>(base + s.op);
    r.key = reinterpret_cast<uint32_t*>(base + s.key);
    r.done = reinterpret_cast<int32_t*>(base + s.done);
    return r;
}

size_t verify_bytes(int set, size_t n) {
    VerifyLayout L;
    return verify_layout(set, n, &L) ? L.bytes : 0;
}

size_t sign_bytes(int set, size_t n) {
    SignLayout L;
    return sign_layout(set, n, &L) ? L.bytes : 0;
}

template <bool VERIFY>
void launch_commit(int set, const int32_t* w, const int32_t* h, const uint8_t* mu, size_t n, uint8_t* c_tilde, const CommitVerify& vd,
                   hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (set == MLDSA_44) hipLaunchKernelGGL((k_commit<4, false, 32, VERIFY>), grid, block, 0, s, w, h, mu, n, c_tilde, vd);
    else if (set == MLDSA_65) hipLaunchKernelGGL((k_commit<6, true, 48, VERIFY>), grid, block, 0, s, w, h, mu, n, c_tilde, vd);
    else hipLaunchKernelGGL((k_commit<8, true, 64, VERIFY>), grid, block, 0, s, w, h, mu, n, c_tilde, vd);
}

int verify_pass(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const uint8_t* rho, const int32_t* t1, size_t n_keys,
                const uint32_t* key_idx, const uint8_t* mu, const int32_t* mu_flag, const uint8_t* sigs, uint8_t* ok, size_t op0, size_t n,
                uint8_t* base, hipStream_t s) {
    VerifyLayout V;
    verify_layout(set, n, &V);
    int32_t* a_hat = reinterpret_cast<int32_t*>(base + V.a_hat);
    int32_t* t1_op = reinterpret_cast<int32_t*>(base + V.t1);
    int32_t* h = reinterpret_cast<int32_t*>(base + V.h);
    int32_t* w = reinterpret_cast<int32_t*>(base + V.w);
    int32_t* z = reinterpret_cast<int32_t*>(base + V.z);
    int32_t* c = reinterpret_cast<int32_t*>(base + V.c);
    uint8_t* rho_op = base + V.rho;
    uint8_t* c_tilde = base + V.c_tilde;
    uint8_t* dec_ok = base + V.dec_ok;
    int32_t* znorm = reinterpret_cast<int32_t*>(base + V.znorm);
    int32_t* key_bad = znorm + n;
    const uint8_t* pass_sigs = sigs + op0 * (size_t)p.sig_len;
    void* st = (void*)s;

    hipLaunchKernelGGL(k_gather_pk, dim3((unsigned)n), dim3(256), 0, s, rho, t1, (uint32_t)n_keys, key_idx, op0, p.k, rho_op, t1_op, key_bad);
    LAYER_LAUNCHED("k_gather_pk launch");
    LAYER_CORE(mldsa_sig_decode(ctx, set, pass_sigs, c_tilde, z, h, dec_ok, n, st), "mldsa_sig_decode");
    LAYER_CORE(mldsa_sample_in_ball(ctx, set, c_tilde, c, n, st), "mldsa_sample_in_ball");
    LAYER_CORE(mldsa_expand_a(ctx, set, rho_op, a_hat, n, st), "mldsa_expand_a");
    LAYER_CORE(mldsa_verify_arith(ctx, set, a_hat, z, c, t1_op, w, n, st), "mldsa_verify_arith");
    LAYER_CORE(mldsa_infinity_norm(ctx, z, (size_t)p.l, n, znorm, st), "mldsa_infinity_norm");
    CommitVerify vd;
    vd.sigs = pass_sigs;
    vd.sig_len = (size_t)p.sig_len;
    vd.dec_ok = dec_ok;
    vd.znorm = znorm;
    vd.zbound = p.gamma1 - p.beta;
    vd.mu_flag = mu_flag ? mu_flag + op0 : nullptr;
    vd.key_bad = key_bad;
    vd.ok = ok + op0;
    launch_commit<true>(set, w, h, mu + op0 * MLDSA_MU_LEN, n, nullptr, vd, s);
    LAYER_LAUNCHED("k_commit launch");
    return MLDSA_OK;
}

void launch_accept(int set, const int32_t* y, const int32_t* w, const int32_t* cs, const uint8_t* ct_row, const RowState& rs,
                   const mldsa_params& p, int32_t* z_out, int32_t* h_out, uint8_t* ct_out, uint32_t rows, hipStream_t s) {
    const dim3 grid(rows), block(256);
    const int32_t gb = p.gamma1 - p.beta;
    if (set == MLDSA_44)
        hipLaunchKernelGGL((k_accept<4, 4, false, 32>), grid, block, 0, s, y, w, cs, ct_row, rs, gb, p.beta, p.omega, z_out, h_out, ct_out);
    else if (set == MLDSA_65)
        hipLaunchKernelGGL((k_accept<6, 5, true, 48>), grid, block, 0, s, y, w, cs, ct_row, rs, gb, p.beta, p.omega, z_out, h_out, ct_out);
    else
        hipLaunchKernelGGL((k_accept<8, 7, true, 64>), grid, block, 0, s, y, w, cs, ct_row, rs, gb, p.beta, p.omega, z_out, h_out, ct_out);
}

struct SignKeys {
    const uint8_t *rho, *cap_k;
    const int32_t *s1, *s2, *t0;
    size_t n_keys;
    const uint32_t* key_idx;
};

int sign_pass(const char* fn, mldsa_ctx* ctx, int set, const mldsa_params& p, const SignKeys& k, const uint8_t* mu, const int32_t* mu_flag,
              const uint8_t* rnd, uint8_t* sigs, int32_t* status, size_t op0, size_t n, uint8_t* base, hipStream_t s) {
    SignLayout S;
    sign_layout(set, n, &S);
    const size_t K = (size_t)p.k, L = (size_t)p.l;
    uint32_t* d_live = reinterpret_cast<uint32_t*>(base + S.counters);
    int32_t* a_hat[2] = {reinterpret_cast<int32_t*>(base + S.a_hat[0]), reinterpret_cast<int32_t*>(base + S.a_hat[1])};
    int32_t* sec = reinterpret_cast<int32_t*>(base + S.sec);
    int32_t* cs = reinterpret_cast<int32_t*>(base + S.cs);
    int32_t* y = reinterpret_cast<int32_t*>(base + S.y);
    int32_t* y_hat = reinterpret_cast<int32_t*>(base + S.y_hat);
    int32_t* z_out = reinterpret_cast<int32_t*>(base + S.z_out);
    int32_t* w = reinterpret_cast<int32_t*>(base + S.w);
    int32_t* h_out = reinterpret_cast<int32_t*>(base + S.h_out);
    int32_t* c = reinterpret_cast<int32_t*>(base + S.c);
    uint8_t* ct_out = base + S.ct_out;
    uint8_t* ct_row = base + S.ct_row;
    int32_t* bad = reinterpret_cast<int32_t*>(base + S.bad);
    uint8_t* rho_op = base + S.rho_op;
    uint32_t* src_of = reinterpret_cast<uint32_t*>(base + S.src_of);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base + S.counts);
    RowState rs[2] = {row_state(base, S.st[0]), row_state(base, S.st[1])};
    void* st = (void*)s;

    // what mldsa_sig_encode reads for every op of the pass, refused ones included
    hipError_t e = hipMemsetAsync(z_out, 0, n * 1024 * L, s);
    if (e == hipSuccess) e = hipMemsetAsync(h_out, 0, n * 1024 * K, s);
    if (e == hipSuccess) e = hipMemsetAsync(ct_out, 0, n * 64, s);
    if (e != hipSuccess) return hip_failed(fn, "clearing the outputs of the pass", e);
    uint32_t rows = (uint32_t)n;
    int cur = 0;
    hipLaunchKernelGGL(k_sign_init, dim3((rows + 255) / 256), dim3(256), 0, s, k.rho, (uint32_t)k.n_keys, k.key_idx, mu, mu_flag, op0, rows,
                       rs[0], rho_op, bad, status);
    hipLaunchKernelGGL(k_rhopp, dim3((rows + 63) / 64), dim3(64), 0, s, k.cap_k, rnd + op0 * 32, rs[0], rows);
    hipLaunchKernelGGL(k_gather_rows, dim3(rows), dim3(256), 0, s, (const int32_t*)nullptr, (int32_t*)nullptr, (const uint32_t*)nullptr,
                       rs[0].key, k.s1, k.s2, k.t0, sec, p.k, p.l);
    LAYER_LAUNCHED("prologue launch");
    LAYER_CORE(mldsa_expand_a(ctx, set, rho_op, a_hat[0], n, st), "mldsa_expand_a");

    const CommitVerify none = {};
    for (;;) {
        const uint32_t n_blocks = (rows + SCAN_BLOCK - 1) / SCAN_BLOCK;
        LAYER_CORE(mldsa_expand_mask(ctx, set, rs[cur].rhopp, rs[cur].kappa, y, rows, st), "mldsa_expand_mask");
        LAYER_CORE(mldsa_ntt(ctx, y, y_hat, rows * L, st), "mldsa_ntt");
        LAYER_CORE(mldsa_mat_vec_mul(ctx, set, a_hat[cur], y_hat, w, rows, st), "mldsa_mat_vec_mul");
        LAYER_CORE(mldsa_inv_ntt(ctx, w, w, rows * K, st), "mldsa_inv_ntt");
        launch_commit<false>(set, w, nullptr, rs[cur].mu, rows, ct_row, none, s);
        LAYER_LAUNCHED("k_commit launch");
        LAYER_CORE(mldsa_sample_in_ball(ctx, set, ct_row, c, rows, st), "mldsa_sample_in_ball");
        LAYER_CORE(mldsa_ntt(ctx, c, c, rows, st), "mldsa_ntt");
        LAYER_CORE(mldsa_pointwise_mont(ctx, c, sec, cs, L + 2 * K, rows, st), "mldsa_pointwise_mont");
        LAYER_CORE(mldsa_inv_ntt(ctx, cs, cs, rows * (L + 2 * K), st), "mldsa_inv_ntt");
        launch_accept(set, y, w, cs, ct_row, rs[cur], p, z_out, h_out, ct_out, rows, s);
        hipLaunchKernelGGL(k_count, dim3(n_blocks), dim3(SCAN_BLOCK), 0, s, rs[cur].done, rows, counts);
        hipLaunchKernelGGL(k_offsets, dim3(1), dim3(64), 0, s, counts, n_blocks, d_live);
        LAYER_LAUNCHED("round launch");
        uint32_t live = 0;  // the round's one look at the device
        e = hipMemcpyAsync(&live, d_live, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_failed(fn, "reading the live count", e);
        if (live == 0) break;
        if (live <= rows / 2) {
            const int nxt = cur ^ 1;
            hipLaunchKernelGGL(k_compact, dim3(n_blocks), dim3(SCAN_BLOCK), 0, s, rs[cur], rows, counts, rs[nxt], src_of);
            hipLaunchKernelGGL(k_gather_rows, dim3(live), dim3(256), 0, s, a_hat[cur], a_hat[nxt], src_of, rs[nxt].key, k.s1, k.s2, k.t0, sec,
                               p.k, p.l);
            LAYER_LAUNCHED("compaction launch");
            cur = nxt;
            rows = live;
        }
    }
    uint8_t* pass_sigs = sigs + op0 * (size_t)p.sig_len;
    LAYER_CORE(mldsa_sig_encode(ctx, set, ct_out, z_out, h_out, pass_sigs, nullptr, n, st), "mldsa_sig_encode");
    hipLaunchKernelGGL(k_zero_refused, dim3((unsigned)n), dim3(64), 0, s, pass_sigs, (size_t)p.sig_len, bad);
    LAYER_LAUNCHED("k_zero_refused launch");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_mu_abi_version(void) { return MLDSA_MU_ABI_VERSION; }

const char* mldsa_mu_last_error(void) { return g_err.c_str(); }

size_t mldsa_mu_verify_scratch_bytes(int set, size_t n_ops) { return verify_bytes(set, n_ops); }

size_t mldsa_mu_sign_scratch_bytes(int set, size_t n_ops) { return sign_bytes(set, n_ops); }

int mldsa_mu_compute(mldsa_ctx* ctx, int mode, const uint8_t* tr, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                     const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, uint8_t* mu, int32_t* mu_flag, size_t n_ops,
                     void* stream) {
    const char* fn = "mldsa_mu_compute";
    if (mode != MLDSA_MODE_PURE && mode != MLDSA_MODE_INTERNAL && mode != MLDSA_MODE_PREHASH)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!tr || !msg_off || !mu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (n_keys == 0 || n_keys > 0xFFFFFFFFu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0 or does not fit 32 bits");
    if (n_ops > MLDSA_MU_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_MU_MAX_OPS ops");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mu_ext, dim3((unsigned)((n_ops + 63) / 64)), dim3(64), 0, s, tr, (uint32_t)n_keys, key_idx, mode, msgs, msg_off, ctxs,
                       ctx_off, mu, mu_flag, n_ops);
    LAYER_LAUNCHED("k_mu_ext launch");
    return MLDSA_OK;
}

int mldsa_verify_mu(mldsa_ctx* ctx, int set, const uint8_t* rho, const int32_t* t1_d2_hat_mont, size_t n_keys, const uint32_t* key_idx,
                    const uint8_t* mu, const int32_t* mu_flag, const uint8_t* sigs, uint8_t* ok, size_t n_ops, void* scratch,
                    size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_verify_mu";
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!rho || !t1_d2_hat_mont || !mu || !sigs || !ok) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (n_keys == 0 || n_keys > 0xFFFFFFFFu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0 or does not fit 32 bits");
    if (n_ops > MLDSA_MU_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_MU_MAX_OPS ops");
    if (!aligned(t1_d2_hat_mont, 16)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": t1_d2_hat_mont must be 16-byte aligned");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    const size_t pass = largest_pass(n_ops, scratch_bytes, [set](size_t n) { return verify_bytes(set, n); });
    if (pass == 0) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_mu_verify_scratch_bytes(set, min(n_ops, 64))");
    LAYER_ON_DEVICE(ctx);
    for (size_t op0 = 0; op0 < n_ops; op0 += pass) {
        const size_t n = n_ops - op0 < pass ? n_ops - op0 : pass;
        const int rc = verify_pass(fn, ctx, set, p, rho, t1_d2_hat_mont, n_keys, key_idx, mu, mu_flag, sigs, ok, op0, n,
                                   static_cast<uint8_t*>(scratch), (hipStream_t)stream);
        if (rc != MLDSA_OK) return rc;
    }
    return MLDSA_OK;
}

int mldsa_sign_mu(mldsa_ctx* ctx, int set, const uint8_t* rho, const uint8_t* cap_k, const int32_t* s_1_hat_mont, const int32_t* s_2_hat_mont,
                  const int32_t* t_0_hat_mont, size_t n_keys, const uint32_t* key_idx, const uint8_t* mu, const int32_t* mu_flag,
                  const uint8_t* rnd, uint8_t* sigs, int32_t* status, size_t n_ops, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_sign_mu";
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!rho || !cap_k || !s_1_hat_mont || !s_2_hat_mont || !t_0_hat_mont || !mu || !rnd || !sigs)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (n_keys == 0 || n_keys > 0xFFFFFFFFu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0 or does not fit 32 bits");
    if (n_ops > MLDSA_MU_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_MU_MAX_OPS ops");
    if (!aligned(s_1_hat_mont, 16) || !aligned(s_2_hat_mont, 16) || !aligned(t_0_hat_mont, 16))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": the key polynomials must be 16-byte aligned");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    const size_t pass = largest_pass(n_ops, scratch_bytes, [set](size_t n) { return sign_bytes(set, n); });
    if (pass == 0) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_mu_sign_scratch_bytes(set, min(n_ops, 64))");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const SignKeys keys = {rho, cap_k, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont, n_keys, key_idx};
    int rc = MLDSA_OK;
    for (size_t op0 = 0; op0 < n_ops && rc == MLDSA_OK; op0 += pass) {
        const size_t n = n_ops - op0 < pass ? n_ops - op0 : pass;
        rc = sign_pass(fn, ctx, set, p, keys, mu, mu_flag, rnd, sigs, status, op0, n, static_cast<uint8_t*>(scratch), s);
    }
    // the scratch held rho'', y, c s1 ... and copies of K's users s1, s2, t0: cleared whatever happened above (written out, not the
    // scaffold's cleared(): this call reports a failed clearing with the HIP runtime's message, not with the core's)
    hipError_t e = hipMemsetAsync(scratch, 0, scratch_bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (rc != MLDSA_OK) return rc;
    return e == hipSuccess ? MLDSA_OK : hip_failed(fn, "clearing the scratch", e);
}

}  // extern "C"
