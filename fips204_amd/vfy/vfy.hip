// libmldsa_vfy.so (include/mldsa_vfy.h): the large-batch, device-resident verify pass of the core's verify_batch (../csrc/pipeline.hip),
// layered on the core's C ABI and rebuilt around three levers:
//   - ExpandA on the folded Keccak round of keccak180.h (180 VALU per round instead of 190): the kernel is bound by its own instruction
//     count, so fewer instructions are the only thing that moves it;
//   - parts: the call is cut into parts (vfy_parts.h).  A call of one part -- every call up to MLDSA_VFY_PART_OPS ops -- is one chain on
//     the caller's stream: ExpandA, k_verify_main, the c~ hash, with the front (key-index check, mu, SampleInBall) on one library-owned
//     stream beside ExpandA and no hand-over between queues on the way.  In a call of several parts ExpandA of part p + 1 runs on one
//     library-owned stream while k_verify_main and the c~ hash of part p run on the other, and the front of every part on the caller's
//     stream underneath.  The order of either shape is data (order_plan() in vfy_parts.h), enqueue() below walks it; only stream
//     events order the work.  The A_hat scratch is a ring of two parts.
//   - k_verify_main's VALU stream: two rows a trip on two register sets, hint bits read from LDS, quad exchanges without a zeroed
//     destination, w1Encode with one gather ("wave helpers of verify_main" below): the kernel is bound by instruction issue as well.
// The device building blocks are the core's, included read-only (field.h, keccak.h, sampler_dev.h, ntt_wave.h, rounding.h, verify_dev.h,
// challenge_dev.h); the kernels below are the core's kernels of the same names on those blocks, cut down to what this pass uses (packed
// A_hat by op, c in bytes, lane-per-op hashes: the pass serves large calls only).  Formats and verdicts are the core's.
// This pass folds back into ../csrc when the core's profile set is next collected.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/mldsa_vfy.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"
#include "../csrc/challenge_dev.h"
#include "../csrc/ntt_wave.h"
#include "../csrc/sampler_dev.h"
#include "../csrc/tables.h"
#include "../csrc/verify_dev.h"
#include "keccak180.h"
#include "vfy_parts.h"

namespace mldsa_vfy {

using mldsa::FWD_TW;
using mldsa::INV_TW;
using mldsa::N;
using mldsa::SHAKE256_RATE;
using mldsa::SWAVES;
using mldsa::Twiddle;
using mldsa::load_le32;
using mldsa::static_for;

// ------------------------------------------------------------------------------------------------------------------ ExpandA
// stream (op, r, s): SHAKE128(rho | s | r) -> RejNTTPoly into the packed row of A_hat[op][r][s].  The core's k_expand_a<K, L, true> on
// the folded round.  FIVE waves per SIMD where the core has four (95 VGPRs: five fit without a spill, six spill and lose 2 %): every
// wave runs the same five permutations, so the grid drains in rounds, and the 30 720 waves of a 65 536-op ML-DSA-65 call are 7.5 rounds
// of 4 096 but 6.0 of 5 120.  Measured per set and size against four waves, builds alternated (profiles/vfy_layer_ab.jsonl, kind
// min_ops): level for ML-DSA-65, ahead for ML-DSA-87, and for ML-DSA-44 the difference between a pass that separates from the core and
// one that does not.  What five waves give up is the core's reason for four: they leave a SIMD 32 VGPRs, so the front's waves no longer
// run UNDERNEATH ExpandA but in the slots its waves free as they finish (enqueue() below has the numbers).  The cap is what keeps the
// kernel free of spills.
#ifndef MLDSA_VFY_EA_WAVES
#define MLDSA_VFY_EA_WAVES 5
#endif
template <int K, int L>
__global__ __launch_bounds__(64 * SWAVES) __attribute__((amdgpu_waves_per_eu(MLDSA_VFY_EA_WAVES, MLDSA_VFY_EA_WAVES))) void k_expand_a(const uint8_t* __restrict__ rho, size_t rho_stride,
                                                                                                    const uint32_t* __restrict__ key_idx,
                                                                                                    int32_t* __restrict__ a_hat, size_t n_ops,
                                                                                                    uint32_t n_keys) {
    const int lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * (64 * SWAVES) + threadIdx.x;
    const size_t wave_base = g - lane;
    const size_t n_streams = n_ops * (size_t)(K * L);
    const bool valid = g < n_streams;
    const size_t op = valid ? g / (K * L) : 0;
    const int rs = valid ? (int)(g % (K * L)) : 0;
    const int r = rs / L, sidx = rs % L;
    KeccakState st;
    // n_keys != 0: key_idx is the caller's, unchecked (k_sanitize_keys checks it beside this kernel): an index outside the table reads
    // key 0 here, its op is refused there
    size_t key = key_idx ? key_idx[op] : op;
    if (n_keys && key >= n_keys) key = 0;
    mldsa::expand_a_seed(st, rho + key * rho_stride, sidx, r);
    rej_ntt_poly_lane_direct180(st, a_hat, wave_base, lane, valid);
}

// the seam's unpack: packed rows -> int32[256] in coefficient order (lane's dwords 3 lane .. 3 lane + 2 hold coefficients 4 lane .. 4 lane + 3)
__global__ __launch_bounds__(256) void k_unpack_a(const uint32_t* __restrict__ packed, int32_t* __restrict__ out, size_t n_polys) {
    const size_t poly = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (poly >= n_polys) return;
    const int lane = threadIdx.x & 63;
    const uint32_t* p = packed + poly * mldsa::PACKED_POLY_DWORDS + 3 * lane;
    reinterpret_cast<int4*>(out + poly * N)[lane] = mldsa::unpack24(mldsa::Packed3{p[0], p[1], p[2]});
}

// -------------------------------------------------------------------------------------------------------------------- front
// safe[op] = key_idx[op] if it is below n_keys, else 0; bad[op] = 2 for the ops that were outside
__global__ __launch_bounds__(256) void k_sanitize_keys(const uint32_t* __restrict__ key_idx, uint32_t n_keys, size_t n_ops,
                                                       uint32_t* __restrict__ safe, int32_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ops) return;
    const uint32_t k = key_idx[i];
    safe[i] = k < n_keys ? k : 0u;
    bad[i] = k < n_keys ? 0 : 2;
}

// mu = H(tr | M', 64), one op per lane: the core's k_mu with its checks, flags and bytes.  msg_off / ctx_off are the CALL's tables
// (n_call + 1 entries); the launch covers ops [op0, op0 + n_ops) of it and the per-op arrays are the launch's own (index op - op0).
constexpr int MU_BLK_STRIDE = 35;  // dwords per lane row (136 bytes + pad, odd stride)
__global__ __launch_bounds__(64) void k_mu(const uint8_t* __restrict__ tr, size_t tr_stride, const uint32_t* __restrict__ key_idx, int mode,
                                           const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ msg_off,
                                           const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off, uint8_t* __restrict__ mu,
                                           size_t mu_stride, int32_t* __restrict__ ctx_bad, const int32_t* __restrict__ key_bad, size_t n_ops,
                                           size_t op0, size_t n_call) {
    __shared__ uint32_t blk[64 * MU_BLK_STRIDE];
    const int lane = threadIdx.x;
    const size_t op = (size_t)blockIdx.x * 64 + lane;
    const bool valid = op < n_ops;
    uint32_t* row = blk + lane * MU_BLK_STRIDE;
    uint8_t* rowb = reinterpret_cast<uint8_t*>(row);

    const uint8_t *trp = nullptr, *mp = nullptr, *cp = nullptr;
    size_t mlen = 0, clen = 0;
    bool live = false;  // the op is hashed
    if (valid) {
        trp = tr + (key_idx ? key_idx[op] : op) * tr_stride;
        const uint64_t m0 = msg_off[op0 + op], m1 = msg_off[op0 + op + 1];
        bool bad_off = !(msg_off[0] <= m0 && m0 <= m1 && m1 <= msg_off[n_call]);
        mp = msgs + m0;
        mlen = (size_t)(m1 - m0);
        bad_off |= mlen != 0 && msgs == nullptr;  // offsets that name bytes of a NULL array
        if (ctx_off) {
            const uint64_t c0 = ctx_off[op0 + op], c1 = ctx_off[op0 + op + 1];
            bad_off |= !(ctx_off[0] <= c0 && c0 <= c1 && c1 <= ctx_off[n_call]);
            cp = ctxs + c0;
            clen = (size_t)(c1 - c0);
            bad_off |= clen != 0 && ctxs == nullptr;
        }
        // 2: malformed offsets or key index out of range; 1: ctx too long
        const int flag = bad_off ? 2 : clen > 255 ? 1 : (key_bad ? key_bad[op] : 0);
        ctx_bad[op] = flag;
        live = !bad_off && clen <= 255;
        if (!live) mlen = clen = 0;
    }
    const size_t pre = (mode == MLDSA_MODE_INTERNAL) ? 0 : 2 + clen;
    const size_t total = live ? 64 + pre + mlen : 0;
    const size_t my_blocks = live ? total / SHAKE256_RATE + 1 : 0;  // the pad always fits in the last block
    size_t max_blocks = my_blocks;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const size_t o = (size_t)__shfl_xor((unsigned long long)max_blocks, m);
        max_blocks = o > max_blocks ? o : max_blocks;
    }
    KeccakState st;
    mldsa::keccak_zero(st);
    for (size_t b = 0; b < max_blocks; b++) {
        if (b < my_blocks) {
            const size_t base = b * SHAKE256_RATE;
            auto byte_at = [&](size_t pos) -> uint8_t {
                if (pos < total) {
                    if (pos < 64) return trp[pos];
                    if (pos < 64 + pre) {
                        const size_t q = pos - 64;
                        return q == 0 ? (uint8_t)(mode == MLDSA_MODE_PREHASH ? 1 : 0) : q == 1 ? (uint8_t)clen : cp[q - 2];
                    }
                    return mp[pos - 64 - pre];
                }
                return pos == total ? (uint8_t)0x1F : (uint8_t)0;
            };
            // whole dwords of tr and of the message by one byte-granular load each; the dwords that straddle a boundary from bytes
            for (int i = 0; i < SHAKE256_RATE / 4; i++) {
                const size_t pos = base + 4 * (size_t)i;
                uint32_t v;
                if (pos + 4 <= 64) v = load_le32(trp + pos);
                else if (pos >= 64 + pre && pos + 4 <= total) v = load_le32(mp + (pos - 64 - pre));
                else if (pos > total) v = 0;
                else v = (uint32_t)byte_at(pos) | ((uint32_t)byte_at(pos + 1) << 8) | ((uint32_t)byte_at(pos + 2) << 16) | ((uint32_t)byte_at(pos + 3) << 24);
                row[i] = v;
            }
            if (b == my_blocks - 1) rowb[SHAKE256_RATE - 1] |= 0x80;
            static_for<0, 17>([&](auto wc) {
                constexpr int W = decltype(wc)::value;
                st.lo[W] ^= row[2 * W];
                st.hi[W] ^= row[2 * W + 1];
            });
            mldsa::keccak_f1600(st);
        }
    }
    if (valid) {
        uint32_t* out = reinterpret_cast<uint32_t*>(mu + op * mu_stride);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            out[2 * i] = st.lo[i];
            out[2 * i + 1] = st.hi[i];
        }
    }
}

// c = SampleInBall(c_tilde), one op per lane, as 256 bytes per op: the four coefficients 64 k + lane in lane's dword (the core's
// k_sample_in_ball<CT, true>)
template <int CT>
__global__ __launch_bounds__(64) void k_sample_in_ball(const uint8_t* __restrict__ c_tilde, size_t ct_stride, int tau, uint32_t* __restrict__ c_out,
                                                       size_t n_ops) {
    __shared__ uint32_t c_lds[64 * mldsa::SIB_C_STRIDE];
    __shared__ uint32_t b_lds[64 * mldsa::SIB_BLK_STRIDE];
    const int lane = threadIdx.x;
    const size_t wave_base = (size_t)blockIdx.x * 64;
    const size_t op = wave_base + lane;
    const bool valid = op < n_ops;
    KeccakState st;
    mldsa::keccak_zero(st);
    if (valid) mldsa::absorb_words<CT / 8>(st, c_tilde + op * ct_stride);
    mldsa::shake_pad<SHAKE256_RATE, CT>(st);
    mldsa::sample_in_ball_lane(st, tau, valid, c_lds + lane * mldsa::SIB_C_STRIDE, b_lds + lane * mldsa::SIB_BLK_STRIDE);
    mldsa::wave_lds_sync();
    for (int row = 0; row < 64; row++) {
        if (wave_base + row >= n_ops) break;
        const uint8_t* cb = reinterpret_cast<const uint8_t*>(c_lds + row * mldsa::SIB_C_STRIDE);
        c_out[(wave_base + row) * 64 + lane] =
            (uint32_t)cb[lane] | ((uint32_t)cb[64 + lane] << 8) | ((uint32_t)cb[128 + lane] << 16) | ((uint32_t)cb[192 + lane] << 24);
    }
}

// ------------------------------------------------------------------------------------------------- wave helpers of verify_main
// k_verify_main is bound by instruction issue, so these are ../csrc/ntt_wave.h's transforms and ../csrc/rounding.h's w1Encode with the
// same data movement in fewer VALU slots.  The core's quad exchanges are v_mov_b32_dpp with old = 0 and bound_ctrl off: the compiler has
// to zero the destination first (one v_mov per exchange).  A quad permutation gives every lane a source, so `old` is never read: with
// bound_ctrl on the zeroing goes, and where the consumer is a VOP2 (the v_or of w1Encode) the exchange folds into it.
template <int CTRL>
__device__ __forceinline__ int32_t dpp_all(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// mldsa::swap_pair: the upper lane's x <-> the lower lane's y (lanes l, l ^ M)
template <int M>
__device__ __forceinline__ void swap_pair(int32_t& x, int32_t& y, int lane) {
    if constexpr (M >= 4) {
        mldsa::swap_pair<M>(x, y, lane);  // permlane swaps, and row DPP whose `old` is the value kept: nothing to zero
    } else {
        constexpr int CTRL = M == 2 ? 0x4E : 0xB1;  // quad_perm:[2,3,0,1] | [1,0,3,2]
        const int32_t px = dpp_all<CTRL>(x), py = dpp_all<CTRL>(y);
        const bool up = (lane & M) != 0;
        x = up ? py : x;
        y = up ? y : px;
    }
}
template <int M>
__device__ __forceinline__ void xchg_hi(int32_t r[4], int lane) {
    swap_pair<M>(r[0], r[2], lane);
    swap_pair<M>(r[1], r[3], lane);
}
template <int M>
__device__ __forceinline__ void xchg_lo(int32_t r[4], int lane) {
    swap_pair<M>(r[0], r[1], lane);
    swap_pair<M>(r[2], r[3], lane);
}

// mldsa::ntt_fwd_wave / ntt_inv_wave on the exchanges above: the same butterflies in the same order, the same twiddle tables
template <class TW>
__device__ __forceinline__ void ntt_fwd_wave(int32_t r[4], const TW& tw, int lane) {
    using mldsa::bf_ct;
    bf_ct(r[0], r[2], mldsa::ZF1);
    bf_ct(r[1], r[3], mldsa::ZF1);
    bf_ct(r[0], r[1], mldsa::ZF2);
    bf_ct(r[2], r[3], mldsa::ZF3);
    xchg_hi<32>(r, lane);
    bf_ct(r[0], r[2], tw.get(0));
    bf_ct(r[1], r[3], tw.get(1));
    xchg_lo<16>(r, lane);
    bf_ct(r[0], r[1], tw.get(2));
    bf_ct(r[2], r[3], tw.get(3));
    xchg_hi<8>(r, lane);
    bf_ct(r[0], r[2], tw.get(4));
    bf_ct(r[1], r[3], tw.get(5));
    xchg_lo<4>(r, lane);
    bf_ct(r[0], r[1], tw.get(6));
    bf_ct(r[2], r[3], tw.get(7));
    xchg_hi<2>(r, lane);
    bf_ct(r[0], r[2], tw.get(8));
    bf_ct(r[1], r[3], tw.get(9));
    xchg_lo<1>(r, lane);
    bf_ct(r[0], r[1], tw.get(10));
    bf_ct(r[2], r[3], tw.get(11));
}
template <class TW>
__device__ __forceinline__ void ntt_inv_wave(int32_t r[4], const TW& tw, int lane, int32_t f) {
    using mldsa::bf_gs;
    bf_gs(r[0], r[1], tw.get(0));
    bf_gs(r[2], r[3], tw.get(1));
    bf_gs(r[0], r[2], tw.get(2));
    bf_gs(r[1], r[3], tw.get(3));
    xchg_lo<1>(r, lane);
    bf_gs(r[0], r[1], tw.get(4));
    bf_gs(r[2], r[3], tw.get(5));
    xchg_hi<2>(r, lane);
    bf_gs(r[0], r[2], tw.get(6));
    bf_gs(r[1], r[3], tw.get(7));
    xchg_lo<4>(r, lane);
    bf_gs(r[0], r[1], tw.get(8));
    bf_gs(r[2], r[3], tw.get(9));
    xchg_hi<8>(r, lane);
    bf_gs(r[0], r[2], tw.get(10));
    bf_gs(r[1], r[3], tw.get(11));
    xchg_lo<16>(r, lane);
    bf_gs(r[0], r[1], tw.get(12));
    bf_gs(r[2], r[3], tw.get(13));
    xchg_hi<32>(r, lane);
    const int32_t zf = (int32_t)((((int64_t)mldsa::ZI1 * f) % mldsa::Q) * mldsa::RINV_MOD_Q % mldsa::Q);  // ZI1 * f * 2^-32 mod q
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int32_t a = r[k], b = r[k + 2];
        r[k] = mldsa::caddq(mldsa::mont_mul(a + b, f));
        r[k + 2] = mldsa::caddq(mldsa::mont_mul(a - b, zf));
    }
}

// mldsa::pack_w1_strided: v[k] = the field of coefficient 64 k + lane, the same bytes at dst.
template <bool G2HI>
__device__ __forceinline__ void pack_w1_strided(const uint32_t v[4], uint8_t* dst, int lane) {
    if constexpr (G2HI) {
        // 8 adjacent lanes make one dword of register k (8 nibbles).  OR over the quad for all four registers; then lane 8 m + k
        // (k < 4) picks ITS register's quad sum and takes the other quad's from lane + 4, which picked the same register: one
        // exchange where the core mirrors all four registers across the half row and selects afterwards (by branches, as compiled).
        uint32_t d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = v[k] << (4 * (lane & 7));
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] |= (uint32_t)dpp_all<0xB1>((int32_t)d[k]);  // quad_perm:[1,0,3,2]
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] |= (uint32_t)dpp_all<0x4E>((int32_t)d[k]);  // quad_perm:[2,3,0,1]
        const uint32_t d01 = (lane & 1) ? d[1] : d[0], d23 = (lane & 1) ? d[3] : d[2];
        uint32_t mine = (lane & 2) ? d23 : d01;
        mine |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)mine, 0x104, 0xF, 0xF, true);  // row_shl:4: lane i reads lane i + 4
        if (!(lane & 4)) mldsa::store_row(reinterpret_cast<uint32_t*>(dst) + 8 * (lane & 3) + (lane >> 3), mine);
    } else {
        // coefficient quads sit in adjacent lanes: 4 x 6 bits = 3 bytes, assembled with DPP quad permutes
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t n1 = (uint32_t)dpp_all<0xB1>((int32_t)v[k]);      // lane ^ 1
            const uint32_t pair = (lane & 1) ? 0u : (v[k] | (n1 << 6));      // 12 bits in even lanes
            const uint32_t n2 = (uint32_t)dpp_all<0x4E>((int32_t)pair);      // lane ^ 2
            if (!(lane & 3)) {
                const uint32_t q24 = pair | (n2 << 12);
                uint8_t* d = dst + 48 * k + 3 * (lane >> 2);
                d[0] = (uint8_t)q24; d[1] = (uint8_t)(q24 >> 8); d[2] = (uint8_t)(q24 >> 16);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- verify_main
// The core's k_verify_main<.., APACK = true> with A_hat by op: one wave per op, sigDecode, NTT(z), NTT(c), the K rows of
// A_hat o z_hat - c_hat o t1_hat -> inverse NTT -> UseHint -> w1Encode, the next A_hat row in flight under the current row's inverse NTT.
constexpr int VW = 4;  // waves (= ops in flight) per block
template <int K, int L, int GB, bool G2HI, int MINW>
__global__ __launch_bounds__(64 * VW) __attribute__((amdgpu_waves_per_eu(MINW))) void k_verify_main(
    const uint32_t* __restrict__ a_hat, const uint8_t* __restrict__ sigs, size_t sig_len, int ctilde_len, const uint32_t* __restrict__ c,
    const int32_t* __restrict__ t1, const uint32_t* __restrict__ key_idx, size_t key_base, int32_t* __restrict__ hvalid, int omega,
    uint8_t* __restrict__ w1, size_t w1_stride, int32_t* __restrict__ znorm, int32_t zbound, size_t n_ops, const Twiddle* __restrict__ fwd_tab,
    const Twiddle* __restrict__ inv_tab) {
    using mldsa::Packed3;
    constexpr int CB = GB + 1;
    constexpr int BITS = G2HI ? 4 : 6;
    __shared__ int4 zh[VW][L + 1][64];
    __shared__ uint32_t hint_lds[VW][mldsa::HINT_LDS_DWORDS];
    __shared__ Twiddle tw_lds[(FWD_TW + INV_TW) * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < FWD_TW * 64; i += 64 * VW) tw_lds[i] = fwd_tab[i];
    for (int i = threadIdx.x; i < INV_TW * 64; i += 64 * VW) tw_lds[FWD_TW * 64 + i] = inv_tab[i];
    __syncthreads();
    const mldsa::LdsTw ftw{tw_lds, lane};
    const mldsa::LdsTw itw{tw_lds + FWD_TW * 64, lane};
    const uint32_t wid = blockIdx.x * VW + wave, n_waves = gridDim.x * VW;

    for (size_t op = wid; op < n_ops; op += n_waves) {
        // the lane index made opaque per op (the core's measurement: address arithmetic on it is redone where it is used instead of
        // being kept across the op loop: 18-24 VGPRs less, -6 % / -3 % run time for ML-DSA-65 / 87)
        unsigned ul = (unsigned)lane;
        asm volatile("" : "+v"(ul));
        const size_t key = key_idx ? (size_t)__builtin_amdgcn_readfirstlane((int)key_idx[op]) : key_base + op;
        const Packed3* arow = reinterpret_cast<const Packed3*>(a_hat + (op * K * (size_t)L) * mldsa::PACKED_POLY_DWORDS);
        const int4* trow = reinterpret_cast<const int4*>(t1 + (key * K) * (size_t)N);
        // (nontemporal, field.h "Cache policy": the op's own ExpandA output is read exactly once)
        Packed3 av[L];
#pragma unroll
        for (int j = 0; j < L; j++) av[j] = mldsa::load_row<mldsa::NT_A_VERIFY>(&arow[(unsigned)(j * 64) + ul]);
        int4 tv = trow[ul];
        // ---- (c_tilde, z, h) <- sigDecode: z in the forward loop, the hint bytes requested here and decoded after it
        const uint8_t* zsrc = sigs + op * sig_len + ctilde_len;
        const mldsa::HintBytes hbytes = mldsa::hint_load(zsrc + L * (32 * CB), omega, K, (int)ul);
        bool zbad = false;
#pragma unroll 1
        for (int j = 0; j <= L; j++) {
            asm volatile("" ::: "memory");  // keep the LDS twiddle reads at their point of use
            int32_t r[4];
            if (j < L) {
                const uint8_t* src = zsrc + (size_t)j * (32 * CB);
                int32_t mx = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    // one byte-granular dword load per field; hints follow z: the over-read is in-buffer
                    r[k] = mldsa::y_from_raw<CB>(mldsa::y_raw_dword<CB, mldsa::NT_ZC>(src, k, (int)ul), (int)ul);
                    const int32_t a = r[k] < 0 ? -r[k] : r[k];
                    mx = a > mx ? a : mx;
                }
                zbad |= mx >= zbound;
            } else {  // c: k_sample_in_ball's bytes, the lane's four coefficients in its dword
                const uint32_t d = mldsa::load_once<mldsa::NT_ZC>(c + op * 64 + ul);
                r[0] = (int8_t)(d & 0xFF); r[1] = (int8_t)((d >> 8) & 0xFF); r[2] = (int8_t)((d >> 16) & 0xFF); r[3] = (int8_t)(d >> 24);
            }
            mldsa_vfy::ntt_fwd_wave(r, ftw, lane);
            if (j == L) {
#pragma unroll
                for (int k = 0; k < 4; k++) r[k] = mldsa::mont_mul(r[k], -1);  // -c_hat * 2^-32: the rows ADD its product with t1
            }
            zh[wave][j][lane] = make_int4(r[0], r[1], r[2], r[3]);
        }
        const bool hint_ok = mldsa::hint_unpack_wave<K>(hbytes, omega, hint_lds[wave], (int)ul);  // the masks stay in LDS for the rows below
        // ||z||inf >= gamma1 - beta and a malformed hint section as per-op flags for the verdict
        if (lane == 0) {
            znorm[op] = __ballot(zbad) != 0ull ? 0x7fffffff : 0;
            hvalid[op] = hint_ok ? 1 : 0;
        }
        // ---- rows, two per trip on two named register sets (K is even): the prefetch of row i + 1 lands in the registers that row reads,
        // where one set cost 15 v_mov a row to hand `next` over to `current`
        auto row = [&](int i, const Packed3 (&a_cur)[L], const int4& t_cur, Packed3 (&a_nxt)[L], int4& t_nxt, bool more) {
            // 64-bit accumulation, one Montgomery reduction per coefficient and row (field.h): |a| < 2^24, |z_hat| < 9 q, at most
            // L + 1 <= 8 terms: |sum| < 2^54 = the reduction's input bound.  c_hat * 2^-32 in (-q, q); t1 from mldsa_pk_expand is in
            // (-q, q); zh[L] holds it negated, so the whole row is one chain of v_mad_i64_i32 with no 64-bit subtraction behind it.
            const int4 cv = zh[wave][L][lane];
            int64_t acc64[4] = {(int64_t)cv.x * t_cur.x, (int64_t)cv.y * t_cur.y, (int64_t)cv.z * t_cur.z, (int64_t)cv.w * t_cur.w};
#pragma unroll
            for (int j = 0; j < L; j++) {
                const int4 zv = zh[wave][j][lane];
                const int4 a4 = mldsa::unpack24(a_cur[j]);
                acc64[0] += (int64_t)a4.x * zv.x;
                acc64[1] += (int64_t)a4.y * zv.y;
                acc64[2] += (int64_t)a4.z * zv.z;
                acc64[3] += (int64_t)a4.w * zv.w;
            }
            int32_t acc[4];
            if (more) {  // next row: in flight during this row's inverse transform
#pragma unroll
                for (int j = 0; j < L; j++) a_nxt[j] = mldsa::load_row<mldsa::NT_A_VERIFY>(&arow[(unsigned)(((i + 1) * L + j) * 64) + ul]);
                t_nxt = trow[(unsigned)((i + 1) * 64) + ul];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] = mldsa::mont_reduce64(acc64[k]);  // (-q, q): the inverse transform's input range
            mldsa_vfy::ntt_inv_wave(acc, itw, lane, mldsa::F_MONT2);
            // acc[k] = w'[64 k + lane], canonical.  UseHint, then pack BITS-bit fields.  The hint bit of coefficient 64 k + lane is bit
            // lane & 31 of mask word 2 k + (lane >> 5): read from the masks hint_unpack_wave left in LDS, two addresses per wave and k
            const uint32_t* hrow = hint_lds[wave] + 24 + i * 8 + (ul >> 5);
            uint8_t* dst = w1 + op * w1_stride + (size_t)i * (32 * BITS);
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t h = (hrow[2 * k] >> (ul & 31)) & 1u;
                v[k] = (uint32_t)mldsa::use_hint<G2HI>((int32_t)h, acc[k]);
            }
            pack_w1_strided<G2HI>(v, dst, lane);
        };
        static_assert(K % 2 == 0, "the row loop runs two rows a trip");
        Packed3 aw[L];
        int4 tw2;
#pragma unroll 1
        for (int i = 0; i < K; i += 2) {
            asm volatile("" ::: "memory");
            row(i, av, tv, aw, tw2, true);
            asm volatile("" ::: "memory");
            row(i + 1, aw, tw2, av, tv, i + 2 < K);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ c~ hash and verdict
// c_tilde' = H(mu | w1Encode(w1'), OUT bytes) and the verdict of verify_internal: the core's k_shake256_2<OUT, true> in its verdict form.
// One op per lane for the permutation; for every rate block the wave loads the 64 ops' 136-byte pieces cooperatively into an LDS tile.
constexpr int CWAVES = 4;
constexpr int CBLOCK = 64 * CWAVES;
template <int OUT>
__global__ __launch_bounds__(CBLOCK) void k_ctilde_verdict(const uint8_t* __restrict__ mu_w1, size_t mw, const uint8_t* __restrict__ sigs, size_t sig_len,
                                                           const int32_t* __restrict__ znorm, int32_t zbound, const int32_t* __restrict__ hvalid,
                                                           const int32_t* __restrict__ ctx_bad, uint8_t* __restrict__ ok, size_t n_ops) {
    __shared__ uint32_t tiles[CWAVES * 64 * mldsa::H_STRIDE];
    __shared__ unsigned long long ptr_a[CWAVES * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* tile = tiles + wave * 64 * mldsa::H_STRIDE;
    const size_t base_op = (size_t)blockIdx.x * CBLOCK;
    if (base_op >= n_ops) return;
    const size_t op = base_op + threadIdx.x;
    const bool valid = op < n_ops;
    // rows of ops past the end of the batch point at the tile's first op: their loads stay legal, their results unused
    const size_t opc = valid ? op : base_op;
    ptr_a[wave * 64 + lane] = (unsigned long long)(mu_w1 + opc * mw);
    mldsa::wave_lds_sync_c();
    KeccakState st;
    mldsa::shake256_2_absorb<true>(st, tile, ptr_a + wave * 64, ptr_a + wave * 64, (int)mw, 0, 0, 0, lane);
    if (!valid) return;
    const uint8_t* c0 = sigs + op * sig_len;  // c_tilde opens the signature
    uint32_t diff = 0;
    static_for<0, OUT / 8>([&](auto wc) {
        constexpr int W = decltype(wc)::value;
        diff |= (st.lo[W] ^ load_le32(c0 + 8 * W)) | (st.hi[W] ^ load_le32(c0 + 8 * W + 4));
    });
    ok[op] = (uint8_t)(diff == 0 && znorm[op] < zbound && hvalid[op] && !ctx_bad[op]);
}

}  // namespace mldsa_vfy

// --------------------------------------------------------------------------------------------------------------- host side
namespace {

using namespace mldsa_layer;
using namespace mldsa_vfy;

// What the library owns on a device, for as long as the process lives: the two streams of the parts, the events that order them, the
// NTT twiddle tables k_verify_main reads (the core's generator, ../csrc/tables.h), and the profile record.
struct DevState {
    int dev = -1;
    int n_cu = 256;
    hipStream_t ea = nullptr, vm = nullptr;  // several parts: ExpandA | verify_main and the c~ hash.  One part: unused | the front
    std::vector<hipEvent_t> ev;              // ordering events, handed out per call from the front
    Twiddle *fwd = nullptr, *inv = nullptr;
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;      // 2 per recorded launch
    std::vector<const char*> prof_name;
    size_t prof_used = 0;
};

std::mutex g_mutex;  // one enqueue at a time: the streams and the events are shared by every call of the process
std::vector<DevState*> g_states;
size_t g_part_ops = 0;  // mldsa_vfy_set_part_ops; 0 = MLDSA_VFY_PART_OPS

size_t part_ops() { return g_part_ops ? g_part_ops : (size_t)MLDSA_VFY_PART_OPS; }

// (g_mutex held, the device current)
int dev_state(const char* fn, int dev, DevState** out) {
    for (DevState* d : g_states)
        if (d->dev == dev) {
            *out = d;
            return MLDSA_OK;
        }
    DevState* d = new DevState;
    d->dev = dev;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cu > 0) d->n_cu = cu;
    const std::vector<mldsa::HostTwiddle> f = mldsa::gen_fwd_lane_twiddles(), i = mldsa::gen_inv_lane_twiddles();
    hipError_t e = hipStreamCreateWithFlags(&d->ea, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->vm, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&d->fwd, f.size() * sizeof(Twiddle));
    if (e == hipSuccess) e = hipMalloc(&d->inv, i.size() * sizeof(Twiddle));
    if (e == hipSuccess) e = hipMemcpy(d->fwd, f.data(), f.size() * sizeof(Twiddle), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->inv, i.data(), i.size() * sizeof(Twiddle), hipMemcpyHostToDevice);
    if (e != hipSuccess || f.size() != (size_t)FWD_TW * 64 || i.size() != (size_t)INV_TW * 64) {
        if (d->ea) (void)hipStreamDestroy(d->ea);
        if (d->vm) (void)hipStreamDestroy(d->vm);
        if (d->fwd) (void)hipFree(d->fwd);
        if (d->inv) (void)hipFree(d->inv);
        delete d;
        (void)hipGetLastError();
        return e != hipSuccess ? hip_failed(fn, "creating the library's streams and tables", e)
                               : fail(MLDSA_ERR_DEVICE, std::string(fn) + ": the core's twiddle tables have another shape");
    }
    g_states.push_back(d);
    *out = d;
    return MLDSA_OK;
}

// ordering events of one call, from the state's pool (grown on demand)
struct Events {
    DevState* d;
    size_t used = 0;
    hipError_t err = hipSuccess;
    explicit Events(DevState* d_) : d(d_) {}
    hipEvent_t next() {
        if (used == d->ev.size()) {
            hipEvent_t e = nullptr;
            const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (rc != hipSuccess) {
                err = rc;
                return nullptr;
            }
            d->ev.push_back(e);
        }
        return d->ev[used++];
    }
};

// an event pair around the launches of one stage of one part, when profiling is on
constexpr size_t PROF_MAX_PAIRS = 4096;
struct ProfScope {
    DevState* d;
    hipStream_t s;
    long idx = -1;
    ProfScope(DevState* d_, hipStream_t s_, const char* name) : d(d_), s(s_) {
        if (!d->prof_on || d->prof_used >= PROF_MAX_PAIRS) return;  // (a record nobody reports stops growing)
        if (d->prof_used * 2 + 2 > d->prof_ev.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess) return;
            if (hipEventCreate(&b) != hipSuccess) {
                (void)hipEventDestroy(a);
                return;
            }
            d->prof_ev.push_back(a);
            d->prof_ev.push_back(b);
            d->prof_name.push_back(name);
        } else {
            d->prof_name[d->prof_used] = name;
        }
        idx = (long)d->prof_used++;
        (void)hipEventRecord(d->prof_ev[2 * idx], s);
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(d->prof_ev[2 * idx + 1], s);
    }
};

#define VFY_HIP(call, what)                                     \
    do {                                                        \
        const hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_failed(fn, what, e_);  \
    } while (0)

// by parameter set: K, L, log2(gamma1), gamma2 == (q - 1) / 32, c_tilde bytes, waves per SIMD of k_verify_main (the core's choices)
#define VFY_BY_SET(set, M)              \
    do {                                \
        if ((set) == MLDSA_44) M(4, 4, 17, false, 32, 5); \
        else if ((set) == MLDSA_65) M(6, 5, 19, true, 48, 4); \
        else M(8, 7, 19, true, 64, 4);  \
    } while (0)

unsigned stream_blocks(size_t n_streams) { return (unsigned)((n_streams + 64 * SWAVES - 1) / (64 * SWAVES)); }

void launch_expand_a(int set, const uint8_t* rho, const uint32_t* key_idx, int32_t* a_hat, size_t n, uint32_t n_keys, hipStream_t s) {
    mldsa_params p;
    (void)mldsa_get_params(set, &p);
    const dim3 grid(stream_blocks(n * (size_t)(p.k * p.l))), block(64 * SWAVES);
#define VFY_EA(KK, LL, GB, G2, CT, MW) hipLaunchKernelGGL((k_expand_a<KK, LL>), grid, block, 0, s, rho, (size_t)32, key_idx, a_hat, n, n_keys)
    VFY_BY_SET(set, VFY_EA);
#undef VFY_EA
}

struct Call {
    int set, mode;
    mldsa_params p;
    const uint8_t *rho, *tr;
    const int32_t* t1;
    size_t n_keys;
    const uint32_t* key_idx;
    const uint8_t* msgs;
    const uint64_t* msg_off;
    const uint8_t* ctxs;
    const uint64_t* ctx_off;
    const uint8_t* sigs;
    uint8_t* ok;
    size_t n_ops;
};

// Enqueues the whole call (g_mutex held, the device current): order_plan() of vfy_parts.h says on which lane every stage of every part
// runs and which events order the lanes; this function walks the plan and issues one runtime call per step.  Lanes: `s` the caller's
// stream, d->ea, d->vm.
// One part (every call up to MLDSA_VFY_PART_OPS ops): one chain on the caller's stream, the front beside it -- two streams in flight.
//   s:     fork | ExpandA | waits for the front | verify_main | c~ hash and verdict
//   d->vm: waits for the fork | key-index check, mu, SampleInBall | front
//   (a cross-queue hand-over costs about 10 us, section 4 of DESIGN.md: with ExpandA, verify_main and the c~ hash on the library's streams
//   a call paid three of them on its critical path; here the one wait left completes at about the time ExpandA does)
// Several parts: three in flight.
//   s:     fork | per part: key-index check, mu, SampleInBall, front[p] | ... | waits for the join
//   d->ea: waits for the fork | per part p: waits for used[p - 2] (the ring half is free), ExpandA, ready[p]
//   d->vm: per part p: waits for ready[p] and front[p], verify_main, used[p] (when a part p + 2 follows), c~ hash and verdict | join
int enqueue(const char* fn, DevState* d, const Call& c, uint8_t* scratch, hipStream_t s) {
    const mldsa_params& p = c.p;
    const PartPlan plan(c.n_ops, part_ops());
    const Carve cv = carve(p.k, p.l, (size_t)p.w1_len, plan);
    const size_t mw = 64 + (size_t)p.w1_len;
    uint32_t* c8 = reinterpret_cast<uint32_t*>(scratch + cv.c);
    int32_t* znorm = reinterpret_cast<int32_t*>(scratch + cv.znorm);
    int32_t* hvalid = reinterpret_cast<int32_t*>(scratch + cv.hvalid);
    int32_t* ctx_bad = reinterpret_cast<int32_t*>(scratch + cv.ctx_bad);
    int32_t* key_bad = reinterpret_cast<int32_t*>(scratch + cv.key_bad);
    uint32_t* kidx = reinterpret_cast<uint32_t*>(scratch + cv.kidx);
    uint8_t* mu_w1 = scratch + cv.mu_w1;
    const size_t sig_len = (size_t)p.sig_len;

    const OrderPlan order = order_plan(plan.n_parts());
    const hipStream_t lanes[N_LANES] = {s, d->ea, d->vm};
    Events evs(d);
    std::vector<hipEvent_t> ev(order.n_events);
    for (hipEvent_t& e : ev) e = evs.next();
    if (evs.err != hipSuccess) return hip_failed(fn, "creating an event", evs.err);

    for (const Step& st : order.steps) {
        const hipStream_t q = lanes[st.lane];
        if (st.act == ACT_RECORD) {
            VFY_HIP(hipEventRecord(ev[st.n], q), (std::string("recording ") + st.what).c_str());
            continue;
        }
        if (st.act == ACT_WAIT) {
            VFY_HIP(hipStreamWaitEvent(q, ev[st.n], 0), (std::string("waiting for ") + st.what).c_str());
            continue;
        }
        const Part part = plan.at(st.n);
        const size_t o = part.first, n = part.count;
        const size_t key_base = c.key_idx ? 0 : o;  // identity mapping: op i uses key i
        int32_t* a_hat = reinterpret_cast<int32_t*>(scratch + cv.ring[part.half]);
        const uint8_t* sg = c.sigs + o * sig_len;
        // the key index k_sanitize_keys leaves for the part, and its flags
        const uint32_t* kp = c.key_idx ? kidx + o : nullptr;
        const int32_t* kb = c.key_idx ? key_bad + o : nullptr;
        switch (st.stage) {
        case STAGE_EXPAND_A: {
            ProfScope ps(d, q, "expand_a");
            launch_expand_a(c.set, c.rho + key_base * 32, c.key_idx ? c.key_idx + o : nullptr, a_hat, n, c.key_idx ? (uint32_t)c.n_keys : 0u, q);
            break;
        }
        // ---- the front of the part, beside ExpandA and enqueued behind it.  (Five ExpandA waves leave a SIMD 32 VGPRs, so SampleInBall's
        // waves get a slot only as ExpandA's drain: it ends with ExpandA, 1.06 ms instead of 0.19.  Launching the front ahead of ExpandA,
        // SampleInBall on the arithmetic stream, brought it to 0.04 ms and made the call 1-2 % SLOWER in the same-box alternation: not
        // kept.)
        case STAGE_FRONT: {
            if (c.key_idx)
                hipLaunchKernelGGL(k_sanitize_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, c.key_idx + o, (uint32_t)c.n_keys, n, kidx + o, key_bad + o);
            {
                ProfScope ps(d, q, "mu");
                hipLaunchKernelGGL(k_mu, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, q, c.tr + key_base * 64, (size_t)64, kp, c.mode, c.msgs, c.msg_off, c.ctxs,
                                   c.ctx_off, mu_w1 + o * mw, mw, ctx_bad + o, kb, n, o, c.n_ops);
            }
            {
                ProfScope ps(d, q, "sample_in_ball");
                const dim3 grid((unsigned)((n + 63) / 64)), block(64);
#define VFY_SIB(KK, LL, GB, G2, CT, MW) hipLaunchKernelGGL((k_sample_in_ball<CT>), grid, block, 0, q, sg, sig_len, p.tau, c8 + o * 64, n)
                VFY_BY_SET(c.set, VFY_SIB);
#undef VFY_SIB
            }
            break;
        }
        case STAGE_VERIFY_MAIN: {
            ProfScope ps(d, q, "verify_main");
            const size_t need = (n + VW - 1) / VW, cap = (size_t)d->n_cu * 16;  // the core's grid_for(.., VW, 16)
            const dim3 grid((unsigned)(need < cap ? need : cap)), block(64 * VW);
#define VFY_VM(KK, LL, GB, G2, CT, MW)                                                                                                         \
    hipLaunchKernelGGL((k_verify_main<KK, LL, GB, G2, MW>), grid, block, 0, q, reinterpret_cast<const uint32_t*>(a_hat), sg, sig_len,          \
                       p.ctilde_len, c8 + o * 64, c.t1, kp, key_base, hvalid + o, p.omega, mu_w1 + o * mw + 64, mw, znorm + o, p.gamma1 - p.beta, n, \
                       d->fwd, d->inv)
            VFY_BY_SET(c.set, VFY_VM);
#undef VFY_VM
            break;
        }
        default: {  // STAGE_CTILDE
            ProfScope ps(d, q, "ctilde_hash");
            const dim3 grid((unsigned)((n + CBLOCK - 1) / CBLOCK)), block(CBLOCK);
#define VFY_CT(KK, LL, GB, G2, CT, MW)                                                                                                    \
    hipLaunchKernelGGL((k_ctilde_verdict<CT>), grid, block, 0, q, mu_w1 + o * mw, mw, sg, sig_len, znorm + o, p.gamma1 - p.beta, hvalid + o, \
                       ctx_bad + o, c.ok + o, n)
            VFY_BY_SET(c.set, VFY_CT);
#undef VFY_CT
            break;
        }
        }
        LAYER_LAUNCHED(st.what);
    }
    return MLDSA_OK;
}

// When an enqueue failed half way the caller's stream must still come behind whatever was launched on the library's streams.
void drain(DevState* d) {
    (void)hipStreamSynchronize(d->ea);
    (void)hipStreamSynchronize(d->vm);
    (void)hipGetLastError();
}

size_t scratch_bytes_of(int set, size_t n_ops) {
    mldsa_params p;
    if (mldsa_get_params(set, &p) != MLDSA_OK || n_ops > MLDSA_VFY_MAX_OPS) return 0;
    return carve(p.k, p.l, (size_t)p.w1_len, PartPlan(n_ops, part_ops())).bytes;
}

}  // namespace

extern "C" {

int mldsa_vfy_abi_version(void) { return MLDSA_VFY_ABI_VERSION; }

const char* mldsa_vfy_last_error(void) { return g_err.c_str(); }

size_t mldsa_vfy_scratch_bytes(int set, size_t n_ops) {
    std::lock_guard<std::mutex> lk(g_mutex);
    return scratch_bytes_of(set, n_ops);
}

size_t mldsa_vfy_set_part_ops(size_t part) {
    std::lock_guard<std::mutex> lk(g_mutex);
    const size_t before = part_ops();
    g_part_ops = part;
    return before;
}

int mldsa_vfy_verify(mldsa_ctx* ctx, int set, int mode, const uint8_t* rho, const uint8_t* tr, const int32_t* t1_d2_hat_mont, size_t n_keys,
                     const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off,
                     const uint8_t* sigs, uint8_t* ok, size_t n_ops, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_vfy_verify";
    Call c;
    const int rc = check_common(fn, ctx, set, n_ops, MLDSA_VFY_MAX_OPS, "MLDSA_VFY_MAX_OPS ops", &c.p);
    if (rc != MLDSA_OK) return rc;
    if (mode != MLDSA_MODE_PURE && mode != MLDSA_MODE_INTERNAL && mode != MLDSA_MODE_PREHASH)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": bad mode");
    if (n_ops == 0) return MLDSA_OK;
    if (!rho || !tr || !t1_d2_hat_mont || !msg_off || !sigs || !ok) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (key_idx ? n_keys == 0 : n_keys < n_ops) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys does not cover the batch");
    if (n_keys > 0xFFFFFFFFu) n_keys = 0xFFFFFFFFu;  // (as the core: an index is 32 bits; without key_idx only keys 0 ... n_ops - 1 are read)
    if (!aligned(t1_d2_hat_mont, 16)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": t1_d2_hat_mont must be 16-byte aligned");
    if (!scratch || !aligned(scratch, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL or not 256-byte aligned");
    LAYER_ON_DEVICE(ctx);
    std::lock_guard<std::mutex> lk(g_mutex);
    if (scratch_bytes < scratch_bytes_of(set, n_ops))
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch is below mldsa_vfy_scratch_bytes(set, n_ops)");
    DevState* d = nullptr;
    const int src = dev_state(fn, dev_, &d);
    if (src != MLDSA_OK) return src;
    c.set = set; c.mode = mode; c.rho = rho; c.tr = tr; c.t1 = t1_d2_hat_mont; c.n_keys = n_keys; c.key_idx = key_idx; c.msgs = msgs;
    c.msg_off = msg_off; c.ctxs = ctxs; c.ctx_off = ctx_off; c.sigs = sigs; c.ok = ok; c.n_ops = n_ops;
    const int erc = enqueue(fn, d, c, static_cast<uint8_t*>(scratch), (hipStream_t)stream);
    if (erc != MLDSA_OK) drain(d);
    return erc;
}

int mldsa_vfy_expand_a(mldsa_ctx* ctx, int set, const uint8_t* rho, int32_t* a_hat, size_t n_ops, void* stream) {
    const char* fn = "mldsa_vfy_expand_a";
    mldsa_params p;
    const int rc = check_common(fn, ctx, set, n_ops, MLDSA_VFY_MAX_OPS, "MLDSA_VFY_MAX_OPS ops", &p);
    if (rc != MLDSA_OK) return rc;
    if (n_ops == 0) return MLDSA_OK;
    if (!rho || !a_hat) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(a_hat, 16)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": a_hat must be 16-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const size_t n_polys = n_ops * (size_t)(p.k * p.l);
    void* packed = nullptr;
    VFY_HIP(hipMalloc(&packed, n_polys * PACKED_POLY_BYTES), "allocating the packed rows");
    launch_expand_a(set, rho, nullptr, static_cast<int32_t*>(packed), n_ops, 0u, s);
    hipLaunchKernelGGL(k_unpack_a, dim3((unsigned)((n_polys + 3) / 4)), dim3(256), 0, s, static_cast<const uint32_t*>(packed), a_hat, n_polys);
    hipError_t e = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(s);
    if (e == hipSuccess) e = se;
    (void)hipFree(packed);
    return e == hipSuccess ? MLDSA_OK : hip_failed(fn, "ExpandA and unpack", e);
}

int mldsa_vfy_profile_enable(mldsa_ctx* ctx, int on) {
    const char* fn = "mldsa_vfy_profile_enable";
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    LAYER_ON_DEVICE(ctx);
    std::lock_guard<std::mutex> lk(g_mutex);
    DevState* d = nullptr;
    const int rc = dev_state(fn, dev_, &d);
    if (rc != MLDSA_OK) return rc;
    d->prof_on = on != 0;
    if (!d->prof_on) d->prof_used = 0;
    return MLDSA_OK;
}

int mldsa_vfy_profile_report(mldsa_ctx* ctx, char* buf, size_t buf_len) {
    const char* fn = "mldsa_vfy_profile_report";
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!buf || buf_len <= 2) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": bad argument");
    LAYER_ON_DEVICE(ctx);
    std::lock_guard<std::mutex> lk(g_mutex);
    DevState* d = nullptr;
    const int rc = dev_state(fn, dev_, &d);
    if (rc != MLDSA_OK) return rc;
    VFY_HIP(hipDeviceSynchronize(), "waiting for the device");
    struct Acc { const char* name; double ms; size_t calls; };
    std::vector<Acc> acc;
    for (size_t i = 0; i < d->prof_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, d->prof_ev[2 * i], d->prof_ev[2 * i + 1]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        bool found = false;
        for (auto& a : acc)
            if (strcmp(a.name, d->prof_name[i]) == 0) {
                a.ms += ms;
                a.calls++;
                found = true;
                break;
            }
        if (!found) acc.push_back({d->prof_name[i], ms, 1});
    }
    std::string out = "{";
    for (size_t i = 0; i < acc.size(); i++)
        out += std::string(i ? ", " : "") + "\"" + acc[i].name + "\": {\"ms\": " + std::to_string(acc[i].ms) + ", \"calls\": " + std::to_string(acc[i].calls) + "}";
    out += "}";
    if (out.size() + 1 > buf_len) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    d->prof_used = 0;
    return MLDSA_OK;
}

}  // extern "C"
