// Keccak-f[1600] with theta folded into the rho inputs: 180 VALU per round instead of the 190 of ../csrc/keccak.h.
//
// keccak.h materialises D[x] = C[x-1] ^ rot1(C[x+1]) (10 v_xor) and applies it with one v_xor per state word (50).  Here D never
// exists: every state word takes xor3(A, C[x-1], rot1(C[x+1])) -- one v_bitop3_b32, which issues at the rate of v_xor_b32
// (profiles/prehash_ubench_valu.txt: 2.62 against 2.7 cycles) -- so a round is
//   20 bitop3 (C) + 10 alignbit (rot1 C) + 50 bitop3 (theta) + 48 alignbit (rho) + 50 bitop3 (chi) + 2 xor (iota) = 180.
// Everything else -- rho / pi by two v_alignbit_b32, chi by bitop3 0xD2, iota -- is keccak.h's, and so is the state layout: the
// sponge helpers of keccak.h and sampler_dev.h work on the same KeccakState.
// The squeeze below is rej_ntt_poly_lane_direct of ../csrc/sampler_dev.h on this permutation: the same bytes out.
#pragma once
#include "../csrc/keccak.h"
#include "../csrc/sampler_dev.h"

namespace mldsa_vfy {

using mldsa::KeccakState;

#define VFY_RHOPI(DST, SRC, ROT)                                                                                                  \
    mldsa::rotl64<ROT>(mldsa::xor3(s.lo[SRC], clo[((SRC) + 4) % 5], rlo[((SRC) + 1) % 5]),                                        \
                       mldsa::xor3(s.hi[SRC], chi_[((SRC) + 4) % 5], rhi[((SRC) + 1) % 5]), blo[DST], bhi[DST])

__device__ __forceinline__ void keccak_round180(KeccakState& s, uint32_t rc_lo, uint32_t rc_hi) {
    uint32_t clo[5], chi_[5], rlo[5], rhi[5], blo[25], bhi[25];
#pragma unroll
    for (int x = 0; x < 5; x++) {
        clo[x] = mldsa::xor3(mldsa::xor3(s.lo[x], s.lo[x + 5], s.lo[x + 10]), s.lo[x + 15], s.lo[x + 20]);
        chi_[x] = mldsa::xor3(mldsa::xor3(s.hi[x], s.hi[x + 5], s.hi[x + 10]), s.hi[x + 15], s.hi[x + 20]);
    }
#pragma unroll
    for (int x = 0; x < 5; x++) mldsa::rotl64<1>(clo[x], chi_[x], rlo[x], rhi[x]);
    // theta + rho + pi: B[y][2x+3y] = rotl(A[x][y] ^ C[x-1] ^ rot1(C[x+1]), r[x][y]); flat index = x + 5y
    VFY_RHOPI(0, 0, 0);
    VFY_RHOPI(10, 1, 1);
    VFY_RHOPI(20, 2, 62);
    VFY_RHOPI(5, 3, 28);
    VFY_RHOPI(15, 4, 27);
    VFY_RHOPI(16, 5, 36);
    VFY_RHOPI(1, 6, 44);
    VFY_RHOPI(11, 7, 6);
    VFY_RHOPI(21, 8, 55);
    VFY_RHOPI(6, 9, 20);
    VFY_RHOPI(7, 10, 3);
    VFY_RHOPI(17, 11, 10);
    VFY_RHOPI(2, 12, 43);
    VFY_RHOPI(12, 13, 25);
    VFY_RHOPI(22, 14, 39);
    VFY_RHOPI(23, 15, 41);
    VFY_RHOPI(8, 16, 45);
    VFY_RHOPI(18, 17, 15);
    VFY_RHOPI(3, 18, 21);
    VFY_RHOPI(13, 19, 8);
    VFY_RHOPI(14, 20, 18);
    VFY_RHOPI(24, 21, 2);
    VFY_RHOPI(9, 22, 61);
    VFY_RHOPI(19, 23, 56);
    VFY_RHOPI(4, 24, 14);
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
#pragma unroll
        for (int x = 0; x < 5; x++) {
            s.lo[y + x] = mldsa::chi(blo[y + x], blo[y + (x + 1) % 5], blo[y + (x + 2) % 5]);
            s.hi[y + x] = mldsa::chi(bhi[y + x], bhi[y + (x + 1) % 5], bhi[y + (x + 2) % 5]);
        }
    }
    s.lo[0] ^= rc_lo;
    s.hi[0] ^= rc_hi;
}
#undef VFY_RHOPI

__device__ __forceinline__ void keccak_f1600_180(KeccakState& s) {
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        const uint32_t rc_lo = mldsa::KECCAK_RC_LO[r];
        const uint32_t rc_hi = ((mldsa::KECCAK_RC_HI_BITS >> r) & 1u) << 31;
        keccak_round180(s, rc_lo, rc_hi);
    }
}

// RejNTTPoly into the packed 24-bit row of the lane's stream, the scheme of mldsa::rej_ntt_poly_lane_direct: per group of four
// candidates (three state words) one 12-byte store when all four are below q and four are still wanted, else the accepted ones byte by
// byte.  `st` holds the absorbed, padded seed; out: the packed rows, 768 bytes per stream, stream wave_base + lane is the lane's.
__device__ __forceinline__ void rej_ntt_poly_lane_direct180(KeccakState& st, int32_t* __restrict__ out, size_t wave_base, int lane, bool valid) {
    constexpr uint32_t ROW = mldsa::PACKED_POLY_DWORDS * 4;
    const size_t wb = ((size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(wave_base >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wave_base);
    uint8_t* base = reinterpret_cast<uint8_t*>(out) + wb * ROW;
    const uint32_t end = (uint32_t)(lane + 1) * ROW;  // the row is full when off reaches this
    uint32_t off = valid ? (uint32_t)lane * ROW : end;
    while (__any(off < end)) {
        keccak_f1600_180(st);
        mldsa::static_for<0, 14>([&](auto gc) {  // group G: bytes 12 G .. 12 G + 11 of the 168-byte block = four candidates
            constexpr int G = decltype(gc)::value;
            // coeff_from_three_bytes x 4 in place: bit 23 of every 3-byte field cleared; z >= q <=> z + (2^23 - q) carries into it
            const uint32_t m0 = mldsa::state_word<3 * G>(st) & 0xFF7FFFFFu, m1 = mldsa::state_word<3 * G + 1>(st) & 0xFFFF7FFFu,
                           m2 = mldsa::state_word<3 * G + 2>(st) & 0x7FFFFF7Fu;
            const uint64_t lo = (((uint64_t)m1 << 32) | m0) + 0x1FFF001FFF001FFFull;
            const uint32_t hi = m2 + 0x001FFF00u + (uint32_t)(lo < 0x1FFF001FFF001FFFull ? 1u : 0u);
            const uint32_t over = ((uint32_t)lo & 0x00800000u) | ((uint32_t)(lo >> 32) & 0x00008000u) | (hi & 0x80000080u);
            if (over == 0u && off + 12u <= end) {
                *reinterpret_cast<mldsa::Packed3Unaligned*>(base + off) = mldsa::Packed3Unaligned{m0, m1, m2};
                off += 12u;
            } else if (off < end) {
                const uint32_t c[4] = {m0 & 0x7FFFFFu, __builtin_amdgcn_alignbit(m1, m0, 24) & 0x7FFFFFu,
                                       __builtin_amdgcn_alignbit(m2, m1, 16) & 0x7FFFFFu, m2 >> 8};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (c[k] < (uint32_t)mldsa::Q && off < end) {
                        uint8_t* dst = base + off;
                        dst[0] = (uint8_t)c[k];
                        dst[1] = (uint8_t)(c[k] >> 8);
                        dst[2] = (uint8_t)(c[k] >> 16);
                        off += 3u;
                    }
                }
            }
        });
    }
}

}  // namespace mldsa_vfy
