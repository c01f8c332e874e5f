// SHA-256 and SHA-512 compression functions for gfx950, one hash state per lane (FIPS 180-4 §6.2, §6.4), and the initial
// values of the six SHA-2 functions that run on them (SHA-224/256, SHA-384/512, SHA-512/224, SHA-512/256).
//
// The HashML-DSA pre-hash PH(M) (reference src/hashing.rs:317-354) runs one message per lane, 64 messages per wave,
// like k_mu's SHAKE256 (csrc/kernels_codec.hip).  The state and the 16-word message schedule live in VGPRs; SHA-512's
// 64-bit words are (lo, hi) dword pairs.  Rounds are fully unrolled with compile-time indices, so every round
// constant is a literal of the instruction stream (round_const): no constant table in LDS or global memory.
//
// Instruction choices (gfx950):
//   Ch(e, f, g)  = v_bitop3_b32 truth table 0xCA      Maj(a, b, c) = 0xE8      x ^ y ^ z = 0x96 (gfx950 has no v_xor3_b32)
//   32-bit rotate = one v_alignbit_b32; 64-bit rotate = two, as csrc/keccak.h rotl64 does
//   64-bit adds are v_add_co_u32 / v_addc_co_u32 pairs (the compiler's lowering of uint64_t +)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mldsa_ph {

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

__device__ __forceinline__ uint32_t bop_ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }
__device__ __forceinline__ uint32_t bop_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
__device__ __forceinline__ uint32_t bop_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// byte swap of one dword: one v_perm_b32 (big-endian words of SHA-2)
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00010203u); }

// A round constant as an SGPR operand materialised in its own round.  Left alone, the compiler hoists all 64 / 160
// constant dwords out of the block loop into SGPRs, and SHA-512's do not fit (SGPR spills to VGPR lanes).  The empty
// volatile asm keeps each one next to its use: one s_mov_b32 on the scalar unit, beside the vector work.
__device__ __forceinline__ uint32_t round_const(uint32_t k) {
    asm volatile("" : "+s"(k));
    return k;
}

template <int R>
__device__ __forceinline__ uint32_t rotr32(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, R); }

// ---------------------------------------------------------------------------------------------------------------- SHA-256
struct Sha256State {
    uint32_t h[8];
};

// Initial values (FIPS 180-4 §5.3).  SHA-256 / SHA-512: fractional parts of the square roots of the first eight primes;
// SHA-384: of the 9th-16th primes; SHA-224: the low 32 bits of SHA-384's.
constexpr uint32_t IV256_SHA256[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint32_t IV256_SHA224[8] = {0xc1059ed8u, 0x367cd507u, 0x3070dd17u, 0xf70e5939u, 0xffc00b31u, 0x68581511u, 0x64f98fa7u, 0xbefa4fa4u};

// iv: 0 = SHA-256, 1 = SHA-224 (PhVar::iv)
__device__ __forceinline__ void sha256_init(Sha256State& s, int iv) {
    static_for<0, 8>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        s.h[i] = iv == 1 ? IV256_SHA224[i] : IV256_SHA256[i];
    });
}

struct Sha256K {
    static constexpr uint32_t k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
};

// one 64-byte block, w[16] = its big-endian words (overwritten: the schedule is rolled in place)
__device__ __forceinline__ void sha256_block(Sha256State& s, uint32_t (&w)[16]) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = s.h[i];
    static_for<0, 64>([&](auto ic) {
        constexpr int t = decltype(ic)::value;
        constexpr uint32_t kt = Sha256K::k[t];
        if constexpr (t >= 16) {
            const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
            const uint32_t s0 = bop_xor3(rotr32<7>(w15), rotr32<18>(w15), w15 >> 3);
            const uint32_t s1 = bop_xor3(rotr32<17>(w2), rotr32<19>(w2), w2 >> 10);
            w[t & 15] = w[t & 15] + s0 + w[(t - 7) & 15] + s1;
        }
        // registers rotate by renaming: v[(8 - t) & 7] is a at round t
        uint32_t& a = v[(0 - t) & 7]; uint32_t& b = v[(1 - t) & 7]; uint32_t& c = v[(2 - t) & 7]; uint32_t& d = v[(3 - t) & 7];
        uint32_t& e = v[(4 - t) & 7]; uint32_t& f = v[(5 - t) & 7]; uint32_t& g = v[(6 - t) & 7]; uint32_t& h = v[(7 - t) & 7];
        const uint32_t t1 = h + bop_xor3(rotr32<6>(e), rotr32<11>(e), rotr32<25>(e)) + bop_ch(e, f, g) + round_const(kt) + w[t & 15];
        const uint32_t t2 = bop_xor3(rotr32<2>(a), rotr32<13>(a), rotr32<22>(a)) + bop_maj(a, b, c);
        d += t1;
        h = t1 + t2;  // h becomes the next round's a
    });
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] += v[i];
}

// ---------------------------------------------------------------------------------------------------------------- SHA-512
struct U64 {
    uint32_t lo, hi;
};

__device__ __forceinline__ U64 add64(U64 a, U64 b) {
    const uint64_t r = (((uint64_t)a.hi << 32) | a.lo) + (((uint64_t)b.hi << 32) | b.lo);
    return {(uint32_t)r, (uint32_t)(r >> 32)};
}
__device__ __forceinline__ U64 lit64(uint64_t k) { return {(uint32_t)k, (uint32_t)(k >> 32)}; }

template <int R>
__device__ __forceinline__ U64 rotr64(U64 x) {
    static_assert(R > 0 && R < 64 && R != 32, "rotate amount");
    if constexpr (R < 32) return {__builtin_amdgcn_alignbit(x.hi, x.lo, R), __builtin_amdgcn_alignbit(x.lo, x.hi, R)};
    else return {__builtin_amdgcn_alignbit(x.lo, x.hi, R - 32), __builtin_amdgcn_alignbit(x.hi, x.lo, R - 32)};
}
template <int R>
__device__ __forceinline__ U64 shr64(U64 x) {
    static_assert(R > 0 && R < 32, "shift amount");
    return {__builtin_amdgcn_alignbit(x.hi, x.lo, R), x.hi >> R};
}
__device__ __forceinline__ U64 xor3_64(U64 a, U64 b, U64 c) { return {bop_xor3(a.lo, b.lo, c.lo), bop_xor3(a.hi, b.hi, c.hi)}; }
__device__ __forceinline__ U64 ch64(U64 e, U64 f, U64 g) { return {bop_ch(e.lo, f.lo, g.lo), bop_ch(e.hi, f.hi, g.hi)}; }
__device__ __forceinline__ U64 maj64(U64 a, U64 b, U64 c) { return {bop_maj(a.lo, b.lo, c.lo), bop_maj(a.hi, b.hi, c.hi)}; }

struct Sha512State {
    U64 h[8];
};

constexpr uint64_t IV512_SHA512[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                      0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint64_t IV512_SHA384[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull, 0x152fecd8f70e5939ull,
                                      0x67332667ffc00b31ull, 0x8eb44a8768581511ull, 0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
// SHA-512/t (§5.3.6): SHA-512 started from IV512_SHA512 ^ a5a5...a5 over the ASCII string "SHA-512/224" / "SHA-512/256"
constexpr uint64_t IV512_SHA512_224[8] = {0x8c3d37c819544da2ull, 0x73e1996689dcd4d6ull, 0x1dfab7ae32ff9c82ull, 0x679dd514582f9fcfull,
                                          0x0f6d2b697bd44da8ull, 0x77e36f7304c48942ull, 0x3f9d85a86a1d36c8ull, 0x1112e6ad91d692a1ull};
constexpr uint64_t IV512_SHA512_256[8] = {0x22312194fc2bf72cull, 0x9f555fa3c84c64c2ull, 0x2393b86b6f53b151ull, 0x963877195940eabdull,
                                          0x96283ee2a88effe3ull, 0xbe5e1e2553863992ull, 0x2b0199fc2c85b8aaull, 0x0eb72ddc81c52ca2ull};

// iv: 0 = SHA-512, 1 = SHA-384, 2 = SHA-512/224, 3 = SHA-512/256 (PhVar::iv)
__device__ __forceinline__ void sha512_init(Sha512State& s, int iv) {
    static_for<0, 8>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        s.h[i] = lit64(iv == 1 ? IV512_SHA384[i] : iv == 2 ? IV512_SHA512_224[i] : iv == 3 ? IV512_SHA512_256[i] : IV512_SHA512[i]);
    });
}

struct Sha512K {
    static constexpr uint64_t k[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
        0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
        0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
        0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
        0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
        0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
        0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
};

// one 128-byte block, w[16] = its big-endian 64-bit words (overwritten)
__device__ __forceinline__ void sha512_block(Sha512State& s, U64 (&w)[16]) {
    U64 v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = s.h[i];
    static_for<0, 80>([&](auto ic) {
        constexpr int t = decltype(ic)::value;
        constexpr uint64_t kt = Sha512K::k[t];
        if constexpr (t >= 16) {
            const U64 w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
            const U64 s0 = xor3_64(rotr64<1>(w15), rotr64<8>(w15), shr64<7>(w15));
            const U64 s1 = xor3_64(rotr64<19>(w2), rotr64<61>(w2), shr64<6>(w2));
            w[t & 15] = add64(add64(w[t & 15], s0), add64(w[(t - 7) & 15], s1));
        }
        U64& a = v[(0 - t) & 7]; U64& b = v[(1 - t) & 7]; U64& c = v[(2 - t) & 7]; U64& d = v[(3 - t) & 7];
        U64& e = v[(4 - t) & 7]; U64& f = v[(5 - t) & 7]; U64& g = v[(6 - t) & 7]; U64& h = v[(7 - t) & 7];
        const U64 t1 = add64(add64(h, xor3_64(rotr64<14>(e), rotr64<18>(e), rotr64<41>(e))),
                             add64(ch64(e, f, g), add64({round_const((uint32_t)kt), round_const((uint32_t)(kt >> 32))}, w[t & 15])));
        const U64 t2 = add64(xor3_64(rotr64<28>(a), rotr64<34>(a), rotr64<39>(a)), maj64(a, b, c));
        d = add64(d, t1);
        h = add64(t1, t2);
    });
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] = add64(s.h[i], v[i]);
}

}  // namespace mldsa_ph
