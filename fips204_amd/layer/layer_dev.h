// The device helpers the layered libraries' kernels share (mu/, seed/, keycheck/; ph/stream.hip and mus/ take wave_max; crl/ and find/
// take wave_sum): the wave-wide OR, sum and maximum, the canonical representative, and the shapes two or more of them agree on -- the LDS tile of the lane-per-state SHAKE256
// and the packed t1 row.  Helpers only: every
// kernel (__global__) stays in its library's .hip file.  The core's device headers are included read-only.
//
// A piece is shared here only if every kernel that uses it compiles to the same instructions as with the piece written out.  Three did
// not pass and stay in the kernels, each with its comments: Power2Round with the lane-shuffle pack of a t1 row (k_seed_t, k_kc_row), the
// staging loop and the XOR step of the SHAKE256 tile (k_commit, k_seed_tr, k_kc_tr), and the OR reduction of k_seed_cmp.  As helpers --
// function or lambda hook, by value or by reference -- they are optimised before they are inlined, and the kernels come out with other
// registers, another schedule or the opposite branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc/field.h"
#include "../csrc/keccak.h"
#include "../csrc/rounding.h"

namespace mldsa_layer {

using mldsa::KeccakState;
using mldsa::u32_any;
typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));

// Lane-per-state SHAKE256 over an LDS tile (k_commit, k_seed_tr, k_kc_tr): one item (an op, a key) per lane.  For every rate block the
// wave stages the 64 items' RATE_DW dwords into tile[64 * TILE_STRIDE] cooperatively -- consecutive lanes on consecutive dwords of one
// item: coalesced loads; item o's dword j at tile[o * TILE_STRIDE + j] --, then, between two __syncthreads, each lane XORs its own row
// (tile + lane * TILE_STRIDE) into its state and permutes.
constexpr int RATE_DW = mldsa::SHAKE256_RATE / 4;  // 34 dwords per rate block
constexpr int TILE_STRIDE = RATE_DW + 1;           // odd row stride: the lanes' rows fall on different banks

constexpr int T1_ROW_DW = 80;  // a row of t1 in a wire public key: 256 coefficients of 10 bits

// OR over the wave, the same word in every lane
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// sum over the wave, the same value in every lane
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
    return v;
}

// maximum over the wave, the same value in every lane
__device__ __forceinline__ size_t wave_max(size_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const size_t o = (size_t)__shfl_xor((unsigned long long)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// (-q, 2 q) -> [0, q)
__device__ __forceinline__ int32_t canon(int32_t x) {
    x += (x >> 31) & mldsa::Q;
    return x - (((mldsa::Q - 1 - x) >> 31) & mldsa::Q);
}

}  // namespace mldsa_layer
