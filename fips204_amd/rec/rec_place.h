// The placement scan of libmldsa_x509sign.so, libmldsa_csr.so (Q = 2: bytes and accepted count) and libmldsa_crl.so (Q = 1: entry
// slots): a stable exclusive scan of Q quantities per item over three launches -- per workgroup the Q sums, one wave that turns the sums
// into exclusive prefixes in place, then per item what lies in front of it.  Helpers only: every kernel stays in its library's .hip file,
// declares its own `__shared__ uint64_t part[WAVES][Q]` and passes it in.  WAVES is the workgroup's size in waves; the launch is
// one-dimensional.
//
// Everything here has internal linkage (the unnamed namespace), for the reason rec_scan.h and ../layer/layer_host.h give.
//
// The rule of ../layer/layer_dev.h holds: a piece is shared only if every kernel that uses it compiles to the same instructions as
// with the piece written out.  The eight kernels that call these keep their registers, LDS and waves per SIMD and have as many
// instructions or fewer; DESIGN.md lists every difference.  For that the kernels keep their quantities in scalars and build the arrays
// at the call (arrays filled inside the kernels' branches did not pass).  k_crl_place did not pass -- 15 VGPRs with place_wave_scan
// and place_before, 13 without -- and keeps its scan written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rec_wave.h"

namespace mldsa_rec {
namespace {

// the lanes' v[q] summed over the workgroup into sums[block][q]; v is left holding the wave's sums
template <size_t Q, size_t WAVES>
__device__ __forceinline__ void place_block_sums(uint64_t (&v)[Q], uint64_t (&part)[WAVES][Q], uint64_t* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < (int)Q; ++q) v[q] += __shfl_xor((unsigned long long)v[q], d, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < (int)Q; ++q) part[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < (int)WAVES; ++w) s += part[w][threadIdx.x];
        sums[(size_t)blockIdx.x * Q + threadIdx.x] = s;
    }
}

// one wave: sums[b][q] -> the sum over the blocks before b (in place); total[q] = the sum over all blocks, in every lane
template <size_t Q>
__device__ __forceinline__ void place_block_offsets(uint64_t* __restrict__ sums, uint32_t n_blocks, uint64_t (&total)[Q]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int q = 0; q < (int)Q; ++q) total[q] = 0;
    for (uint32_t base = 0; base < n_blocks; base += 64) {
        const uint32_t b = base + lane;
#pragma unroll
        for (int q = 0; q < (int)Q; ++q) {
            const uint64_t v = b < n_blocks ? sums[(size_t)b * Q + q] : 0;
            const uint64_t inc = wave_inclusive(v, lane);
            if (b < n_blocks) sums[(size_t)b * Q + q] = total[q] + inc - v;
            total[q] += __shfl((unsigned long long)inc, 63, 64);
        }
    }
}

// The same quantities scanned inside the workgroup, in two steps with the kernel's own `if (i >= n) return;` between them where it has
// one.  First the wave scans and the waves' totals into LDS, up to the barrier: inc[q] = the wave's inclusive scan of v[q].
template <size_t Q, size_t WAVES>
__device__ __forceinline__ void place_wave_scan(const uint64_t (&v)[Q], uint64_t (&part)[WAVES][Q], uint64_t (&inc)[Q]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < (int)Q; ++q) inc[q] = wave_inclusive(v[q], lane);
    if (lane == 63) {
#pragma unroll
        for (int q = 0; q < (int)Q; ++q) part[wave][q] = inc[q];
    }
    __syncthreads();
}

// then before[q] = what the blocks before, the waves before and the lanes before add up to.  A scan, so places follow input order.
template <size_t Q, size_t WAVES>
__device__ __forceinline__ void place_before(const uint64_t (&v)[Q], const uint64_t (&inc)[Q], const uint64_t (&part)[WAVES][Q],
                                             const uint64_t* __restrict__ sums, uint64_t (&before)[Q]) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < (int)Q; ++q) before[q] = sums[(size_t)blockIdx.x * Q + q] + inc[q] - v[q];
    for (int w = 0; w < (int)WAVES; ++w) {
        if (w >= wave) break;
#pragma unroll
        for (int q = 0; q < (int)Q; ++q) before[q] += part[w][q];
    }
}

// ---- the byte layout of an output buffer (Q = 2: q = 0 the bytes, q = 1 the count of accepted items) -----------------------------------
// `Totals` has accepted, refused and out_bytes.  The totals as they stand when every item fits:
template <class Totals>
__device__ __forceinline__ void place_totals(Totals* __restrict__ totals, uint32_t n, const uint64_t (&total)[2]) {
    totals->accepted = total[1];
    totals->refused = n - total[1];
    totals->out_bytes = total[0];
}

// The SPACE rule of an accepted item of `bytes` bytes at `at` with `ahead` accepted items in front of it: true where it lies inside
// out_len.  Offsets only grow: the items in front of the one that straddles out_len fit, it and all behind it do not, so that one
// corrects the totals' counts.
template <class Totals>
__device__ __forceinline__ bool place_fits(uint64_t at, uint64_t bytes, uint64_t out_len, uint64_t ahead, uint32_t n, Totals* __restrict__ totals) {
    if (in_range(at, bytes, out_len)) return true;
    if (at <= out_len) {
        totals->accepted = ahead;
        totals->refused = n - ahead;
    }
    return false;
}

}  // namespace
}  // namespace mldsa_rec
