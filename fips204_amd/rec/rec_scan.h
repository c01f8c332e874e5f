// The device code the record libraries share (libmldsa_rec.so, libmldsa_recsign.so): the three kernels of the plan -- classify, offsets,
// apply: a stable exclusive scan of ten quantities per op.  The wave's scan and the wave's copy of an unaligned field, which the
// certificate layers take as well, are in rec_wave.h.
// Each library instantiates the kernels on its descriptor type `Op` (which has msg_len and ctx_len) and, for k_classify, on its `Check`:
// a small struct passed by value that holds what a descriptor is checked against and whose __device__ call operator returns the
// descriptor's class.  k_pack and k_scatter are each library's own and stay in its .hip file (../layer/layer_dev.h).
//
// Everything here has internal linkage (the unnamed namespace).  Both libraries are loaded into one process: a kernel template with
// external linkage would give each of them a weak host stub of one name, the loader would bind both to one address, and the second
// library's kernel registration would alias the first's (../layer/layer_host.h tells the same of its error slot).
//
// The rule of ../layer/layer_dev.h holds: a piece is shared only if every kernel that uses it compiles to the same instructions as
// with the piece written out.  All of these passed in both libraries; libmldsa_recsign.so's k_classify has three independent constant
// moves of its prologue in another order, nothing else (DESIGN.md has the table of the ten kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rec_plan.h"
#include "rec_wave.h"

namespace mldsa_rec {
namespace {

constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr uint32_t SLOT_MASK = (1u << 30) - 1;

// the ten scanned quantities of one op: v[c] = 1 for its class, v[4 + c] / v[7 + c] = its message / context bytes if it is accepted
__device__ __forceinline__ void op_values(int cls, uint32_t msg_len, uint32_t ctx_len, uint64_t (&v)[SCAN_VALUES]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = cls == c ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[4 + c] = cls == c ? msg_len : 0;
        v[7 + c] = cls == c ? ctx_len : 0;
    }
}

// one op per thread, SCAN_BLOCK per workgroup: check(descriptor) gives the op's class; the workgroup's ten sums go to sums[block]
template <class Op, class Check>
__global__ __launch_bounds__(SCAN_BLOCK) void k_classify(const Op* __restrict__ ops, uint32_t n, Check check, uint32_t* __restrict__ class_slot,
                                                         uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[SCAN_WAVES][SCAN_VALUES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int cls = -1;  // no op: counted nowhere
    uint32_t msg_len = 0, ctx_len = 0;
    if (i < n) {
        const Op d = ops[i];
        cls = check(d);
        msg_len = d.msg_len;
        ctx_len = d.ctx_len;
        class_slot[i] = (uint32_t)cls << 30;
    }
    uint64_t v[SCAN_VALUES];
    op_values(cls, msg_len, ctx_len, v);
#pragma unroll
    for (int q = 0; q < (int)SCAN_VALUES; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor((unsigned long long)v[q], d, 64);
        if (lane == 0) part[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < SCAN_VALUES) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < SCAN_WAVES; ++w) s += part[w][threadIdx.x];
        sums[(size_t)blockIdx.x * SCAN_VALUES + threadIdx.x] = s;
    }
}

// one wave per scanned quantity q (ten workgroups of one wave, each on its own column): sums[b][q] -> the sum over the blocks before b
// (in place); totals[q] = the sum over all blocks
__global__ __launch_bounds__(64) void k_offsets(uint64_t* __restrict__ sums, uint32_t n_blocks, uint64_t* __restrict__ totals) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 64) {
        const uint32_t b = base + lane;
        const uint64_t v = b < n_blocks ? sums[(size_t)b * SCAN_VALUES + q] : 0;
        const uint64_t inc = wave_inclusive(v, lane);
        if (b < n_blocks) sums[(size_t)b * SCAN_VALUES + q] = carry + inc - v;
        carry += __shfl((unsigned long long)inc, 63, 64);
    }
    if (lane == 0) totals[q] = carry;
}

// the same ten quantities scanned inside the workgroup (wave scans, then the waves' totals through LDS): slot, message position and
// context position of every op within its class.  A scan, so slots follow input order.
template <class Op>
__global__ __launch_bounds__(SCAN_BLOCK) void k_apply(const Op* __restrict__ ops, uint32_t n, const uint64_t* __restrict__ sums,
                                                      uint32_t* __restrict__ class_slot, uint64_t* __restrict__ msg_pos,
                                                      uint64_t* __restrict__ ctx_pos) {
    __shared__ uint64_t part[SCAN_WAVES][SCAN_VALUES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int cls = -1;
    uint32_t msg_len = 0, ctx_len = 0;
    if (i < n) {
        cls = (int)(class_slot[i] >> 30);  // k_classify's verdict on this descriptor
        if (cls != CLASS_REFUSED) {        // lengths only: no offset of the descriptor is followed here
            msg_len = ops[i].msg_len;
            ctx_len = ops[i].ctx_len;
        }
    }
    uint64_t v[SCAN_VALUES], before[SCAN_VALUES];
    op_values(cls, msg_len, ctx_len, v);
#pragma unroll
    for (int q = 0; q < (int)SCAN_VALUES; ++q) {
        const uint64_t inc = wave_inclusive(v[q], lane);
        before[q] = inc - v[q];
        if (lane == 63) part[wave][q] = inc;
    }
    __syncthreads();
    if (i >= n) return;
    // the three quantities of the op's own class: what the blocks before, the waves before and the lanes before add up to
    uint64_t slot = 0, mp = 0, cp = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (cls != c) continue;
        const uint64_t* base = sums + (size_t)blockIdx.x * SCAN_VALUES;
        slot = base[c] + before[c];
        if (c < 3) {
            mp = base[4 + c] + before[4 + c];
            cp = base[7 + c] + before[7 + c];
        }
        for (int w = 0; w < SCAN_WAVES; ++w) {
            if (w >= wave) break;
            slot += part[w][c];
            if (c < 3) {
                mp += part[w][4 + c];
                cp += part[w][7 + c];
            }
        }
    }
    class_slot[i] = ((uint32_t)cls << 30) | ((uint32_t)slot & SLOT_MASK);
    msg_pos[i] = mp;
    ctx_pos[i] = cp;
}

}  // namespace
}  // namespace mldsa_rec
