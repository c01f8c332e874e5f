// The two wave-level helpers that more libraries than the record pair take: the wave's inclusive scan of a 64-bit quantity and the wave's
// copy of an unaligned field by the copy plan of rec_plan.h.  rec_scan.h builds the record libraries' class scan on them; rec_place.h
// builds the placement scan of libmldsa_x509sign.so, libmldsa_csr.so and libmldsa_crl.so on the first, and the frame and TBS writers of
// the first two call the second.  No kernel here: a library that includes this header compiles none it does not launch.
//
// Everything here has internal linkage (the unnamed namespace), for the reason rec_scan.h and ../layer/layer_host.h give.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rec_plan.h"

namespace mldsa_rec {
namespace {

__device__ __forceinline__ uint64_t wave_inclusive(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// ---- the copy ---------------------------------------------------------------------------------------------------------------------------
// `len` bytes from offset `off` of a window of `window_len` bytes (the range lies inside it: the range check passed) to dst, by the
// whole wave.  The window is the blob for a field of a record, a class's sigs array for libmldsa_recsign.so's scatter.  `base` is the
// window's address rounded down to 16 and mis = window - base: the frame of rec_plan.h.  Every wide load lies inside the window, every
// wide store inside [dst, dst + len).
__device__ __forceinline__ void copy_field(const uint8_t* __restrict__ base, uint32_t mis, uint64_t window_len, uint64_t off, uint32_t len,
                                           uint8_t* __restrict__ dst, int lane) {
    const uint64_t src = mis + off;
    const CopyPlan p = copy_plan(src, len, (uint64_t)(uintptr_t)dst, mis, mis + window_len);
    for (uint32_t b = lane; b < p.head; b += 64) dst[b] = base[src + b];
    uint8_t* body = dst + p.head;
#pragma unroll 2
    for (uint64_t c = lane; c < p.body; c += 64) {
        const uint64_t at = chunk_src(p, src, c);
        const uint4 lo = *reinterpret_cast<const uint4*>(base + at);
        uint4 hi = make_uint4(0, 0, 0, 0);
        if (p.shift != 0) hi = *reinterpret_cast<const uint4*>(base + at + 16);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t o[4];
        funnel16(w, p.shift, o);
        *reinterpret_cast<uint4*>(body + 16 * c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    const uint64_t done = p.head + 16 * p.body;
    for (uint32_t b = lane; b < p.tail; b += 64) dst[done + b] = base[src + done + b];
}

}  // namespace
}  // namespace mldsa_rec
