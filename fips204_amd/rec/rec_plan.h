// The pure arithmetic of libmldsa_rec.so (include/mldsa_rec.h): the range check and classification of an untrusted descriptor, and the
// copy plan that moves an unaligned field of the blob to its packed place.  No HIP here: every function is constexpr, so the kernels of
// rec.hip call these very functions and tests/cpp/rec_plan_main.cpp compiles the file alone, under the sanitizers, and replays the plan on
// host memory.
//
// Coordinates of the copy plan.  Positions are byte positions in a frame whose 0 is 16-byte aligned: the blob's address rounded down to 16.
// The blob occupies the window [lo, hi) = [mis, mis + blob_len) of that frame, mis = blob & 15, and a field at blob offset `off` lies at
// src = mis + off.  Of the destination only its address mod 16 matters.  The plan copies len bytes in three pieces:
//   head   bytes [0, head), one by one: up to the first 16-byte boundary of the destination (+ 16 where the first wide load would
//          begin below lo);
//   body   `body` chunks of 16 bytes to 16-byte aligned destinations.  Chunk c takes the aligned 16-byte load at chunk_src(p, src, c)
//          and, when shift != 0, the next one, and funnel-shifts the 32 bytes right by `shift` bytes: shift = (src - dst) & 15 is the
//          difference between the two alignments and the same for every chunk.  Every such load lies inside [lo, hi): the last chunk is
//          left to the tail where its second load would end above hi;
//   tail   the remaining bytes [head + 16 body, len), one by one.
// head and tail are at most 31 bytes each.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mldsa_rec {

// ---- the descriptor's range check ---------------------------------------------------------------------------------------------------
// [off, off + len) inside [0, blob_len), safe against 64-bit wrap: nothing is added before it is known to fit.  An empty range is
// accepted wherever off <= blob_len.
constexpr bool in_range(uint64_t off, uint64_t len, uint64_t blob_len) { return off <= blob_len && len <= blob_len - off; }

constexpr int CLASS_44 = 0, CLASS_65 = 1, CLASS_87 = 2, CLASS_REFUSED = 3;
constexpr uint32_t pk_len(int c) { return c == CLASS_44 ? 1312 : c == CLASS_65 ? 1952 : 2592; }
constexpr uint32_t sig_len(int c) { return c == CLASS_44 ? 2420 : c == CLASS_65 ? 3309 : 4627; }
constexpr int set_of_class(int c) { return c == CLASS_44 ? 44 : c == CLASS_65 ? 65 : 87; }
constexpr uint32_t CTX_MAX = 255;  // the core's rule

constexpr int class_of_set(uint32_t set) { return set == 44 ? CLASS_44 : set == 65 ? CLASS_65 : set == 87 ? CLASS_87 : CLASS_REFUSED; }

// The class of an op from the fields of its descriptor: refused for an unknown set, a nonzero reserved byte, a context longer than 255
// bytes, or any of the four ranges not inside the blob.
constexpr int classify(uint64_t pk_off, uint64_t sig_off, uint64_t msg_off, uint64_t ctx_off, uint32_t msg_len, uint32_t ctx_len,
                       uint32_t set, uint32_t reserved, uint64_t blob_len) {
    const int c = class_of_set(set);
    if (c == CLASS_REFUSED || reserved != 0 || ctx_len > CTX_MAX) return CLASS_REFUSED;
    if (!in_range(pk_off, pk_len(c), blob_len) || !in_range(sig_off, sig_len(c), blob_len)) return CLASS_REFUSED;
    if (!in_range(msg_off, msg_len, blob_len) || !in_range(ctx_off, ctx_len, blob_len)) return CLASS_REFUSED;
    return c;
}

// ---- the copy plan ------------------------------------------------------------------------------------------------------------------
struct CopyPlan {
    uint32_t head = 0;   // bytes copied one by one in front
    uint32_t shift = 0;  // bytes the body's 32-byte windows are shifted right by, 0 ... 15
    uint64_t body = 0;   // 16-byte chunks
    uint32_t tail = 0;   // bytes copied one by one behind
};

// The caller vouches for lo <= src and src + len <= hi (the range check passed).
constexpr CopyPlan copy_plan(uint64_t src, uint64_t len, uint64_t dst, uint64_t lo, uint64_t hi) {
    CopyPlan p;
    p.shift = (uint32_t)((src - dst) & 15);
    uint64_t head = (0 - dst) & 15;
    if (head > len) head = len;
    // the first wide load begins at src + head - shift: below the window -> one more chunk's worth goes byte by byte
    if (p.shift != 0 && len - head >= 16 && src + head < lo + p.shift) head += 16;
    uint64_t body = (len - head) / 16;
    // with a shift the last chunk's second load ends 16 - shift bytes behind the chunk's last source byte
    if (p.shift != 0 && body != 0 && src + head + 16 * body + (16 - p.shift) > hi) body -= 1;
    p.head = (uint32_t)head;
    p.body = body;
    p.tail = (uint32_t)(len - head - 16 * body);
    return p;
}

// position of chunk c's first 16-byte load (a multiple of 16); with shift != 0 the second load is at + 16
constexpr uint64_t chunk_src(const CopyPlan& p, uint64_t src, uint64_t c) { return src + p.head + 16 * c - p.shift; }

// the eight dwords w[0 ... 7] of two consecutive aligned loads, shifted right by `shift` bytes (little endian): the four dwords out
constexpr uint32_t funnel(uint32_t a, uint32_t b, uint32_t bits) { return bits ? (a >> bits) | (b << (32 - bits)) : a; }

template <int DS>
constexpr void funnel_at(const uint32_t (&w)[8], uint32_t bits, uint32_t (&out)[4]) {
    out[0] = funnel(w[DS], w[DS + 1], bits);
    out[1] = funnel(w[DS + 1], w[DS + 2], bits);
    out[2] = funnel(w[DS + 2], w[DS + 3], bits);
    out[3] = funnel(w[DS + 3], w[DS + 4], bits);
}

constexpr void funnel16(const uint32_t (&w)[8], uint32_t shift, uint32_t (&out)[4]) {
    const uint32_t bits = (shift & 3) * 8;
    switch (shift >> 2) {  // constant indices in every arm: the dwords stay in registers
        case 0: funnel_at<0>(w, bits, out); break;
        case 1: funnel_at<1>(w, bits, out); break;
        case 2: funnel_at<2>(w, bits, out); break;
        default: funnel_at<3>(w, bits, out); break;
    }
}

// ---- the scratch formulas (include/mldsa_rec.h spells them out) -----------------------------------------------------------------------
constexpr size_t SCAN_BLOCK = 256;   // MLDSA_REC_SCAN_BLOCK
constexpr size_t SCAN_VALUES = 10;   // per block: the four class counts, message bytes and context bytes of the three accepted classes
constexpr size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// The working memory of the placement scan (rec_place.h) over n items in workgroups of `block`: `q` 64-bit sums per workgroup, and for
// the two libraries that lay out an output buffer (q = PLACE_SUMS) one 32-bit length per item behind them; 0 past the library's cap.
constexpr size_t PLACE_SUMS = 2;  // the workgroup's sum of output lengths and its count of accepted items
constexpr size_t scan_blocks(size_t n, size_t block) { return (n + block - 1) / block; }
constexpr size_t place_sums_bytes(size_t n, size_t block, size_t q) { return up256(8 * q * scan_blocks(n, block)); }
constexpr size_t place_plan_bytes(size_t n, size_t block, size_t cap) {
    return n > cap ? 0 : place_sums_bytes(n, block, PLACE_SUMS) + up256(4 * n);
}

}  // namespace mldsa_rec
