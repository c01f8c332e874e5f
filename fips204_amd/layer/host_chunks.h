// The chunk plan of the host-memory feed (host_feed.h: mldsa_hash_*_host, mldsa_mus_host_compute) as pure host code (no HIP here:
// tests/cpp/host_chunks_main.cpp compiles it alone, under the sanitizers).  The bytes [off[0], off[n_ops]) of a batch of messages are cut
// into chunks of at most `staging` bytes at arbitrary byte positions; a message may span any number of chunks and a chunk may hold any
// number of messages.  For every chunk the plan gives the byte range, the range of ops that have bytes in it, and -- piece_lo / piece_hi,
// the two functions mus's update kernels apply to the one offset table of the call -- where each of those ops' bytes lie in the chunk.
// `off` is a table that mldsa_check_offsets has accepted: n_ops + 1 non-decreasing offsets.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mldsa_layer {

// The bytes of the pair [p0, p1) that fall into the window [win_lo, win_hi) are [piece_lo(p0, win_lo), piece_hi(p1, win_hi)), if that
// is not empty.  (constexpr: the kernels call the same two functions.)
constexpr uint64_t piece_lo(uint64_t p0, uint64_t win_lo) { return p0 > win_lo ? p0 : win_lo; }
constexpr uint64_t piece_hi(uint64_t p1, uint64_t win_hi) { return p1 < win_hi ? p1 : win_hi; }

struct Chunk {
    uint64_t lo = 0, hi = 0;     // the chunk's bytes [lo, hi) of the batch, 0 < hi - lo <= staging
    size_t first = 0, last = 0;  // ops [first, last): `first` and `last - 1` have bytes in the chunk, and no op outside the range has
};

// offset of boundary i (first <= i <= last) inside the chunk: the chunk's piece of op i is [rel(i), rel(i + 1)) of its bytes
inline uint64_t piece_off_in_chunk(const uint64_t* off, size_t i, const Chunk& c) { return piece_hi(piece_lo(off[i], c.lo), c.hi) - c.lo; }

// ChunkPlan plan(off, n_ops, staging); Chunk c; while (plan.next(&c)) ...   -- the chunks in order; none for an empty batch
class ChunkPlan {
public:
    ChunkPlan(const uint64_t* off, size_t n_ops, uint64_t staging)
        : off_(off), n_ops_(n_ops), staging_(staging), at_(n_ops ? off[0] : 0), end_(n_ops ? off[n_ops] : 0) {}

    bool next(Chunk* c) {
        if (staging_ == 0 || at_ >= end_) return false;
        c->lo = at_;
        c->hi = end_ - at_ <= staging_ ? end_ : at_ + staging_;
        // ops before `first_` end at or before the chunk's start (an empty message on the boundary among them): no bytes here
        while (first_ < n_ops_ && off_[first_ + 1] <= c->lo) first_++;
        c->first = first_;
        // the first op at or after first_ that starts at or behind the chunk's end: binary search, the table is non-decreasing
        size_t a = first_, b = n_ops_;
        while (a < b) {
            const size_t mid = a + (b - a) / 2;
            if (off_[mid] < c->hi) a = mid + 1;
            else b = mid;
        }
        c->last = a;
        at_ = c->hi;
        return true;
    }

private:
    const uint64_t* off_;
    size_t n_ops_;
    uint64_t staging_, at_, end_;
    size_t first_ = 0;
};

}  // namespace mldsa_layer
