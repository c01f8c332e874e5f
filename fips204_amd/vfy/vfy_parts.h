// The part plan and the scratch carve of mldsa_vfy_verify as pure host code (no HIP here: tests/cpp/vfy_parts_main.cpp compiles it
// alone, under the sanitizers).  A call of n_ops ops is cut into parts of `part` ops (the last one may be shorter); part i writes its
// A_hat into half i & 1 of a two-part ring, everything else is one row per op of the call.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mldsa_vfy {

constexpr size_t PACKED_POLY_BYTES = 768;  // the core's 24-bit A_hat row (field.h PACKED_POLY_DWORDS)
constexpr size_t CARVE_ALIGN = 256;

struct Part {
    size_t first = 0, count = 0;  // ops [first, first + count) of the call
    int half = 0;                 // the ring half its A_hat lives in
};

// PartPlan plan(n_ops, part); for (i < plan.n_parts()) plan.at(i)  -- every op in exactly one part, in order; none for an empty call
struct PartPlan {
    size_t n_ops, part;
    PartPlan(size_t n_ops_, size_t part_) : n_ops(n_ops_), part(part_ ? part_ : 1) {}
    size_t n_parts() const { return n_ops / part + (n_ops % part ? 1 : 0); }
    // ring halves in use: a call of one part needs one
    size_t halves() const { return n_parts() > 1 ? 2 : n_parts(); }
    // ops a ring half holds
    size_t half_ops() const { return n_ops < part ? n_ops : part; }
    Part at(size_t i) const {
        Part p;
        p.first = i * part;
        p.count = n_ops - p.first < part ? n_ops - p.first : part;
        p.half = (int)(i & 1);
        return p;
    }
};

// byte offsets into a CARVE_ALIGN-aligned scratch; every array starts CARVE_ALIGN-aligned
struct Carve {
    size_t ring[2];  // A_hat of a part: half_ops * k * l packed rows (ring[1] == ring[0] when the call is one part)
    size_t ring_bytes;
    size_t c;        // c as one byte per coefficient: 256 bytes per op
    size_t znorm, hvalid, ctx_bad, key_bad, kidx;  // one dword per op
    size_t mu_w1;    // rows of mu | w1: 64 + w1_len bytes per op
    size_t bytes;    // the whole scratch
};

inline size_t carve_up(size_t x) { return (x + CARVE_ALIGN - 1) / CARVE_ALIGN * CARVE_ALIGN; }

inline Carve carve(int k, int l, size_t w1_len, const PartPlan& plan) {
    Carve c;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += carve_up(bytes);
        return here;
    };
    c.ring_bytes = plan.half_ops() * (size_t)(k * l) * PACKED_POLY_BYTES;
    c.ring[0] = take(c.ring_bytes);
    c.ring[1] = plan.halves() > 1 ? take(c.ring_bytes) : c.ring[0];
    c.c = take(plan.n_ops * 256);
    c.znorm = take(plan.n_ops * 4);
    c.hvalid = take(plan.n_ops * 4);
    c.ctx_bad = take(plan.n_ops * 4);
    c.key_bad = take(plan.n_ops * 4);
    c.kidx = take(plan.n_ops * 4);
    c.mu_w1 = take(plan.n_ops * (64 + w1_len));
    c.bytes = at + CARVE_ALIGN;  // (the slack of the core's own carve, pipeline.hip VerifyWs)
    return c;
}

}  // namespace mldsa_vfy
