// The pure arithmetic of libmldsa_recsign.so (include/mldsa_recsign.h): the refusal rules of an untrusted signing descriptor, as one
// constexpr function.  No HIP here: the kernels of recsign.hip call this very function and tests/cpp/recsign_plan_main.cpp compiles the
// file alone, under the sanitizers.  The range check, the copy plan, the funnel shift, the lengths and the classes are those of
// ../rec/rec_plan.h, included and not copied.
//
// The copy plan serves both directions.  k_pack moves a field of the blob to its packed place, as libmldsa_rec.so does: the window is
// the blob.  k_scatter moves a row of a class's dense sigs array to its hole in `out`: the window [lo, hi) is that array, n_c * SIG_LEN
// bytes, the source is lo + slot * SIG_LEN, and of the destination out + sig_off only the address mod 16 enters the plan.  The body's
// 16-byte stores begin at the destination's first 16-byte boundary and end at most at its last byte, so they lie wholly inside the hole;
// head and tail go byte by byte.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../rec/rec_plan.h"

namespace mldsa_recsign {

using mldsa_rec::CLASS_44;
using mldsa_rec::CLASS_65;
using mldsa_rec::CLASS_87;
using mldsa_rec::CLASS_REFUSED;
using mldsa_rec::class_of_set;
using mldsa_rec::chunk_src;
using mldsa_rec::copy_plan;
using mldsa_rec::CopyPlan;
using mldsa_rec::CTX_MAX;
using mldsa_rec::funnel16;
using mldsa_rec::in_range;
using mldsa_rec::SCAN_BLOCK;
using mldsa_rec::SCAN_VALUES;
using mldsa_rec::set_of_class;
using mldsa_rec::sig_len;
using mldsa_rec::up256;

constexpr uint32_t FLAG_RND = 1;  // MLDSA_RECSIGN_RND: the op's 32 bytes of randomness lie at rnd_off
constexpr uint32_t RND_LEN = 32;
// the status codes of include/mldsa_hip.h (recsign.hip asserts the equality)
constexpr int ST_OK = 0, ST_PARAM = -1, ST_CTX_LEN = -2;

struct Verdict {
    int cls = CLASS_REFUSED;  // CLASS_44 / _65 / _87 of an accepted op
    int status = ST_PARAM;    // ST_OK for an accepted op, else the refusal's code
};

// The refusal rules, tested in the order the header states them.  n_keys: the rows of the three key tables in class order; a set
// with no keys is not served, so every key of it is out of range.
constexpr Verdict check_op(uint64_t msg_off, uint64_t ctx_off, uint64_t rnd_off, uint64_t sig_off, uint32_t msg_len, uint32_t key,
                           uint32_t ctx_len, uint32_t set, uint32_t flags, uint32_t reserved, uint64_t blob_len, uint64_t out_len,
                           uint64_t n_keys_44, uint64_t n_keys_65, uint64_t n_keys_87) {
    Verdict v;
    const int c = class_of_set(set);
    if (c == CLASS_REFUSED || (flags & ~FLAG_RND) != 0 || reserved != 0) return v;  // 1
    if (ctx_len > CTX_MAX) {                                                         // 2
        v.status = ST_CTX_LEN;
        return v;
    }
    const uint64_t n_keys = c == CLASS_44 ? n_keys_44 : c == CLASS_65 ? n_keys_65 : n_keys_87;
    if (key >= n_keys) return v;                                                                // 3
    if (!in_range(msg_off, msg_len, blob_len) || !in_range(ctx_off, ctx_len, blob_len)) return v;  // 4
    if ((flags & FLAG_RND) != 0 && !in_range(rnd_off, RND_LEN, blob_len)) return v;
    if (!in_range(sig_off, sig_len(c), out_len)) return v;                                      // 5
    v.cls = c;
    v.status = ST_OK;
    return v;
}

}  // namespace mldsa_recsign
