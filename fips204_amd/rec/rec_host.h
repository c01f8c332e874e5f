// The host code the record libraries share (libmldsa_rec.so, libmldsa_recsign.so) around the plan of rec_scan.h: the layouts of the
// plan's working memory and of what a whole pass keeps in front of its arena, the check of a caller's plan memory, the plan's three
// launches, and the whole pass's one wait for the totals.  The arenas differ: arena_layout, the pack, the scatter and the entry points
// are each library's own.  The totals and info types are template arguments (mldsa_rec_totals / mldsa_recsign_totals, the two
// *_info); `fn` is the entry point's name and `lib` the library's prefix ("mldsa_rec", "mldsa_recsign"), for the messages.
// Internal linkage throughout, as ../layer/layer_host.h: each library gets its own copy.
#pragma once
#include "../layer/layer_host.h"
#include "rec_scan.h"

namespace mldsa_rec {
namespace {

using namespace mldsa_layer;

constexpr size_t MAX_OPS = (size_t)1 << 30;  // MLDSA_REC_MAX_OPS, MLDSA_RECSIGN_MAX_OPS

// ---- the layouts ------------------------------------------------------------------------------------------------------------------------
struct PlanLayout {
    size_t n_blocks, sums, msg_pos, ctx_pos, bytes;
};

bool plan_layout(size_t n, PlanLayout* o) {
    if (n > MAX_OPS) return false;
    Taker t;
    t.round = 256;
    o->n_blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    o->sums = t.take(8 * SCAN_VALUES * o->n_blocks);
    o->msg_pos = t.take(8 * n);
    o->ctx_pos = t.take(8 * n);
    o->bytes = t.at;
    return true;
}

struct FrontLayout {
    size_t class_slot, totals, plan, bytes;
};

bool front_layout(size_t n, FrontLayout* o, PlanLayout* p) {
    if (!plan_layout(n, p)) return false;
    Taker t;
    t.round = 256;
    o->class_slot = t.take(4 * n);
    o->totals = t.take(8 * SCAN_VALUES);
    o->plan = t.take(p->bytes);
    o->bytes = t.at;
    return true;
}

// the bodies of the libraries' *_plan_bytes and *_front_bytes
size_t plan_bytes(size_t n_ops) {
    PlanLayout L;
    return plan_layout(n_ops, &L) ? L.bytes : 0;
}

size_t front_bytes(size_t n_ops) {
    FrontLayout F;
    PlanLayout L;
    return front_layout(n_ops, &F, &L) ? F.bytes : 0;
}

// the caller's plan memory holds the plan of n_ops <= MAX_OPS ops; *L = its layout
int check_plan_memory(const char* fn, const char* lib, const void* plan, size_t bytes, size_t n_ops, PlanLayout* L) {
    plan_layout(n_ops, L);
    if (!plan || !aligned(plan, 256) || bytes < L->bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": plan is NULL, not 256-byte aligned or smaller than " + lib + "_plan_bytes");
    return MLDSA_OK;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
// every check is the caller's: 1 <= n_ops <= MAX_OPS, the current device is the context's
template <class Op, class Check, class Totals>
int launch_plan(const char* fn, const Op* ops, size_t n_ops, Check check, uint32_t* class_slot, Totals* totals, void* plan, const PlanLayout& L,
                hipStream_t s) {
    static_assert(sizeof(Totals) == 8 * SCAN_VALUES, "k_offsets writes the totals as the ten sums in turn");
    uint8_t* base = static_cast<uint8_t*>(plan);
    uint64_t* sums = reinterpret_cast<uint64_t*>(base + L.sums);
    const uint32_t n = (uint32_t)n_ops, nb = (uint32_t)L.n_blocks;
    hipLaunchKernelGGL((k_classify<Op, Check>), dim3(nb), dim3(SCAN_BLOCK), 0, s, ops, n, check, class_slot, sums);
    hipLaunchKernelGGL(k_offsets, dim3(SCAN_VALUES), dim3(64), 0, s, sums, nb, reinterpret_cast<uint64_t*>(totals));
    hipLaunchKernelGGL(k_apply<Op>, dim3(nb), dim3(SCAN_BLOCK), 0, s, ops, n, sums, class_slot, reinterpret_cast<uint64_t*>(base + L.msg_pos),
                       reinterpret_cast<uint64_t*>(base + L.ctx_pos));
    LAYER_LAUNCHED("plan launch");
    return MLDSA_OK;
}

// ---- the totals -------------------------------------------------------------------------------------------------------------------------
// the totals describe n_ops ops and their byte counts are small enough to be added up (the first half of a library's arena_of)
template <class Totals>
bool totals_consistent(const Totals& t, size_t n_ops) {
    for (int c = 0; c < 4; ++c)
        if (t.n[c] > n_ops) return false;
    if (t.n[0] + t.n[1] + t.n[2] + t.n[3] != n_ops) return false;
    const uint64_t limit = (uint64_t)1 << 60;
    for (int c = 0; c < 3; ++c)
        if (t.msg_bytes[c] > limit || t.ctx_bytes[c] > limit) return false;
    return true;
}

uint64_t sum3(const uint64_t (&v)[3]) { return v[0] + v[1] + v[2]; }

// Behind launch_plan in a whole pass, the call's one host wait of its own: the arena depends on the mix.  *tot = the plan's totals;
// *A = their arena by arena_of, the library's (false when the totals do not describe n_ops ops); *info, if there is one, is filled.
// MLDSA_ERR_NOMEM, with nothing more launched, when the scratch behind its first front_bytes bytes does not hold the arena.
template <class Totals, class Arena, class ArenaOf, class Info>
int read_totals(const char* fn, const Totals* d_totals, size_t n_ops, ArenaOf arena_of, size_t front_bytes, size_t scratch_bytes, Totals* tot,
                Arena* A, Info* info, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(tot, d_totals, sizeof(*tot), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_failed(fn, "reading the totals", e);
    if (!arena_of(*tot, n_ops, A)) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": the plan's totals do not add up to n_ops");
    if (info) {
        for (int c = 0; c < 4; ++c) info->n[c] = tot->n[c];
        info->msg_bytes = sum3(tot->msg_bytes);
        info->ctx_bytes = sum3(tot->ctx_bytes);
        info->scratch_needed = front_bytes + A->bytes;
    }
    if (scratch_bytes - front_bytes < A->bytes)
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch holds " + std::to_string(scratch_bytes) + " bytes, this mix needs " +
                                         std::to_string(front_bytes + A->bytes));
    return MLDSA_OK;
}

}  // namespace
}  // namespace mldsa_rec
