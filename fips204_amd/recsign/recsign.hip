// libmldsa_recsign.so (include/mldsa_recsign.h): batched signing of serialized request records -- a blob and one descriptor per op, any
// mix of parameter sets -- by sorting the ops by set and packing each set's dense arrays on the device in front of the core's signing
// call, and by writing every signature to its byte offset in the output buffer behind it.
//
// The phases are separate launches and the kernel boundaries do all the ordering: no wave waits for another workgroup.
//   the plan    k_classify, k_offsets, k_apply of ../rec/rec_scan.h, shared with libmldsa_rec.so: the descriptor's check
//               (recsign_plan.h) gives the op's class, a stable scan its slot, message position and context position within the class,
//               and the totals.
//   k_pack      one wave per op: message, context and rnd copied to their places by the copy plan of ../rec/rec_plan.h (copy_field of
//               ../rec/rec_scan.h) -- aligned 16-byte loads, funnel-shifted in registers by the difference of the two alignments, aligned
//               16-byte stores, single bytes at the ends --, zeros for an op without rnd, key_idx[slot] = key.
//   k_scatter   one wave per op: the op's row of its class's sigs to out + sig_off by the same plan (the window is the sigs array),
//               status[i] = the class's status[slot]; the refusal's code, and nothing else, for a refused op.
// What bounds them: k_pack reads and writes |M| + |ctx| + 32 bytes once per op and k_scatter SIG_LEN (with a shift every 16-byte source
// chunk is loaded by two neighbouring lanes; the second comes from L1 / L2); the plan reads the 48-byte descriptors twice, pack and
// scatter once each.
// Here: the descriptor's adaptor, the pack, the scatter, the arena, pack_sign_scatter, the clearing of rnd and the entry points.  The
// plan's layouts, its launches and the wait for the totals are ../rec/rec_host.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_recsign.h"
#include "../layer/layer_host.h"
#include "../rec/rec_host.h"
#include "../rec/rec_scan.h"
#include "recsign_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_rec;  // the shared plan: rec_scan.h, rec_host.h
using namespace mldsa_recsign;

static_assert(sizeof(mldsa_recsign_op) == 48 && sizeof(mldsa_recsign_totals) == 8 * SCAN_VALUES, "the layouts of include/mldsa_recsign.h");
static_assert(SCAN_BLOCK == MLDSA_RECSIGN_SCAN_BLOCK && SCAN_BLOCK % 64 == 0 && MAX_OPS == MLDSA_RECSIGN_MAX_OPS,
              "the caps of include/mldsa_recsign.h");
static_assert(CLASS_44 == MLDSA_RECSIGN_CLASS_44 && CLASS_65 == MLDSA_RECSIGN_CLASS_65 && CLASS_87 == MLDSA_RECSIGN_CLASS_87 &&
                  CLASS_REFUSED == MLDSA_RECSIGN_CLASS_REFUSED, "the classes of include/mldsa_recsign.h");
static_assert(ST_OK == MLDSA_OK && ST_PARAM == MLDSA_ERR_PARAM && ST_CTX_LEN == MLDSA_ERR_CTX_LEN && FLAG_RND == MLDSA_RECSIGN_RND,
              "the codes of include/mldsa_hip.h and the flag of include/mldsa_recsign.h");

constexpr int OP_WAVES = 4;  // ops per workgroup of k_pack and k_scatter

// what a descriptor is checked against: the two buffer lengths and the rows of the three key tables
struct Limits {
    uint64_t blob_len, out_len;
    uint32_t n_keys[3];
};

__device__ __forceinline__ Verdict check(const mldsa_recsign_op& d, const Limits& L) {
    return check_op(d.msg_off, d.ctx_off, d.rnd_off, d.sig_off, d.msg_len, d.key, d.ctx_len, d.set, d.flags, d.reserved, L.blob_len, L.out_len,
                    L.n_keys[0], L.n_keys[1], L.n_keys[2]);
}

// k_classify's check
struct ClassOf {
    Limits L;
    __device__ int operator()(const mldsa_recsign_op& d) const { return check(d, L).cls; }
};

// the arrays of one class that k_pack fills
struct PackClass {
    uint32_t* key_idx;
    uint8_t *msgs, *ctxs, *rnd;
    uint64_t *msg_off, *ctx_off;
    uint64_t n, msg_bytes, ctx_bytes;
};
struct PackArgs {
    PackClass c[3];
};

__global__ __launch_bounds__(64 * OP_WAVES) void k_pack(const uint8_t* __restrict__ blob, const mldsa_recsign_op* __restrict__ ops, uint32_t n,
                                                        Limits L, const uint32_t* __restrict__ class_slot,
                                                        const uint64_t* __restrict__ msg_pos, const uint64_t* __restrict__ ctx_pos,
                                                        PackArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (blockIdx.x == 0 && threadIdx.x == c && a.c[c].n == 0) {  // an empty class: its tables' one entry
            a.c[c].msg_off[0] = 0;
            a.c[c].ctx_off[0] = 0;
        }
    }
    if (i >= n) return;
    const uint32_t cs = class_slot[i];
    const int cls = (int)(cs >> 30);
    if (cls == CLASS_REFUSED) return;
    const mldsa_recsign_op d = ops[i];
    // The descriptor is checked again and the plan's numbers against the counts the host passed: only then is an offset followed or a
    // row written.  (cls is wave-uniform: one op per wave.)
    if (check(d, L).cls != cls) return;
    PackClass k = a.c[0];  // (selected, not indexed: the arguments stay in scalar registers)
    if (cls == CLASS_65) k = a.c[1];
    if (cls == CLASS_87) k = a.c[2];
    const uint64_t slot = cs & SLOT_MASK, mp = msg_pos[i], cp = ctx_pos[i];
    if (slot >= k.n || !in_range(mp, d.msg_len, k.msg_bytes) || !in_range(cp, d.ctx_len, k.ctx_bytes)) return;
    const uint32_t mis = (uint32_t)((uintptr_t)blob & 15);
    const uint8_t* base = blob - mis;
    copy_field(base, mis, L.blob_len, d.msg_off, d.msg_len, k.msgs + mp, lane);
    copy_field(base, mis, L.blob_len, d.ctx_off, d.ctx_len, k.ctxs + cp, lane);
    uint8_t* rnd = k.rnd + slot * RND_LEN;
    if ((d.flags & FLAG_RND) != 0) {
        copy_field(base, mis, L.blob_len, d.rnd_off, RND_LEN, rnd, lane);
    } else if (lane < (int)(RND_LEN / 4)) {
        reinterpret_cast<uint32_t*>(rnd)[lane] = 0;  // the deterministic variant; rnd_off is not followed
    }
    if (lane == 0) {
        k.key_idx[slot] = d.key;
        k.msg_off[slot] = mp;
        k.ctx_off[slot] = cp;
        if (slot + 1 == k.n) {  // the class's last op closes its tables
            k.msg_off[k.n] = mp + d.msg_len;
            k.ctx_off[k.n] = cp + d.ctx_len;
        }
    }
}

struct ScatterArgs {
    const uint8_t* sigs[3];
    const int32_t* status[3];
    uint64_t n[3];
};

__global__ __launch_bounds__(64 * OP_WAVES) void k_scatter(const mldsa_recsign_op* __restrict__ ops, uint32_t n, Limits L,
                                                           const uint32_t* __restrict__ class_slot, ScatterArgs a, uint8_t* __restrict__ out,
                                                           int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const mldsa_recsign_op d = ops[i];
    const Verdict v = check(d, L);  // again: what is written, and where, rests on the descriptor as it reads now
    if (v.cls == CLASS_REFUSED) {
        if (lane == 0) status[i] = v.status;
        return;
    }
    const uint32_t cs = class_slot[i];
    const uint64_t slot = cs & SLOT_MASK;
    const uint8_t* sigs = a.sigs[0];
    const int32_t* st = a.status[0];
    uint64_t n_c = a.n[0];
    if (v.cls == CLASS_65) sigs = a.sigs[1], st = a.status[1], n_c = a.n[1];
    if (v.cls == CLASS_87) sigs = a.sigs[2], st = a.status[2], n_c = a.n[2];
    if ((int)(cs >> 30) != v.cls || slot >= n_c) {  // a plan that does not belong to these descriptors: nothing of it is followed
        if (lane == 0) status[i] = ST_PARAM;
        return;
    }
    const uint32_t len = sig_len(v.cls);
    const uint32_t mis = (uint32_t)((uintptr_t)sigs & 15);
    copy_field(sigs - mis, mis, n_c * len, slot * len, len, out + d.sig_off, lane);
    if (lane == 0) status[i] = st[slot];
}

// ------------------------------------------------------------------------------------------------------------ host side
// the arena: per class key_idx, msg_off, ctx_off, sigs, status; then the rnd rows of the three classes back to back (one region); then
// the messages and the contexts of the three classes back to back
struct ArenaLayout {
    size_t key_idx[3], msg_off[3], ctx_off[3], sigs[3], status[3], rnd, rnd_bytes, msgs, ctxs, bytes;
};

bool arena_layout(const uint64_t (&n)[3], uint64_t msg_bytes, uint64_t ctx_bytes, ArenaLayout* o) {
    const uint64_t limit = (uint64_t)1 << 62;  // nothing below overflows under it
    if (msg_bytes > limit || ctx_bytes > limit) return false;
    Taker t;
    t.round = 256;
    for (int c = 0; c < 3; ++c) {
        if (n[c] > MLDSA_RECSIGN_MAX_OPS) return false;
        o->key_idx[c] = t.take(4 * (size_t)n[c]);
        o->msg_off[c] = t.take(8 * ((size_t)n[c] + 1));
        o->ctx_off[c] = t.take(8 * ((size_t)n[c] + 1));
        o->sigs[c] = t.take((size_t)n[c] * sig_len(c));
        o->status[c] = t.take(4 * (size_t)n[c]);
    }
    o->rnd = t.take(RND_LEN * (size_t)(n[0] + n[1] + n[2]));
    o->rnd_bytes = t.at - o->rnd;
    o->msgs = t.take((size_t)msg_bytes);
    o->ctxs = t.take((size_t)ctx_bytes);
    o->bytes = t.at;
    return true;
}

// the checks the entry points share; the message names what failed.  *L is filled.
int check_call(const char* fn, const mldsa_ctx* ctx, uint64_t blob_len, uint64_t out_len, const mldsa_recsign_op* ops, size_t n_ops,
               const size_t* n_keys, Limits* L) {
    if (n_ops > MLDSA_RECSIGN_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_RECSIGN_MAX_OPS ops");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!ops || !n_keys) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(ops, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": ops must be 8-byte aligned");
    L->blob_len = blob_len;
    L->out_len = out_len;
    for (int c = 0; c < 3; ++c) {
        if (n_keys[c] > UINT32_MAX) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys above UINT32_MAX");
        L->n_keys[c] = (uint32_t)n_keys[c];
    }
    return MLDSA_OK;
}

// totals (host) are consistent with n_ops and the arena is large enough: the caller checked
int launch_pack(const char* fn, const uint8_t* blob, const mldsa_recsign_op* ops, size_t n_ops, const Limits& lim, const uint32_t* class_slot,
                const void* plan, const PlanLayout& L, const mldsa_recsign_totals& tot, void* arena, const ArenaLayout& A,
                mldsa_recsign_packed* out, hipStream_t s) {
    uint8_t* base = static_cast<uint8_t*>(arena);
    const uint8_t* pl = static_cast<const uint8_t*>(plan);
    PackArgs a;
    uint64_t m_at = 0, c_at = 0, r_at = 0;
    for (int c = 0; c < 3; ++c) {
        PackClass& k = a.c[c];
        k.key_idx = reinterpret_cast<uint32_t*>(base + A.key_idx[c]);
        k.msg_off = reinterpret_cast<uint64_t*>(base + A.msg_off[c]);
        k.ctx_off = reinterpret_cast<uint64_t*>(base + A.ctx_off[c]);
        k.rnd = base + A.rnd + r_at;
        k.msgs = base + A.msgs + m_at;
        k.ctxs = base + A.ctxs + c_at;
        k.n = tot.n[c];
        k.msg_bytes = tot.msg_bytes[c];
        k.ctx_bytes = tot.ctx_bytes[c];
        m_at += tot.msg_bytes[c];
        c_at += tot.ctx_bytes[c];
        r_at += RND_LEN * tot.n[c];
        mldsa_recsign_class& o = out->c[c];
        o.n = (size_t)k.n;
        o.key_idx = k.key_idx, o.msgs = k.msgs, o.ctxs = k.ctxs, o.rnd = k.rnd, o.msg_off = k.msg_off, o.ctx_off = k.ctx_off;
        o.sigs = base + A.sigs[c];
        o.status = reinterpret_cast<int32_t*>(base + A.status[c]);
    }
    out->rnd_region = base + A.rnd;
    out->rnd_region_bytes = A.rnd_bytes;
    const uint32_t n = (uint32_t)n_ops;
    hipLaunchKernelGGL(k_pack, dim3((n + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, s, blob, ops, n, lim, class_slot,
                       reinterpret_cast<const uint64_t*>(pl + L.msg_pos), reinterpret_cast<const uint64_t*>(pl + L.ctx_pos), a);
    LAYER_LAUNCHED("k_pack launch");
    return MLDSA_OK;
}

// the counts of `packed` are at most n_ops and its used pointers non-NULL: the caller checked
int launch_scatter(const char* fn, const mldsa_recsign_op* ops, size_t n_ops, const Limits& lim, const uint32_t* class_slot,
                   const mldsa_recsign_packed& P, uint8_t* out, int32_t* status, hipStream_t s) {
    ScatterArgs a;
    for (int c = 0; c < 3; ++c) {
        a.sigs[c] = P.c[c].sigs;
        a.status[c] = P.c[c].status;
        a.n[c] = P.c[c].n;
    }
    const uint32_t n = (uint32_t)n_ops;
    hipLaunchKernelGGL(k_scatter, dim3((n + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, s, ops, n, lim, class_slot, a, out, status);
    LAYER_LAUNCHED("k_scatter launch");
    return MLDSA_OK;
}

// the arena of the totals; false when they do not describe n_ops ops or the size does not fit
bool arena_of(const mldsa_recsign_totals& t, size_t n_ops, ArenaLayout* A) {
    const uint64_t n[3] = {t.n[0], t.n[1], t.n[2]};
    return totals_consistent(t, n_ops) && arena_layout(n, sum3(t.msg_bytes), sum3(t.ctx_bytes), A);
}

// steps 4 to 6 of the whole pass, behind the plan and the check of the scratch; *P is filled before anything is launched
int pack_sign_scatter(const char* fn, mldsa_ctx* ctx, int mode, const mldsa_recsign_keys* keys, const uint8_t* blob,
                      const mldsa_recsign_op* ops, size_t n_ops, const Limits& lim, const uint32_t* class_slot, const void* plan,
                      const PlanLayout& L, const mldsa_recsign_totals& tot, void* arena, const ArenaLayout& A, mldsa_recsign_packed* P,
                      uint8_t* out, int32_t* status, void* stream) {
    int rc = launch_pack(fn, blob, ops, n_ops, lim, class_slot, plan, L, tot, arena, A, P, (hipStream_t)stream);
    if (rc != MLDSA_OK) return rc;
    for (int c = 0; c < 3; ++c) {
        const mldsa_recsign_class& k = P->c[c];
        const mldsa_recsign_keys& t = keys[c];
        if (k.n == 0) continue;
        LAYER_CORE(mldsa_sign(ctx, set_of_class(c), mode, t.rho, t.cap_k, t.tr, t.s_1_hat_mont, t.s_2_hat_mont, t.t_0_hat_mont, t.n_keys, k.key_idx,
                              k.msgs, k.msg_off, k.ctxs, k.ctx_off, k.rnd, k.sigs, k.status, k.n, stream),
                   "the core's signing call");
    }
    return launch_scatter(fn, ops, n_ops, lim, class_slot, *P, out, status, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int mldsa_recsign_abi_version(void) { return MLDSA_RECSIGN_ABI_VERSION; }

const char* mldsa_recsign_last_error(void) { return g_err.c_str(); }

size_t mldsa_recsign_plan_bytes(size_t n_ops) { return plan_bytes(n_ops); }

size_t mldsa_recsign_front_bytes(size_t n_ops) { return front_bytes(n_ops); }

size_t mldsa_recsign_arena_bytes(size_t n44, size_t n65, size_t n87, uint64_t msg_bytes, uint64_t ctx_bytes) {
    ArenaLayout A;
    const uint64_t n[3] = {n44, n65, n87};
    return arena_layout(n, msg_bytes, ctx_bytes, &A) ? A.bytes : 0;
}

size_t mldsa_recsign_arena_bytes_max(size_t n_ops, uint64_t msg_bytes, uint64_t ctx_bytes) {
    if (n_ops > MLDSA_RECSIGN_MAX_OPS || msg_bytes > ((uint64_t)1 << 62) || ctx_bytes > ((uint64_t)1 << 62)) return 0;
    return 2 * up256(4 * n_ops) + 2 * up256(8 * n_ops + 24) + up256(n_ops * sig_len(CLASS_87)) + 5 * 512 + up256(RND_LEN * n_ops) +
           up256((size_t)msg_bytes) + up256((size_t)ctx_bytes);
}

int mldsa_recsign_plan(mldsa_ctx* ctx, uint64_t blob_len, uint64_t out_len, const mldsa_recsign_op* ops, size_t n_ops, const size_t* n_keys,
                       uint32_t* class_slot, mldsa_recsign_totals* totals, void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_recsign_plan";
    if (n_ops == 0) return MLDSA_OK;
    Limits lim;
    int rc = check_call(fn, ctx, blob_len, out_len, ops, n_ops, n_keys, &lim);
    if (rc != MLDSA_OK) return rc;
    PlanLayout L;
    if (!class_slot || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4) || !aligned(totals, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned, totals 8-byte aligned");
    rc = check_plan_memory(fn, "mldsa_recsign", plan, plan_bytes, n_ops, &L);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_plan(fn, ops, n_ops, ClassOf{lim}, class_slot, totals, plan, L, (hipStream_t)stream);
}

int mldsa_recsign_pack(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, uint64_t out_len, const mldsa_recsign_op* ops, size_t n_ops,
                       const size_t* n_keys, const uint32_t* class_slot, const void* plan, size_t plan_bytes, const mldsa_recsign_totals* totals,
                       void* arena, size_t arena_bytes, mldsa_recsign_packed* packed, void* stream) {
    const char* fn = "mldsa_recsign_pack";
    if (n_ops == 0) {
        if (packed) memset(packed, 0, sizeof(*packed));
        return MLDSA_OK;
    }
    Limits lim;
    int rc = check_call(fn, ctx, blob_len, out_len, ops, n_ops, n_keys, &lim);
    if (rc != MLDSA_OK) return rc;
    if (!blob && blob_len != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    PlanLayout L;
    if (!class_slot || !totals || !packed) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned");
    rc = check_plan_memory(fn, "mldsa_recsign", plan, plan_bytes, n_ops, &L);
    if (rc != MLDSA_OK) return rc;
    ArenaLayout A;
    if (!arena_of(*totals, n_ops, &A)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": the totals do not describe n_ops ops");
    if (!arena || !aligned(arena, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": arena is NULL or not 256-byte aligned");
    if (arena_bytes < A.bytes) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": arena smaller than mldsa_recsign_arena_bytes of the totals");
    LAYER_ON_DEVICE(ctx);
    return launch_pack(fn, blob, ops, n_ops, lim, class_slot, plan, L, *totals, arena, A, packed, (hipStream_t)stream);
}

int mldsa_recsign_scatter(mldsa_ctx* ctx, const mldsa_recsign_op* ops, size_t n_ops, uint64_t blob_len, uint8_t* out, uint64_t out_len,
                          const size_t* n_keys, const uint32_t* class_slot, const mldsa_recsign_packed* packed, int32_t* status, void* stream) {
    const char* fn = "mldsa_recsign_scatter";
    if (n_ops == 0) return MLDSA_OK;
    Limits lim;
    const int rc = check_call(fn, ctx, blob_len, out_len, ops, n_ops, n_keys, &lim);
    if (rc != MLDSA_OK) return rc;
    if (!out || !class_slot || !packed || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4) || !aligned(status, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot and status must be 4-byte aligned");
    for (int c = 0; c < 3; ++c) {
        const mldsa_recsign_class& k = packed->c[c];
        if (k.n > n_ops || (k.n != 0 && (!k.sigs || !k.status || !aligned(k.status, 4))))
            return fail(MLDSA_ERR_PARAM, std::string(fn) + ": packed does not describe n_ops ops");
    }
    LAYER_ON_DEVICE(ctx);
    return launch_scatter(fn, ops, n_ops, lim, class_slot, *packed, out, status, (hipStream_t)stream);
}

int mldsa_recsign_sign(mldsa_ctx* ctx, int mode, const mldsa_recsign_keys* keys, const uint8_t* blob, uint64_t blob_len,
                       const mldsa_recsign_op* ops, size_t n_ops, uint8_t* out, uint64_t out_len, int32_t* status, void* scratch,
                       size_t scratch_bytes, mldsa_recsign_info* info, void* stream) {
    const char* fn = "mldsa_recsign_sign";
    if (n_ops == 0) return MLDSA_OK;
    size_t n_keys[3] = {0, 0, 0};
    for (int c = 0; keys && c < 3; ++c) n_keys[c] = keys[c].n_keys;
    Limits lim;
    int rc = check_call(fn, ctx, blob_len, out_len, ops, n_ops, keys ? n_keys : nullptr, &lim);
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !out || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(status, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": status must be 4-byte aligned");
    // the core refuses an unknown mode before it launches anything; so does this call, which would otherwise find out after its wait
    if (mode != MLDSA_MODE_PURE && mode != MLDSA_MODE_INTERNAL && mode != MLDSA_MODE_PREHASH)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    for (int c = 0; c < 3; ++c) {
        const mldsa_recsign_keys& t = keys[c];
        if (t.n_keys != 0 && (!t.rho || !t.cap_k || !t.tr || !t.s_1_hat_mont || !t.s_2_hat_mont || !t.t_0_hat_mont))
            return fail(MLDSA_ERR_PARAM, std::string(fn) + ": a served set's key table has a NULL pointer");
    }
    FrontLayout F;
    PlanLayout L;
    front_layout(n_ops, &F, &L);
    if (!scratch || !aligned(scratch, 256) || scratch_bytes < F.bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_recsign_front_bytes");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint32_t* class_slot = reinterpret_cast<uint32_t*>(base + F.class_slot);
    mldsa_recsign_totals* d_totals = reinterpret_cast<mldsa_recsign_totals*>(base + F.totals);
    void* plan = base + F.plan;
    rc = launch_plan(fn, ops, n_ops, ClassOf{lim}, class_slot, d_totals, plan, L, s);
    if (rc != MLDSA_OK) return rc;
    mldsa_recsign_totals tot;
    ArenaLayout A;
    rc = read_totals(fn, d_totals, n_ops, arena_of, F.bytes, scratch_bytes, &tot, &A, info, s);  // the call's one host wait of its own
    if (rc != MLDSA_OK) return rc;
    mldsa_recsign_packed P;
    rc = pack_sign_scatter(fn, ctx, mode, keys, blob, ops, n_ops, lim, class_slot, plan, L, tot, base + F.bytes, A, &P, out, status, stream);
    // rnd is the scratch's one secret: its rows are cleared behind the call's last kernel whatever rc says
    const int zrc = A.rnd_bytes ? mldsa_memset(base + F.bytes + A.rnd, 0, A.rnd_bytes, stream) : MLDSA_OK;
    if (rc != MLDSA_OK) return rc;
    return zrc == MLDSA_OK ? MLDSA_OK : core_failed(fn, "mldsa_memset", zrc);
}

}  // extern "C"
