// libmldsa_rec.so (include/mldsa_rec.h): batched verification from serialized records -- a blob and one descriptor per op, any mix of
// parameter sets -- by sorting the ops by set and packing each set's dense arrays on the device, in front of mldsa_verify_pk.
//
// The phases are separate launches and the kernel boundaries do all the ordering: no wave waits for another workgroup.
//   the plan    k_classify, k_offsets, k_apply of rec_scan.h, shared with libmldsa_recsign.so: the descriptor's range check (rec_plan.h)
//               gives the op's class, a stable scan its slot, message position and context position within the class, and the totals.
//   k_pack      one wave per op: the op's four fields copied to their rows by the copy plan of rec_plan.h (copy_field of rec_scan.h) --
//               aligned 16-byte loads, funnel-shifted in registers by the difference of the two alignments, aligned 16-byte stores,
//               single bytes at the ends.
//   k_scatter   ok[i] = ok_c[slot], 0 for a refused op.
// What bounds them: k_pack reads and writes PK_LEN + SIG_LEN + |M| + |ctx| once per op (with a shift every 16-byte source chunk is
// loaded by two neighbouring lanes; the second comes from L1 / L2); the plan reads the 40-byte descriptors twice.
// Here: the descriptor's adaptor, the pack, the scatter, the arena and the entry points.  The plan's layouts, its launches and the wait
// for the totals are rec_host.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_rec.h"
#include "../layer/layer_host.h"
#include "rec_host.h"
#include "rec_plan.h"
#include "rec_scan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_rec;

static_assert(sizeof(mldsa_rec_op) == 40 && sizeof(mldsa_rec_totals) == 8 * SCAN_VALUES, "the layouts of include/mldsa_rec.h");
static_assert(SCAN_BLOCK == MLDSA_REC_SCAN_BLOCK && SCAN_BLOCK % 64 == 0 && MAX_OPS == MLDSA_REC_MAX_OPS, "the caps of include/mldsa_rec.h");
static_assert(CLASS_44 == MLDSA_REC_CLASS_44 && CLASS_65 == MLDSA_REC_CLASS_65 && CLASS_87 == MLDSA_REC_CLASS_87 &&
                  CLASS_REFUSED == MLDSA_REC_CLASS_REFUSED, "the classes of include/mldsa_rec.h");

constexpr int PACK_WAVES = 4;  // ops per workgroup of k_pack

__device__ __forceinline__ int classify_op(const mldsa_rec_op& d, uint64_t blob_len) {
    return classify(d.pk_off, d.sig_off, d.msg_off, d.ctx_off, d.msg_len, d.ctx_len, d.set, d.reserved, blob_len);
}

// k_classify's check: what a descriptor is checked against is the blob's length
struct InBlob {
    uint64_t blob_len;
    __device__ int operator()(const mldsa_rec_op& d) const { return classify_op(d, blob_len); }
};

// the arena of one class, as the kernels take it
struct ClassArrays {
    uint8_t *pk, *sigs, *msgs, *ctxs, *ok;
    uint64_t *msg_off, *ctx_off;
    uint64_t n, msg_bytes, ctx_bytes;
};
struct PackArgs {
    ClassArrays c[3];
};

__global__ __launch_bounds__(64 * PACK_WAVES) void k_pack(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                          const mldsa_rec_op* __restrict__ ops, uint32_t n,
                                                          const uint32_t* __restrict__ class_slot, const uint64_t* __restrict__ msg_pos,
                                                          const uint64_t* __restrict__ ctx_pos, PackArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
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
    const mldsa_rec_op d = ops[i];
    // The descriptor is checked again and the plan's numbers against the counts the host passed: only then is an offset followed or a
    // row written.  (cls is wave-uniform: one op per wave.)
    if (classify_op(d, blob_len) != cls) return;
    ClassArrays k = a.c[0];  // (selected, not indexed: the arguments stay in scalar registers)
    if (cls == CLASS_65) k = a.c[1];
    if (cls == CLASS_87) k = a.c[2];
    const uint64_t slot = cs & SLOT_MASK, mp = msg_pos[i], cp = ctx_pos[i];
    if (slot >= k.n || !in_range(mp, d.msg_len, k.msg_bytes) || !in_range(cp, d.ctx_len, k.ctx_bytes)) return;
    const uint32_t mis = (uint32_t)((uintptr_t)blob & 15);
    const uint8_t* base = blob - mis;
    copy_field(base, mis, blob_len, d.pk_off, pk_len(cls), k.pk + slot * pk_len(cls), lane);
    copy_field(base, mis, blob_len, d.sig_off, sig_len(cls), k.sigs + slot * sig_len(cls), lane);
    copy_field(base, mis, blob_len, d.msg_off, d.msg_len, k.msgs + mp, lane);
    copy_field(base, mis, blob_len, d.ctx_off, d.ctx_len, k.ctxs + cp, lane);
    if (lane == 0) {
        k.msg_off[slot] = mp;
        k.ctx_off[slot] = cp;
        if (slot + 1 == k.n) {  // the class's last op closes its tables
            k.msg_off[k.n] = mp + d.msg_len;
            k.ctx_off[k.n] = cp + d.ctx_len;
        }
    }
}

struct ScatterArgs {
    const uint8_t* ok[3];
    uint64_t n[3];
};

__global__ __launch_bounds__(256) void k_scatter(const uint32_t* __restrict__ class_slot, uint32_t n, ScatterArgs a, uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t cs = class_slot[i];
    const int cls = (int)(cs >> 30);
    const uint32_t slot = cs & SLOT_MASK;
    uint8_t v = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (cls == c && slot < a.n[c]) v = a.ok[c][slot];
    ok[i] = v;
}

// ------------------------------------------------------------------------------------------------------------ host side
// the arena: per class pk, sigs, msg_off, ctx_off, ok; then the messages and the contexts of the three classes back to back
struct ArenaLayout {
    size_t pk[3], sigs[3], msg_off[3], ctx_off[3], ok[3], msgs, ctxs, bytes;
};

bool arena_layout(const uint64_t (&n)[3], uint64_t msg_bytes, uint64_t ctx_bytes, ArenaLayout* o) {
    const uint64_t limit = (uint64_t)1 << 62;  // nothing below overflows under it
    if (msg_bytes > limit || ctx_bytes > limit) return false;
    Taker t;
    t.round = 256;
    for (int c = 0; c < 3; ++c) {
        if (n[c] > MLDSA_REC_MAX_OPS) return false;
        o->pk[c] = t.take((size_t)n[c] * pk_len(c));
        o->sigs[c] = t.take((size_t)n[c] * sig_len(c));
        o->msg_off[c] = t.take(8 * ((size_t)n[c] + 1));
        o->ctx_off[c] = t.take(8 * ((size_t)n[c] + 1));
        o->ok[c] = t.take((size_t)n[c]);
    }
    o->msgs = t.take((size_t)msg_bytes);
    o->ctxs = t.take((size_t)ctx_bytes);
    o->bytes = t.at;
    return true;
}

// the checks the three entry points share; the message names what failed
int check_records(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops) {
    if (n_ops > MLDSA_REC_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_REC_MAX_OPS ops");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if ((!blob && blob_len != 0) || !ops) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(ops, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": ops must be 8-byte aligned");
    return MLDSA_OK;
}

// totals (host) are consistent with n_ops and the arena is large enough: the caller checked
int launch_pack(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, const uint32_t* class_slot,
                const void* plan, const PlanLayout& L, const mldsa_rec_totals& tot, void* arena, const ArenaLayout& A, mldsa_rec_packed* out,
                hipStream_t s) {
    uint8_t* base = static_cast<uint8_t*>(arena);
    const uint8_t* pl = static_cast<const uint8_t*>(plan);
    PackArgs a;
    uint64_t m_at = 0, c_at = 0;
    for (int c = 0; c < 3; ++c) {
        ClassArrays& k = a.c[c];
        k.pk = base + A.pk[c];
        k.sigs = base + A.sigs[c];
        k.msg_off = reinterpret_cast<uint64_t*>(base + A.msg_off[c]);
        k.ctx_off = reinterpret_cast<uint64_t*>(base + A.ctx_off[c]);
        k.ok = base + A.ok[c];
        k.msgs = base + A.msgs + m_at;
        k.ctxs = base + A.ctxs + c_at;
        k.n = tot.n[c];
        k.msg_bytes = tot.msg_bytes[c];
        k.ctx_bytes = tot.ctx_bytes[c];
        m_at += tot.msg_bytes[c];
        c_at += tot.ctx_bytes[c];
        mldsa_rec_class& o = out->c[c];
        o.n = (size_t)k.n;
        o.pk = k.pk, o.sigs = k.sigs, o.msgs = k.msgs, o.ctxs = k.ctxs, o.ok = k.ok, o.msg_off = k.msg_off, o.ctx_off = k.ctx_off;
    }
    const uint32_t n = (uint32_t)n_ops;
    hipLaunchKernelGGL(k_pack, dim3((n + PACK_WAVES - 1) / PACK_WAVES), dim3(64 * PACK_WAVES), 0, s, blob, blob_len, ops, n, class_slot,
                       reinterpret_cast<const uint64_t*>(pl + L.msg_pos), reinterpret_cast<const uint64_t*>(pl + L.ctx_pos), a);
    LAYER_LAUNCHED("k_pack launch");
    return MLDSA_OK;
}

// the arena of the totals; false when they do not describe n_ops ops or the size does not fit
bool arena_of(const mldsa_rec_totals& t, size_t n_ops, ArenaLayout* A) {
    const uint64_t n[3] = {t.n[0], t.n[1], t.n[2]};
    return totals_consistent(t, n_ops) && arena_layout(n, sum3(t.msg_bytes), sum3(t.ctx_bytes), A);
}

}  // namespace

extern "C" {

int mldsa_rec_abi_version(void) { return MLDSA_REC_ABI_VERSION; }

const char* mldsa_rec_last_error(void) { return g_err.c_str(); }

size_t mldsa_rec_plan_bytes(size_t n_ops) { return plan_bytes(n_ops); }

size_t mldsa_rec_front_bytes(size_t n_ops) { return front_bytes(n_ops); }

size_t mldsa_rec_scratch_bytes(size_t n44, size_t n65, size_t n87, uint64_t msg_bytes, uint64_t ctx_bytes) {
    ArenaLayout A;
    const uint64_t n[3] = {n44, n65, n87};
    return arena_layout(n, msg_bytes, ctx_bytes, &A) ? A.bytes : 0;
}

size_t mldsa_rec_scratch_bytes_max(size_t n_ops, uint64_t msg_bytes, uint64_t ctx_bytes) {
    if (n_ops > MLDSA_REC_MAX_OPS || msg_bytes > ((uint64_t)1 << 62) || ctx_bytes > ((uint64_t)1 << 62)) return 0;
    return up256(n_ops * pk_len(CLASS_87)) + up256(n_ops * sig_len(CLASS_87)) + 2 * up256(8 * n_ops + 24) + up256(n_ops) + 5 * 512 +
           up256((size_t)msg_bytes) + up256((size_t)ctx_bytes);
}

int mldsa_rec_plan(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, uint32_t* class_slot,
                   mldsa_rec_totals* totals, void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_rec_plan";
    if (n_ops == 0) return MLDSA_OK;
    int rc = check_records(fn, ctx, blob, blob_len, ops, n_ops);
    if (rc != MLDSA_OK) return rc;
    PlanLayout L;
    if (!class_slot || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4) || !aligned(totals, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned, totals 8-byte aligned");
    rc = check_plan_memory(fn, "mldsa_rec", plan, plan_bytes, n_ops, &L);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_plan(fn, ops, n_ops, InBlob{blob_len}, class_slot, totals, plan, L, (hipStream_t)stream);
}

int mldsa_rec_pack(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, const uint32_t* class_slot,
                   const void* plan, size_t plan_bytes, const mldsa_rec_totals* totals, void* arena, size_t arena_bytes, mldsa_rec_packed* out,
                   void* stream) {
    const char* fn = "mldsa_rec_pack";
    if (n_ops == 0) {
        if (out) memset(out, 0, sizeof(*out));
        return MLDSA_OK;
    }
    int rc = check_records(fn, ctx, blob, blob_len, ops, n_ops);
    if (rc != MLDSA_OK) return rc;
    PlanLayout L;
    if (!class_slot || !totals || !out) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned");
    rc = check_plan_memory(fn, "mldsa_rec", plan, plan_bytes, n_ops, &L);
    if (rc != MLDSA_OK) return rc;
    ArenaLayout A;
    if (!arena_of(*totals, n_ops, &A)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": the totals do not describe n_ops ops");
    if (!arena || !aligned(arena, 256)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": arena is NULL or not 256-byte aligned");
    if (arena_bytes < A.bytes) return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": arena smaller than mldsa_rec_scratch_bytes of the totals");
    LAYER_ON_DEVICE(ctx);
    return launch_pack(fn, blob, blob_len, ops, n_ops, class_slot, plan, L, *totals, arena, A, out, (hipStream_t)stream);
}

int mldsa_rec_verify(mldsa_ctx* ctx, int mode, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, uint8_t* ok,
                     void* scratch, size_t scratch_bytes, mldsa_rec_info* info, void* stream) {
    const char* fn = "mldsa_rec_verify";
    if (n_ops == 0) return MLDSA_OK;
    int rc = check_records(fn, ctx, blob, blob_len, ops, n_ops);
    if (rc != MLDSA_OK) return rc;
    // the core refuses an unknown mode before it launches anything; so does this call, which would otherwise find out after its wait
    if (mode != MLDSA_MODE_PURE && mode != MLDSA_MODE_INTERNAL && mode != MLDSA_MODE_PREHASH)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (!ok) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    FrontLayout F;
    PlanLayout L;
    front_layout(n_ops, &F, &L);
    if (!scratch || !aligned(scratch, 256) || scratch_bytes < F.bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_rec_front_bytes");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint32_t* class_slot = reinterpret_cast<uint32_t*>(base + F.class_slot);
    mldsa_rec_totals* d_totals = reinterpret_cast<mldsa_rec_totals*>(base + F.totals);
    void* plan = base + F.plan;
    rc = launch_plan(fn, ops, n_ops, InBlob{blob_len}, class_slot, d_totals, plan, L, s);
    if (rc != MLDSA_OK) return rc;
    mldsa_rec_totals tot;
    ArenaLayout A;
    rc = read_totals(fn, d_totals, n_ops, arena_of, F.bytes, scratch_bytes, &tot, &A, info, s);  // the call's one host wait
    if (rc != MLDSA_OK) return rc;
    mldsa_rec_packed P;
    rc = launch_pack(fn, blob, blob_len, ops, n_ops, class_slot, plan, L, tot, base + F.bytes, A, &P, s);
    if (rc != MLDSA_OK) return rc;
    ScatterArgs sc;
    for (int c = 0; c < 3; ++c) {
        const mldsa_rec_class& k = P.c[c];
        sc.ok[c] = k.ok;
        sc.n[c] = k.n;
        if (k.n == 0) continue;
        LAYER_CORE(mldsa_verify_pk(ctx, set_of_class(c), mode, k.pk, k.n, nullptr, k.msgs, k.msg_off, k.ctxs, k.ctx_off, k.sigs, k.ok, k.n, stream),
                   "mldsa_verify_pk");
    }
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)((n_ops + 255) / 256)), dim3(256), 0, s, class_slot, (uint32_t)n_ops, sc, ok);
    LAYER_LAUNCHED("k_scatter launch");
    return MLDSA_OK;
}

}  // extern "C"
