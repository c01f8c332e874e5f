// libmldsa_rec.so (include/mldsa_rec.h): batched verification from serialized records -- a blob and one descriptor per op, any mix of
// parameter sets -- by sorting the ops by set and packing each set's dense arrays on the device, in front of mldsa_verify_pk.
//
// The phases are separate launches and the kernel boundaries do all the ordering: no wave waits for another workgroup.
//   k_classify  one op per thread, MLDSA_REC_SCAN_BLOCK per workgroup: the descriptor's range check (rec_plan.h) gives the op's class;
//               the workgroup's ten sums -- ops per class, message and context bytes per accepted class -- go to sums[block].
//   k_offsets   one wave per quantity: sums[block] -> the sums of the blocks before it (in place); the ten totals.
//   k_apply     the same ten quantities scanned inside the workgroup (wave scans, then the waves' totals through LDS): slot, message
//               position and context position of every op within its class.  A scan, so slots follow input order.
//   k_pack      one wave per op: the op's four fields copied to their rows by the copy plan of rec_plan.h -- aligned 16-byte loads,
//               funnel-shifted in registers by the difference of the two alignments, aligned 16-byte stores, single bytes at the ends.
//   k_scatter   ok[i] = ok_c[slot], 0 for a refused op.
// What bounds them: k_pack reads and writes PK_LEN + SIG_LEN + |M| + |ctx| once per op (with a shift every 16-byte source chunk is
// loaded by two neighbouring lanes; the second comes from L1 / L2); the plan reads the 40-byte descriptors twice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_rec.h"
#include "../layer/layer_host.h"
#include "rec_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_rec;

static_assert(sizeof(mldsa_rec_op) == 40 && sizeof(mldsa_rec_totals) == 8 * SCAN_VALUES, "the layouts of include/mldsa_rec.h");
static_assert(SCAN_BLOCK == MLDSA_REC_SCAN_BLOCK && SCAN_BLOCK % 64 == 0, "the scan block of include/mldsa_rec.h");
static_assert(CLASS_44 == MLDSA_REC_CLASS_44 && CLASS_65 == MLDSA_REC_CLASS_65 && CLASS_87 == MLDSA_REC_CLASS_87 &&
                  CLASS_REFUSED == MLDSA_REC_CLASS_REFUSED, "the classes of include/mldsa_rec.h");

constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int PACK_WAVES = 4;  // ops per workgroup of k_pack
constexpr uint32_t SLOT_MASK = (1u << 30) - 1;

__device__ __forceinline__ int classify_op(const mldsa_rec_op& d, uint64_t blob_len) {
    return classify(d.pk_off, d.sig_off, d.msg_off, d.ctx_off, d.msg_len, d.ctx_len, d.set, d.reserved, blob_len);
}

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

__device__ __forceinline__ uint64_t wave_inclusive(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_classify(const mldsa_rec_op* __restrict__ ops, uint32_t n, uint64_t blob_len,
                                                         uint32_t* __restrict__ class_slot, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[SCAN_WAVES][SCAN_VALUES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int cls = -1;  // no op: counted nowhere
    uint32_t msg_len = 0, ctx_len = 0;
    if (i < n) {
        const mldsa_rec_op d = ops[i];
        cls = classify_op(d, blob_len);
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

__global__ __launch_bounds__(SCAN_BLOCK) void k_apply(const mldsa_rec_op* __restrict__ ops, uint32_t n, const uint64_t* __restrict__ sums,
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

// ---- the copy ---------------------------------------------------------------------------------------------------------------------------
// `len` bytes from blob offset `off` (range check passed) to dst, by the whole wave.  `base` is the blob's address rounded down to 16 and
// mis = blob - base: the frame of rec_plan.h.
__device__ __forceinline__ void copy_field(const uint8_t* __restrict__ base, uint32_t mis, uint64_t blob_len, uint64_t off, uint32_t len,
                                           uint8_t* __restrict__ dst, int lane) {
    const uint64_t src = mis + off;
    const CopyPlan p = copy_plan(src, len, (uint64_t)(uintptr_t)dst, mis, mis + blob_len);
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
struct PlanLayout {
    size_t n_blocks, sums, msg_pos, ctx_pos, bytes;
};

bool plan_layout(size_t n, PlanLayout* o) {
    if (n > MLDSA_REC_MAX_OPS) return false;
    Taker t;
    t.round = 256;
    o->n_blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    o->sums = t.take(8 * SCAN_VALUES * o->n_blocks);
    o->msg_pos = t.take(8 * n);
    o->ctx_pos = t.take(8 * n);
    o->bytes = t.at;
    return true;
}

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

struct FrontLayout {
    size_t class_slot, totals, plan, bytes;
};

bool front_layout(size_t n, FrontLayout* o, PlanLayout* p) {
    if (!plan_layout(n, p)) return false;
    Taker t;
    t.round = 256;
    o->class_slot = t.take(4 * n);
    o->totals = t.take(sizeof(mldsa_rec_totals));
    o->plan = t.take(p->bytes);
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

// every check is the caller's: 1 <= n_ops <= MLDSA_REC_MAX_OPS, the current device is the context's
int launch_plan(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, uint32_t* class_slot,
                mldsa_rec_totals* totals, void* plan, const PlanLayout& L, hipStream_t s) {
    (void)blob;
    uint8_t* base = static_cast<uint8_t*>(plan);
    uint64_t* sums = reinterpret_cast<uint64_t*>(base + L.sums);
    const uint32_t n = (uint32_t)n_ops, nb = (uint32_t)L.n_blocks;
    hipLaunchKernelGGL(k_classify, dim3(nb), dim3(SCAN_BLOCK), 0, s, ops, n, blob_len, class_slot, sums);
    hipLaunchKernelGGL(k_offsets, dim3(SCAN_VALUES), dim3(64), 0, s, sums, nb, reinterpret_cast<uint64_t*>(totals));
    hipLaunchKernelGGL(k_apply, dim3(nb), dim3(SCAN_BLOCK), 0, s, ops, n, sums, class_slot, reinterpret_cast<uint64_t*>(base + L.msg_pos),
                       reinterpret_cast<uint64_t*>(base + L.ctx_pos));
    LAYER_LAUNCHED("plan launch");
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
    for (int c = 0; c < 4; ++c)
        if (t.n[c] > n_ops) return false;
    if (t.n[0] + t.n[1] + t.n[2] + t.n[3] != n_ops) return false;
    const uint64_t limit = (uint64_t)1 << 60;
    for (int c = 0; c < 3; ++c)
        if (t.msg_bytes[c] > limit || t.ctx_bytes[c] > limit) return false;
    const uint64_t n[3] = {t.n[0], t.n[1], t.n[2]};
    return arena_layout(n, t.msg_bytes[0] + t.msg_bytes[1] + t.msg_bytes[2], t.ctx_bytes[0] + t.ctx_bytes[1] + t.ctx_bytes[2], A);
}

}  // namespace

extern "C" {

int mldsa_rec_abi_version(void) { return MLDSA_REC_ABI_VERSION; }

const char* mldsa_rec_last_error(void) { return g_err.c_str(); }

size_t mldsa_rec_plan_bytes(size_t n_ops) {
    PlanLayout L;
    return plan_layout(n_ops, &L) ? L.bytes : 0;
}

size_t mldsa_rec_front_bytes(size_t n_ops) {
    FrontLayout F;
    PlanLayout L;
    return front_layout(n_ops, &F, &L) ? F.bytes : 0;
}

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
    const int rc = check_records(fn, ctx, blob, blob_len, ops, n_ops);
    if (rc != MLDSA_OK) return rc;
    PlanLayout L;
    plan_layout(n_ops, &L);
    if (!class_slot || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4) || !aligned(totals, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned, totals 8-byte aligned");
    if (!plan || !aligned(plan, 256) || plan_bytes < L.bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": plan is NULL, not 256-byte aligned or smaller than mldsa_rec_plan_bytes");
    LAYER_ON_DEVICE(ctx);
    return launch_plan(fn, blob, blob_len, ops, n_ops, class_slot, totals, plan, L, (hipStream_t)stream);
}

int mldsa_rec_pack(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_rec_op* ops, size_t n_ops, const uint32_t* class_slot,
                   const void* plan, size_t plan_bytes, const mldsa_rec_totals* totals, void* arena, size_t arena_bytes, mldsa_rec_packed* out,
                   void* stream) {
    const char* fn = "mldsa_rec_pack";
    if (n_ops == 0) {
        if (out) memset(out, 0, sizeof(*out));
        return MLDSA_OK;
    }
    const int rc = check_records(fn, ctx, blob, blob_len, ops, n_ops);
    if (rc != MLDSA_OK) return rc;
    PlanLayout L;
    plan_layout(n_ops, &L);
    if (!class_slot || !totals || !out) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(class_slot, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": class_slot must be 4-byte aligned");
    if (!plan || !aligned(plan, 256) || plan_bytes < L.bytes)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": plan is NULL, not 256-byte aligned or smaller than mldsa_rec_plan_bytes");
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
    rc = launch_plan(fn, blob, blob_len, ops, n_ops, class_slot, d_totals, plan, L, s);
    if (rc != MLDSA_OK) return rc;
    // the call's one host wait: the arena depends on the mix
    mldsa_rec_totals tot;
    hipError_t e = hipMemcpyAsync(&tot, d_totals, sizeof(tot), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_failed(fn, "reading the totals", e);
    ArenaLayout A;
    if (!arena_of(tot, n_ops, &A)) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": the plan's totals do not add up to n_ops");
    if (info) {
        for (int c = 0; c < 4; ++c) info->n[c] = tot.n[c];
        info->msg_bytes = tot.msg_bytes[0] + tot.msg_bytes[1] + tot.msg_bytes[2];
        info->ctx_bytes = tot.ctx_bytes[0] + tot.ctx_bytes[1] + tot.ctx_bytes[2];
        info->scratch_needed = F.bytes + A.bytes;
    }
    if (scratch_bytes - F.bytes < A.bytes)
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": scratch holds " + std::to_string(scratch_bytes) + " bytes, this mix needs " +
                                         std::to_string(F.bytes + A.bytes));
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
