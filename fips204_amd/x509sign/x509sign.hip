// libmldsa_x509sign.so (include/mldsa_x509sign.h): TBSCertificates in a blob to framed DER certificates in an output buffer and one
// mldsa_recsign_op per certificate -- the check of every TBS, the layout of `out` and the frame on the device, in front of
// mldsa_recsign_sign (which this library neither links nor calls).
//
// Four launches, ordered by the kernel boundaries alone: no wave waits for another workgroup.
//   k_x509sign_check    one request per lane, CHECK_BLOCK lanes per workgroup, as k_x509_parse: the rules and the walk of x509sign_plan.h
//                       on the blob; status[i], cert_len (0 when refused) and, per workgroup, the sum of the lengths and the count of
//                       accepted requests.
//   k_x509sign_offsets  one wave: the workgroups' two sums to exclusive prefixes (in place), and the totals.
//   k_x509sign_apply    the same two quantities scanned inside the workgroup (the wave scans, the waves' totals through LDS): every
//                       certificate's offset in `out`, the SPACE rule, out_certs[i], ops[i], status[i].  The one certificate whose
//                       range straddles out_len -- the first that does not fit -- corrects the totals' counts.
//   k_x509sign_frame    one certificate per wave, FRAME_WAVES per workgroup: 4 header bytes, the TBS by copy_field of ../rec/rec_wave.h
//                       (aligned 16-byte loads, funnel-shifted, aligned 16-byte stores, single bytes at the ends), 18 trailer bytes.
// What bounds them: latency of the walk's dependent loads in k_x509sign_check; k_x509sign_frame reads len and writes len + 22 bytes per
// certificate (with a shift every 16-byte source chunk is loaded by two neighbouring lanes; the second comes from L1 / L2) and a
// certificate of 1.5 ... 3 KB is 1.5 ... 3 steps of its wave, so the launch is bound by the waves' fixed cost, not by the bytes: measured
// 2.5 / 3.1 / 3.6 TB/s for ML-DSA-44 / 65 / 87 TBSs where a plain copy reaches 4.2 ... 4.5 (profiles/x509sign_bench.jsonl).
// The scan of the first three kernels is the placement scan of ../rec/rec_place.h, which libmldsa_csr.so shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_x509sign.h"
#include "../layer/layer_host.h"
#include "../rec/rec_place.h"
#include "../x509/x509_dev.h"
#include "x509sign_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_x509sign;
using mldsa_rec::copy_field;
using mldsa_rec::PLACE_SUMS;
using mldsa_x509::BlobBytes;

static_assert(sizeof(mldsa_x509sign_req) == 32 && sizeof(mldsa_x509_cert) == 16 && sizeof(mldsa_recsign_op) == 48 &&
                  sizeof(mldsa_x509sign_totals) == 24, "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_ALG == MLDSA_X509_ALG &&
                  ST_ENTRY == MLDSA_X509SIGN_ENTRY && ST_KEY == MLDSA_X509SIGN_KEY && ST_LONG == MLDSA_X509SIGN_LONG &&
                  ST_SPACE == MLDSA_X509SIGN_SPACE, "the status codes of include/mldsa_x509sign.h and include/mldsa_x509.h");
static_assert(FLAG_RND == MLDSA_X509SIGN_RND && FLAG_RND == MLDSA_RECSIGN_RND && MAX_CERTS == MLDSA_X509SIGN_MAX_CERTS &&
                  CHECK_BLOCK == MLDSA_X509SIGN_SCAN_BLOCK && CHECK_BLOCK % 64 == 0, "the flag and the caps of include/mldsa_x509sign.h");
static_assert(max_tbs_len(CLASS_44) == 63097 && max_tbs_len(CLASS_65) == 62208 && max_tbs_len(CLASS_87) == 60890 &&
                  cert_len(CLASS_87, max_tbs_len(CLASS_87)) == 65539, "the bounds include/mldsa_x509sign.h states");

constexpr int CHECK_WAVES = CHECK_BLOCK / 64;
constexpr int FRAME_WAVES = 4;  // certificates per workgroup of k_x509sign_frame

// what a request is checked against: the two buffer lengths and the rows of the three key tables
struct Limits {
    uint64_t blob_len, out_len;
    uint32_t n_keys[3];
};

__global__ __launch_bounds__(CHECK_BLOCK) void k_x509sign_check(const uint8_t* __restrict__ blob, const mldsa_x509sign_req* __restrict__ reqs,
                                                                uint32_t n, Limits L, uint8_t* __restrict__ status,
                                                                uint32_t* __restrict__ lens, uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[CHECK_WAVES][PLACE_SUMS];
    const uint32_t i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    uint64_t bytes = 0, count = 0;  // no request: counted nowhere
    if (i < n) {
        const mldsa_x509sign_req r = reqs[i];
        int st = entry_status(r.off, r.rnd_off, r.len, r.key, r.set, r.flags, r.reserved, L.blob_len, L.n_keys[0], L.n_keys[1], L.n_keys[2]);
        if (st == ST_OK) st = walk_tbs(BlobBytes{blob + r.off}, r.len, r.set);
        if (st == ST_OK) {
            bytes = cert_len(class_of_set(r.set), r.len);
            count = 1;
        }
        status[i] = (uint8_t)st;
        lens[i] = (uint32_t)bytes;
    }
    uint64_t v[PLACE_SUMS] = {bytes, count};
    mldsa_rec::place_block_sums(v, part, sums);
}

// one wave: sums[b][q] -> the sum over the blocks before b (in place); the totals as they stand when every certificate fits
__global__ __launch_bounds__(64) void k_x509sign_offsets(uint64_t* __restrict__ sums, uint32_t n_blocks, uint32_t n,
                                                         mldsa_x509sign_totals* __restrict__ totals) {
    uint64_t total[PLACE_SUMS];
    mldsa_rec::place_block_offsets(sums, n_blocks, total);
    if (threadIdx.x == 0) mldsa_rec::place_totals(totals, n, total);
}

__global__ __launch_bounds__(CHECK_BLOCK) void k_x509sign_apply(const mldsa_x509sign_req* __restrict__ reqs, uint32_t n, uint64_t out_len,
                                                                const uint32_t* __restrict__ lens, const uint64_t* __restrict__ sums,
                                                                mldsa_x509_cert* __restrict__ out_certs, mldsa_recsign_op* __restrict__ ops,
                                                                uint8_t* __restrict__ status, mldsa_x509sign_totals* __restrict__ totals) {
    __shared__ uint64_t part[CHECK_WAVES][PLACE_SUMS];
    const uint32_t i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    int st = ST_OK;
    uint64_t bytes = 0, count = 0;
    if (i < n) {
        st = status[i];  // k_x509sign_check's verdict on this request
        if (st == ST_OK) {
            bytes = lens[i];
            count = 1;
        }
    }
    const uint64_t v[PLACE_SUMS] = {bytes, count};
    uint64_t inc[PLACE_SUMS], before[PLACE_SUMS];
    mldsa_rec::place_wave_scan(v, part, inc);
    if (i >= n) return;
    mldsa_rec::place_before(v, inc, part, sums, before);
    const uint64_t at = before[0];
    if (st == ST_OK && !mldsa_rec::place_fits(at, bytes, out_len, before[1], n, totals)) st = ST_SPACE;
    const bool acc = st == ST_OK;  // every other certificate's rows are the refusal's
    const mldsa_x509sign_req r = reqs[i];
    mldsa_x509_cert& c = out_certs[i];
    c.off = acc ? at : 0;
    c.len = acc ? (uint32_t)bytes : 0;
    c.issuer = acc ? r.issuer : MLDSA_X509_NO_ISSUER;
    mldsa_recsign_op& op = ops[i];
    op.msg_off = acc ? r.off : 0;
    op.ctx_off = 0;
    op.rnd_off = acc ? r.rnd_off : 0;
    op.sig_off = acc ? at + r.len + FRAME_LEN : 0;
    op.msg_len = acc ? r.len : 0;
    op.key = acc ? r.key : 0;
    op.ctx_len = 0;
    op.set = acc ? r.set : 0;
    op.flags = acc ? r.flags : 0;
    op.reserved = 0;
    status[i] = (uint8_t)st;
}

__global__ __launch_bounds__(64 * FRAME_WAVES) void k_x509sign_frame(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                                     const mldsa_x509sign_req* __restrict__ reqs, uint32_t n,
                                                                     uint8_t* __restrict__ out, uint64_t out_len,
                                                                     const mldsa_x509_cert* __restrict__ out_certs,
                                                                     const uint8_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave: one certificate per wave)
    if (status[i] != ST_OK) return;
    const mldsa_x509sign_req r = reqs[i];
    const mldsa_x509_cert c = out_certs[i];
    // Both ranges are checked again, and the row against the request: only then is an offset followed or a byte written.
    const int cls = class_of_set(r.set);
    if (cls == CLASS_REFUSED || r.len < 2 || r.len > max_tbs_len(cls) || !in_range(r.off, r.len, blob_len)) return;
    if (c.len != cert_len(cls, r.len) || !in_range(c.off, c.len, out_len)) return;
    uint8_t* cert = out + c.off;
    if (lane < (int)HEADER_LEN) cert[lane] = (uint8_t)header_byte(lane, c.len);
    const uint32_t mis = (uint32_t)((uintptr_t)blob & 15);
    copy_field(blob - mis, mis, blob_len, r.off, r.len, cert + HEADER_LEN, lane);
    if (lane < (int)TRAILER_LEN) cert[HEADER_LEN + r.len + lane] = (uint8_t)trailer_byte(lane, cls);
}

// ------------------------------------------------------------------------------------------------------------ host side
// the checks the entry points share; the message names what failed
int check_reqs(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509sign_req* reqs, size_t n) {
    if (n > MLDSA_X509SIGN_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_X509SIGN_MAX_CERTS certificates");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if ((!blob && blob_len != 0) || !reqs) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(reqs, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": reqs must be 8-byte aligned");
    return MLDSA_OK;
}

// *L is filled
int check_plan(const char* fn, uint64_t blob_len, uint64_t out_len, const size_t* n_keys, size_t n, const mldsa_x509_cert* out_certs,
               const mldsa_recsign_op* ops, const uint8_t* status, const mldsa_x509sign_totals* totals, const void* plan, size_t bytes,
               Limits* L) {
    if (!n_keys || !out_certs || !ops || !status || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(out_certs, 8) || !aligned(ops, 8) || !aligned(totals, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": out_certs, ops and totals must be 8-byte aligned");
    L->blob_len = blob_len;
    L->out_len = out_len;
    for (int c = 0; c < 3; ++c) {
        if (n_keys[c] > UINT32_MAX) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys above UINT32_MAX");
        L->n_keys[c] = (uint32_t)n_keys[c];
    }
    if (!plan || !aligned(plan, 256) || bytes < plan_bytes(n))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": plan is NULL, not 256-byte aligned or smaller than mldsa_x509sign_plan_bytes");
    return MLDSA_OK;
}

int check_frame(const char* fn, const uint8_t* blob, uint64_t blob_len, const uint8_t* out, uint64_t out_len, const mldsa_x509_cert* out_certs,
                const uint8_t* status) {
    if ((!out && out_len != 0) || !out_certs || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(out_certs, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": out_certs must be 8-byte aligned");
    if (!ranges_apart(blob, blob_len, out, out_len)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": out overlaps the blob");
    return MLDSA_OK;
}

// every check is the caller's: 1 <= n <= MLDSA_X509SIGN_MAX_CERTS, the current device is the context's
int launch_plan(const char* fn, const uint8_t* blob, const mldsa_x509sign_req* reqs, size_t n_certs, const Limits& lim,
                mldsa_x509_cert* out_certs, mldsa_recsign_op* ops, uint8_t* status, mldsa_x509sign_totals* totals, void* plan, hipStream_t s) {
    uint8_t* base = static_cast<uint8_t*>(plan);
    uint64_t* sums = reinterpret_cast<uint64_t*>(base);
    uint32_t* lens = reinterpret_cast<uint32_t*>(base + plan_sums_bytes(n_certs));
    const uint32_t n = (uint32_t)n_certs, nb = (uint32_t)n_blocks(n_certs);
    hipLaunchKernelGGL(k_x509sign_check, dim3(nb), dim3(CHECK_BLOCK), 0, s, blob, reqs, n, lim, status, lens, sums);
    hipLaunchKernelGGL(k_x509sign_offsets, dim3(1), dim3(64), 0, s, sums, nb, n, totals);
    hipLaunchKernelGGL(k_x509sign_apply, dim3(nb), dim3(CHECK_BLOCK), 0, s, reqs, n, lim.out_len, lens, sums, out_certs, ops, status, totals);
    LAYER_LAUNCHED("plan launch");
    return MLDSA_OK;
}

int launch_frame(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_x509sign_req* reqs, size_t n_certs, uint8_t* out,
                 uint64_t out_len, const mldsa_x509_cert* out_certs, const uint8_t* status, hipStream_t s) {
    const uint32_t n = (uint32_t)n_certs;
    hipLaunchKernelGGL(k_x509sign_frame, dim3((n + FRAME_WAVES - 1) / FRAME_WAVES), dim3(64 * FRAME_WAVES), 0, s, blob, blob_len, reqs, n, out,
                       out_len, out_certs, status);
    LAYER_LAUNCHED("k_x509sign_frame launch");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_x509sign_abi_version(void) { return MLDSA_X509SIGN_ABI_VERSION; }

const char* mldsa_x509sign_last_error(void) { return g_err.c_str(); }

size_t mldsa_x509sign_cert_len(int set, size_t tbs_len) {
    const int c = class_of_set((uint32_t)set);
    if (set < 0 || c == CLASS_REFUSED || tbs_len > max_tbs_len(c)) return 0;
    return cert_len(c, (uint32_t)tbs_len);
}

size_t mldsa_x509sign_out_bytes_max(size_t n, uint64_t tbs_bytes) {
    const uint64_t per = FRAME_LEN + sig_len(CLASS_87);
    if (n > MLDSA_X509SIGN_MAX_CERTS || tbs_bytes > SIZE_MAX - n * per) return 0;
    return (size_t)(tbs_bytes + n * per);
}

size_t mldsa_x509sign_plan_bytes(size_t n) { return plan_bytes(n); }

int mldsa_x509sign_plan(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509sign_req* reqs, size_t n, const size_t* n_keys,
                        uint64_t out_len, mldsa_x509_cert* out_certs, mldsa_recsign_op* ops, uint8_t* status, mldsa_x509sign_totals* totals,
                        void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_x509sign_plan";
    if (n == 0) return MLDSA_OK;
    Limits lim;
    int rc = check_reqs(fn, ctx, blob, blob_len, reqs, n);
    if (rc == MLDSA_OK) rc = check_plan(fn, blob_len, out_len, n_keys, n, out_certs, ops, status, totals, plan, plan_bytes, &lim);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_plan(fn, blob, reqs, n, lim, out_certs, ops, status, totals, plan, (hipStream_t)stream);
}

int mldsa_x509sign_frame(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509sign_req* reqs, size_t n, uint8_t* out,
                         uint64_t out_len, const mldsa_x509_cert* out_certs, const uint8_t* status, void* stream) {
    const char* fn = "mldsa_x509sign_frame";
    if (n == 0) return MLDSA_OK;
    int rc = check_reqs(fn, ctx, blob, blob_len, reqs, n);
    if (rc == MLDSA_OK) rc = check_frame(fn, blob, blob_len, out, out_len, out_certs, status);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_frame(fn, blob, blob_len, reqs, n, out, out_len, out_certs, status, (hipStream_t)stream);
}

int mldsa_x509sign_issue_ops(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509sign_req* reqs, size_t n,
                             const size_t* n_keys, uint8_t* out, uint64_t out_len, mldsa_x509_cert* out_certs, mldsa_recsign_op* ops,
                             uint8_t* status, mldsa_x509sign_totals* totals, void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_x509sign_issue_ops";
    if (n == 0) return MLDSA_OK;
    Limits lim;
    int rc = check_reqs(fn, ctx, blob, blob_len, reqs, n);
    if (rc == MLDSA_OK) rc = check_plan(fn, blob_len, out_len, n_keys, n, out_certs, ops, status, totals, plan, plan_bytes, &lim);
    if (rc == MLDSA_OK) rc = check_frame(fn, blob, blob_len, out, out_len, out_certs, status);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    rc = launch_plan(fn, blob, reqs, n, lim, out_certs, ops, status, totals, plan, (hipStream_t)stream);
    if (rc != MLDSA_OK) return rc;
    return launch_frame(fn, blob, blob_len, reqs, n, out, out_len, out_certs, status, (hipStream_t)stream);
}

}  // extern "C"
