// libmldsa_csr.so (include/mldsa_csr.h): PKCS#10 certification requests in a blob to mldsa_rec_op descriptors (the proof of possession,
// in front of mldsa_rec_verify) and, given the verdicts, to TBSCertificates laid out in an output buffer with one mldsa_x509sign_req
// each (in front of mldsa_x509sign_issue_ops).  This library links and calls none of them.
//
// Five kernels, ordered by the kernel boundaries alone: no wave waits for another workgroup.
//   k_csr_parse      one request per lane, SCAN_BLOCK lanes per workgroup, as k_x509_parse: the range check and the walk of csr_plan.h on
//                    the blob; one mldsa_csr_fields row, one mldsa_rec_op and one status byte per request.
//   k_csr_check      one request per lane: the stage-2 rules of csr_plan.h up to LONG on the row, the entry, the verdict and the template's
//                    TLV headers; status[i], tbs_len (0 when refused) and, per workgroup, the sum of the lengths and the count of
//                    accepted requests.
//   k_csr_offsets    one wave: the workgroups' two sums to exclusive prefixes (in place), and the totals.
//   k_csr_apply      the same two quantities scanned inside the workgroup (the wave scans, the waves' totals through LDS): every
//                    TBSCertificate's offset in `out`, the SPACE rule, reqs_out[i], status[i].  The one request whose range straddles
//                    out_len -- the first that does not fit -- corrects the totals' counts.
//   k_csr_tbs_write  one request per wave, WRITE_WAVES per workgroup: 24 fixed bytes by single lanes, the six pieces by copy_field of
//                    ../rec/rec_wave.h (aligned 16-byte loads, funnel-shifted, aligned 16-byte stores, single bytes at the ends).
// The scan of the three middle kernels is the placement scan of ../rec/rec_place.h, which libmldsa_x509sign.so shares.
// What bounds them: latency of the walk's dependent loads in k_csr_parse and of the template headers' in k_csr_check; k_csr_tbs_write
// reads and writes tbs_len bytes per request, 1.4 ... 2.7 KB in six pieces of which four are under 64 bytes, so a wave's life is its
// prologue and six dependent load-store steps: measured 1.5 / 2.0 / 2.4 TB/s for ML-DSA-44 / 65 / 87 where a plain copy reaches 4.4 ... 5.1
// (profiles/csr_bench.jsonl).  What helps is waves in flight: the wave's three rows are read through scalar loads, which keeps the
// kernel at 58 VGPRs and eight waves per SIMD.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_csr.h"
#include "../layer/layer_host.h"
#include "../rec/rec_place.h"
#include "../x509/x509_dev.h"
#include "csr_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_csr;
using mldsa_rec::copy_field;
using mldsa_rec::PLACE_SUMS;
using mldsa_x509::BlobBytes;

static_assert(sizeof(mldsa_csr_item) == 16 && sizeof(mldsa_csr_fields) == 56 && sizeof(mldsa_csr_issue) == 64 &&
                  sizeof(mldsa_csr_totals) == 24 && sizeof(mldsa_rec_op) == 40 && sizeof(mldsa_x509sign_req) == 32,
              "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_ALG == MLDSA_X509_ALG &&
                  ST_SIG == MLDSA_X509_SIG && ST_VERSION == MLDSA_CSR_VERSION && ST_KEY == MLDSA_CSR_KEY && ST_POP == MLDSA_CSR_POP &&
                  ST_ENTRY == MLDSA_CSR_ENTRY && ST_TEMPLATE == MLDSA_CSR_TEMPLATE && ST_LONG == MLDSA_CSR_LONG && ST_SPACE == MLDSA_CSR_SPACE,
              "the status codes of include/mldsa_csr.h and include/mldsa_x509.h");
static_assert(FLAG_RND == MLDSA_CSR_RND && FLAG_RND == MLDSA_X509SIGN_RND && SERIAL_MAX == MLDSA_CSR_SERIAL_MAX &&
                  MAX_REQUESTS == MLDSA_CSR_MAX_REQUESTS && SCAN_BLOCK == MLDSA_CSR_SCAN_BLOCK && SCAN_BLOCK % 64 == 0,
              "the flag and the caps of include/mldsa_csr.h");

constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int WRITE_WAVES = 4;  // requests per workgroup of k_csr_tbs_write

__global__ __launch_bounds__(SCAN_BLOCK) void k_csr_parse(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                          const mldsa_csr_item* __restrict__ items, uint32_t n,
                                                          mldsa_csr_fields* __restrict__ fields, mldsa_rec_op* __restrict__ ops,
                                                          uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const mldsa_csr_item c = items[i];
    mldsa_csr_fields r = {};
    mldsa_rec_op op = {};  // all zero unless the request is accepted
    r.status = ST_RANGE;
    if (in_range(c.off, c.len, blob_len) && c.len >= 2) {
        const Walk w = walk(BlobBytes{blob + c.off}, c.len);
        r.status = (uint8_t)w.status;
        if (w.status != ST_DER) {
            r.cri_off = c.off + w.cri_off;
            r.cri_len = w.cri_len;
            r.subject_off = c.off + w.subject_off;
            r.subject_len = w.subject_len;
            r.spki_off = c.off + w.spki_off;
            r.spki_len = w.spki_len;
        }
        if (w.status == ST_OK) {
            r.set = (uint8_t)w.set;
            r.sig_off = c.off + w.sig_off;
            r.key_off = c.off + w.key_off;
            op.pk_off = r.key_off;
            op.sig_off = r.sig_off;
            op.msg_off = r.cri_off;
            op.msg_len = r.cri_len;
            op.set = r.set;
        }
    }
    fields[i] = r;
    ops[i] = op;
    status[i] = r.status;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_csr_check(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                          const mldsa_csr_fields* __restrict__ fields,
                                                          const mldsa_csr_issue* __restrict__ entries, const uint8_t* __restrict__ ok,
                                                          uint32_t n, uint8_t* __restrict__ status, uint32_t* __restrict__ lens,
                                                          uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[SCAN_WAVES][PLACE_SUMS];
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    uint64_t bytes = 0, count = 0;  // no request: counted nowhere
    if (i < n) {
        const mldsa_csr_fields r = fields[i];
        const mldsa_csr_issue e = entries[i];
        const int st = tbs_status(BlobBytes{blob}, blob_len, r, e, ok[i]);
        if (st == ST_OK) {
            bytes = tbs_len(e, r);
            count = 1;
        }
        status[i] = (uint8_t)st;
        lens[i] = (uint32_t)bytes;
    }
    uint64_t v[PLACE_SUMS] = {bytes, count};
    mldsa_rec::place_block_sums(v, part, sums);
}

// one wave: sums[b][q] -> the sum over the blocks before b (in place); the totals as they stand when every TBSCertificate fits
__global__ __launch_bounds__(64) void k_csr_offsets(uint64_t* __restrict__ sums, uint32_t n_blocks, uint32_t n,
                                                    mldsa_csr_totals* __restrict__ totals) {
    uint64_t total[PLACE_SUMS];
    mldsa_rec::place_block_offsets(sums, n_blocks, total);
    if (threadIdx.x == 0) mldsa_rec::place_totals(totals, n, total);
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_csr_apply(const mldsa_csr_issue* __restrict__ entries, uint32_t n, uint64_t out_len,
                                                          const uint32_t* __restrict__ lens, const uint64_t* __restrict__ sums,
                                                          mldsa_x509sign_req* __restrict__ reqs_out, uint8_t* __restrict__ status,
                                                          mldsa_csr_totals* __restrict__ totals) {
    __shared__ uint64_t part[SCAN_WAVES][PLACE_SUMS];
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int st = ST_OK;
    uint64_t bytes = 0, count = 0;
    if (i < n) {
        st = status[i];  // k_csr_check's verdict on this request
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
    const bool acc = st == ST_OK;  // every other request's row is all zero
    const mldsa_csr_issue& e = entries[i];
    mldsa_x509sign_req q = {};
    if (acc) {
        q.off = at;
        q.rnd_off = e.rnd_off;
        q.len = (uint32_t)bytes;
        q.key = e.key;
        q.issuer = e.issuer;
        q.set = e.set;
        q.flags = e.flags;
    }
    reqs_out[i] = q;
    status[i] = (uint8_t)st;
}

__global__ __launch_bounds__(64 * WRITE_WAVES) void k_csr_tbs_write(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                                    const mldsa_csr_fields* __restrict__ fields,
                                                                    const mldsa_csr_issue* __restrict__ entries, uint32_t n,
                                                                    uint8_t* __restrict__ out, uint64_t out_len,
                                                                    const mldsa_x509sign_req* __restrict__ reqs_out,
                                                                    const uint8_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    // (the wave's number as a scalar: the three rows below are then read once per wave into scalar registers, not once per lane)
    const uint32_t i = blockIdx.x * WRITE_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave: one request per wave)
    if (status[i] != ST_OK) return;
    const mldsa_csr_fields r = fields[i];
    const mldsa_csr_issue e = entries[i];
    const mldsa_x509sign_req q = reqs_out[i];
    // Every range is checked again, and the row against the entry: only then is an offset followed or a byte written.
    if (!write_allowed(r, e, q.off, q.len, blob_len, out_len)) return;
    const Pieces p = pieces(e, r);
    uint8_t* tbs = out + q.off;
    if (lane < (int)PREFIX_LEN) tbs[lane] = (uint8_t)prefix_byte(lane, q.len, e.serial_len);
    if (lane < (int)ALG_LEN) tbs[p.alg_at + lane] = (uint8_t)alg_byte(lane, class_of_set(e.set));
    const uint32_t mis = (uint32_t)((uintptr_t)blob & 15);
#pragma unroll
    for (int k = 0; k < 6; ++k) copy_field(blob - mis, mis, blob_len, piece_off(e, r, k), p.len[k], tbs + p.at[k], lane);
}

// ------------------------------------------------------------------------------------------------------------ host side
// the checks the entry points share; the message names what failed
int check_common_args(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, size_t n) {
    if (n > MLDSA_CSR_MAX_REQUESTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_CSR_MAX_REQUESTS requests");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (!blob && blob_len != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    return MLDSA_OK;
}

int check_rows(const char* fn, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries, const mldsa_x509sign_req* reqs_out,
               const uint8_t* status) {
    if (!fields || !entries || !reqs_out || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(fields, 8) || !aligned(entries, 8) || !aligned(reqs_out, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": fields, entries and reqs_out must be 8-byte aligned");
    return MLDSA_OK;
}

int check_plan(const char* fn, const uint8_t* ok, size_t n, const mldsa_csr_totals* totals, const void* plan, size_t bytes) {
    if (!ok || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(totals, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": totals must be 8-byte aligned");
    if (!plan || !aligned(plan, 256) || bytes < plan_bytes(n))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": plan is NULL, not 256-byte aligned or smaller than mldsa_csr_plan_bytes");
    return MLDSA_OK;
}

int check_write(const char* fn, const uint8_t* blob, uint64_t blob_len, const uint8_t* out, uint64_t out_len) {
    if (!out && out_len != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!ranges_apart(blob, blob_len, out, out_len)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": out overlaps the blob");
    return MLDSA_OK;
}

// every check is the caller's: 1 <= n <= MLDSA_CSR_MAX_REQUESTS, the current device is the context's
int launch_plan(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries,
                const uint8_t* ok, size_t n_reqs, uint64_t out_len, mldsa_x509sign_req* reqs_out, uint8_t* status, mldsa_csr_totals* totals,
                void* plan, hipStream_t s) {
    uint8_t* base = static_cast<uint8_t*>(plan);
    uint64_t* sums = reinterpret_cast<uint64_t*>(base);
    uint32_t* lens = reinterpret_cast<uint32_t*>(base + plan_sums_bytes(n_reqs));
    const uint32_t n = (uint32_t)n_reqs, nb = (uint32_t)n_blocks(n_reqs);
    hipLaunchKernelGGL(k_csr_check, dim3(nb), dim3(SCAN_BLOCK), 0, s, blob, blob_len, fields, entries, ok, n, status, lens, sums);
    hipLaunchKernelGGL(k_csr_offsets, dim3(1), dim3(64), 0, s, sums, nb, n, totals);
    hipLaunchKernelGGL(k_csr_apply, dim3(nb), dim3(SCAN_BLOCK), 0, s, entries, n, out_len, lens, sums, reqs_out, status, totals);
    LAYER_LAUNCHED("plan launch");
    return MLDSA_OK;
}

int launch_write(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries,
                 size_t n_reqs, uint8_t* out, uint64_t out_len, const mldsa_x509sign_req* reqs_out, const uint8_t* status, hipStream_t s) {
    const uint32_t n = (uint32_t)n_reqs;
    hipLaunchKernelGGL(k_csr_tbs_write, dim3((n + WRITE_WAVES - 1) / WRITE_WAVES), dim3(64 * WRITE_WAVES), 0, s, blob, blob_len, fields,
                       entries, n, out, out_len, reqs_out, status);
    LAYER_LAUNCHED("k_csr_tbs_write launch");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_csr_abi_version(void) { return MLDSA_CSR_ABI_VERSION; }

const char* mldsa_csr_last_error(void) { return g_err.c_str(); }

size_t mldsa_csr_tbs_len(int set, size_t serial_len, size_t issuer_len, size_t validity_len, size_t subject_len, size_t spki_len,
                         size_t ext_len) {
    const int c = class_of_set((uint32_t)set);
    if (set < 0 || c == CLASS_REFUSED || serial_len == 0 || serial_len > SERIAL_MAX) return 0;
    size_t total = FIXED_LEN + serial_len;
    for (const size_t part : {issuer_len, validity_len, subject_len, spki_len, ext_len}) {
        if (part > max_tbs_len(c)) return 0;  // (and so no sum below wraps)
        total += part;
    }
    return total > max_tbs_len(c) ? 0 : total;
}

size_t mldsa_csr_plan_bytes(size_t n) { return plan_bytes(n); }

int mldsa_csr_parse(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_item* items, size_t n, mldsa_csr_fields* fields,
                    mldsa_rec_op* ops, uint8_t* status, void* stream) {
    const char* fn = "mldsa_csr_parse";
    if (n == 0) return MLDSA_OK;
    const int rc = check_common_args(fn, ctx, blob, blob_len, n);
    if (rc != MLDSA_OK) return rc;
    if (!items || !fields || !ops || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(items, 8) || !aligned(fields, 8) || !aligned(ops, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": items, fields and ops must be 8-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_csr_parse, dim3((unsigned)n_blocks(n)), dim3(SCAN_BLOCK), 0, (hipStream_t)stream, blob, blob_len, items, (uint32_t)n,
                       fields, ops, status);
    LAYER_LAUNCHED("k_csr_parse launch");
    return MLDSA_OK;
}

int mldsa_csr_tbs_plan(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries,
                       const uint8_t* ok, size_t n, uint64_t out_len, mldsa_x509sign_req* reqs_out, uint8_t* status, mldsa_csr_totals* totals,
                       void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_csr_tbs_plan";
    if (n == 0) return MLDSA_OK;
    int rc = check_common_args(fn, ctx, blob, blob_len, n);
    if (rc == MLDSA_OK) rc = check_rows(fn, fields, entries, reqs_out, status);
    if (rc == MLDSA_OK) rc = check_plan(fn, ok, n, totals, plan, plan_bytes);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_plan(fn, blob, blob_len, fields, entries, ok, n, out_len, reqs_out, status, totals, plan, (hipStream_t)stream);
}

int mldsa_csr_tbs_write(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries,
                        size_t n, uint8_t* out, uint64_t out_len, const mldsa_x509sign_req* reqs_out, const uint8_t* status, void* stream) {
    const char* fn = "mldsa_csr_tbs_write";
    if (n == 0) return MLDSA_OK;
    int rc = check_common_args(fn, ctx, blob, blob_len, n);
    if (rc == MLDSA_OK) rc = check_rows(fn, fields, entries, reqs_out, status);
    if (rc == MLDSA_OK) rc = check_write(fn, blob, blob_len, out, out_len);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_write(fn, blob, blob_len, fields, entries, n, out, out_len, reqs_out, status, (hipStream_t)stream);
}

int mldsa_csr_tbs(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields* fields, const mldsa_csr_issue* entries,
                  const uint8_t* ok, size_t n, uint8_t* out, uint64_t out_len, mldsa_x509sign_req* reqs_out, uint8_t* status,
                  mldsa_csr_totals* totals, void* plan, size_t plan_bytes, void* stream) {
    const char* fn = "mldsa_csr_tbs";
    if (n == 0) return MLDSA_OK;
    int rc = check_common_args(fn, ctx, blob, blob_len, n);
    if (rc == MLDSA_OK) rc = check_rows(fn, fields, entries, reqs_out, status);
    if (rc == MLDSA_OK) rc = check_plan(fn, ok, n, totals, plan, plan_bytes);
    if (rc == MLDSA_OK) rc = check_write(fn, blob, blob_len, out, out_len);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    rc = launch_plan(fn, blob, blob_len, fields, entries, ok, n, out_len, reqs_out, status, totals, plan, (hipStream_t)stream);
    if (rc != MLDSA_OK) return rc;
    return launch_write(fn, blob, blob_len, fields, entries, n, out, out_len, reqs_out, status, (hipStream_t)stream);
}

}  // extern "C"
