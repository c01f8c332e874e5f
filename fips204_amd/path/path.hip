// libmldsa_path.so (include/mldsa_path.h): the last leg of X.509 path validation -- validity dates, the CA constraints of the
// extensions, the freshness of the CRLs and one verdict per certificate for its whole chain.  This library links and calls none of the
// other layers; it reads the rows that libmldsa_x509.so and libmldsa_crl.so wrote.
//
// Five kernels, one item per lane each, PATH_BLOCK lanes per workgroup; the two of mldsa_path_chain are ordered by the kernel boundary
// alone: no wave waits for another.
//   k_path_times      one Time TLV per lane: parse_time of path_plan.h on at most 17 bytes of the blob.
//   k_path_parse      one certificate per lane, as k_x509_parse: the range check and walk_policy on the blob, one mldsa_path_fields row.
//   k_path_crl_times  one CRL per lane: the two Times at the offsets of its mldsa_crl_fields row and the freshness rule.
//   k_path_node       one certificate per lane: the rules it breaks for itself and as an issuer, folded into one 8-byte node.
//   k_path_climb      one certificate per lane: at most MAX_DEPTH + 1 dependent 8-byte node reads up to the anchor.
// What bounds them: latency of the walk's dependent loads in k_path_parse, and lanes of one wave that leave the extension loop at
// different counts wait for the longest; k_path_climb is a chain of random 8-byte reads in an array that mostly stays in L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_path.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"
#include "../x509/x509_dev.h"
#include "path_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_path;
using mldsa_x509::BlobBytes;

static_assert(sizeof(mldsa_path_fields) == FIELDS_BYTES && offsetof(mldsa_path_fields, not_after) == FIELDS_NOT_AFTER &&
                  offsetof(mldsa_path_fields, ext_off) == FIELDS_EXT_OFF && offsetof(mldsa_path_fields, crit_off) == FIELDS_CRIT_OFF &&
                  offsetof(mldsa_path_fields, ext_len) == FIELDS_EXT_LEN && offsetof(mldsa_path_fields, path_len) == FIELDS_PATH_LEN &&
                  offsetof(mldsa_path_fields, key_usage) == FIELDS_KEY_USAGE && offsetof(mldsa_path_fields, flags) == FIELDS_FLAGS &&
                  offsetof(mldsa_path_fields, n_ext) == FIELDS_N_EXT && offsetof(mldsa_path_fields, status) == FIELDS_STATUS &&
                  sizeof(mldsa_path_result) == RESULT_BYTES && offsetof(mldsa_path_result, verdict) == RESULT_VERDICT &&
                  offsetof(mldsa_path_result, depth) == RESULT_DEPTH && sizeof(mldsa_x509_cert) == 16 && sizeof(mldsa_crl_fields) == 88,
              "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_VERSION == MLDSA_PATH_VERSION &&
                  ST_TIME == MLDSA_PATH_TIME && ST_EXT == MLDSA_PATH_EXT && ST_CRITICAL == MLDSA_PATH_CRITICAL && MLDSA_PATH_VERSION > MLDSA_CRL_SPACE,
              "the status codes of include/mldsa_path.h and include/mldsa_x509.h");
static_assert(V_TRUSTED == MLDSA_PATH_TRUSTED && V_CERT == MLDSA_PATH_CERT && V_SIG == MLDSA_PATH_SIG && V_POLICY == MLDSA_PATH_POLICY &&
                  V_NOT_YET == MLDSA_PATH_NOT_YET && V_EXPIRED == MLDSA_PATH_EXPIRED && V_REVOKED == MLDSA_PATH_REVOKED &&
                  V_REVOCATION == MLDSA_PATH_REVOCATION && V_NOT_CA == MLDSA_PATH_NOT_CA && V_KEY_USAGE == MLDSA_PATH_KEY_USAGE &&
                  V_PATH_LEN == MLDSA_PATH_PATH_LEN && V_NO_ANCHOR == MLDSA_PATH_NO_ANCHOR && V_DEPTH == MLDSA_PATH_DEPTH,
              "the verdicts of include/mldsa_path.h");
static_assert(CRL_FRESH == MLDSA_PATH_CRL_FRESH && CRL_REFUSED == MLDSA_PATH_CRL_REFUSED && CRL_TIME == MLDSA_PATH_CRL_TIME &&
                  CRL_NOT_YET == MLDSA_PATH_CRL_NOT_YET && CRL_STALE == MLDSA_PATH_CRL_STALE && REV_GOOD == MLDSA_CRL_GOOD &&
                  REV_REVOKED == MLDSA_CRL_REVOKED && REV_NO_CRL == MLDSA_CRL_NO_CRL,
              "the CRL codes of include/mldsa_path.h and include/mldsa_crl.h");
static_assert(FLAG_ALLOW_UNKNOWN_CRITICAL == MLDSA_PATH_ALLOW_UNKNOWN_CRITICAL && FLAG_REQUIRE_NEXT_UPDATE == MLDSA_PATH_REQUIRE_NEXT_UPDATE &&
                  FLAG_ALLOW_NO_CRL == MLDSA_PATH_ALLOW_NO_CRL && F_V3 == MLDSA_PATH_V3 && F_HAS_BC == MLDSA_PATH_HAS_BC &&
                  F_IS_CA == MLDSA_PATH_IS_CA && F_HAS_KU == MLDSA_PATH_HAS_KU && MAX_EXTS == MLDSA_PATH_MAX_EXTS &&
                  MAX_DEPTH == MLDSA_PATH_MAX_DEPTH && NO_PATH_LEN == MLDSA_PATH_NO_PATH_LEN && MAX_CERTS == MLDSA_PATH_MAX_CERTS &&
                  NO_ISSUER == MLDSA_X509_NO_ISSUER && MAX_EXTS <= 255 && MAX_DEPTH <= 255,
              "the flags and the caps of include/mldsa_path.h; n_ext and depth are one byte each");

constexpr int PATH_BLOCK = 256;  // items per workgroup of every kernel here

// packed node a of the scratch array; climb vouches for a < n
struct Nodes {
    const uint64_t* at;
    __host__ __device__ __forceinline__ uint64_t operator()(uint32_t a) const { return at[a]; }
};

// the Time TLV at blob offset off, read through at most TIME_TLV_MAX bytes and never behind the blob's end; *in_blob: two bytes at
// least lie inside the blob
__device__ __forceinline__ Time time_at(const uint8_t* __restrict__ blob, uint64_t blob_len, uint64_t off, bool* in_blob) {
    *in_blob = in_range(off, 2, blob_len);
    if (!*in_blob) return Time{};
    const uint64_t room = blob_len - off;
    return parse_time(BlobBytes{blob + off}, 0, room < TIME_TLV_MAX ? (uint32_t)room : TIME_TLV_MAX);
}

__global__ __launch_bounds__(PATH_BLOCK) void k_path_times(const uint8_t* __restrict__ blob, uint64_t blob_len, const uint64_t* __restrict__ offs,
                                                           uint32_t n, int64_t* __restrict__ seconds, uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * PATH_BLOCK + threadIdx.x;
    if (i >= n) return;
    bool in_blob = false;
    const Time t = time_at(blob, blob_len, offs[i], &in_blob);
    seconds[i] = t.ok ? t.seconds : 0;
    status[i] = (uint8_t)(!in_blob ? ST_RANGE : t.ok ? ST_OK : ST_TIME);
}

__global__ __launch_bounds__(PATH_BLOCK) void k_path_parse(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                           const mldsa_x509_cert* __restrict__ certs, uint32_t n, uint32_t flags,
                                                           mldsa_path_fields* __restrict__ fields) {
    const uint32_t i = blockIdx.x * PATH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const mldsa_x509_cert c = certs[i];
    mldsa_path_fields r = {};
    r.status = ST_RANGE;
    if (in_range(c.off, c.len, blob_len) && c.len >= 2) {
        const Policy w = walk_policy(BlobBytes{blob + c.off}, c.len, flags);
        r.status = (uint8_t)w.status;
        if (w.status != ST_DER) {
            r.not_before = w.not_before;
            r.not_after = w.not_after;
            if (w.ext_off != 0) r.ext_off = c.off + w.ext_off;
            if (w.crit_off != 0) r.crit_off = c.off + w.crit_off;
            r.ext_len = w.ext_len;
            r.path_len = w.path_len;
            r.key_usage = (uint16_t)w.key_usage;
            r.flags = (uint8_t)w.flags;
            r.n_ext = (uint8_t)w.n_ext;
        }
    }
    fields[i] = r;
}

__global__ __launch_bounds__(PATH_BLOCK) void k_path_crl_times(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                               const mldsa_crl_fields* __restrict__ crl_fields,
                                                               const uint8_t* __restrict__ crl_status, const uint8_t* __restrict__ crl_ok, uint32_t n,
                                                               int64_t now, uint32_t flags, int64_t* __restrict__ this_s,
                                                               int64_t* __restrict__ next_s, uint8_t* __restrict__ time_status,
                                                               uint8_t* __restrict__ fresh_ok) {
    const uint32_t c = blockIdx.x * PATH_BLOCK + threadIdx.x;
    if (c >= n) return;
    const bool accepted = crl_status[c] == ST_OK && crl_fields[c].status == ST_OK;
    Time t0, t1;
    bool times_ok = false, has_next = false;
    if (accepted) {  // only then is an offset of the row followed
        const uint64_t this_off = crl_fields[c].this_off, next_off = crl_fields[c].next_off;
        bool in_blob = false;
        t0 = time_at(blob, blob_len, this_off, &in_blob);
        has_next = next_off != 0;
        if (has_next) t1 = time_at(blob, blob_len, next_off, &in_blob);
        times_ok = t0.ok && (!has_next || t1.ok);
    }
    const int st = crl_time_status(accepted, times_ok, t0.seconds, has_next, t1.seconds, now, flags);
    this_s[c] = t0.ok ? t0.seconds : 0;
    next_s[c] = t1.ok ? t1.seconds : 0;
    time_status[c] = (uint8_t)st;
    fresh_ok[c] = (crl_ok == nullptr || crl_ok[c] != 0) && st == CRL_FRESH ? 1 : 0;
}

__global__ __launch_bounds__(PATH_BLOCK) void k_path_node(const mldsa_x509_cert* __restrict__ certs, const mldsa_path_fields* __restrict__ policy,
                                                          const uint8_t* __restrict__ cert_status, const uint8_t* __restrict__ cert_ok,
                                                          const uint8_t* __restrict__ revocation, const uint8_t* __restrict__ anchor, uint32_t n,
                                                          int64_t now, uint32_t flags, uint64_t* __restrict__ nodes) {
    const uint32_t i = blockIdx.x * PATH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const mldsa_path_fields p = policy[i];
    const int own = own_rule(cert_status[i], cert_ok[i] != 0, p.status, p.not_before, p.not_after, revocation != nullptr,
                             revocation != nullptr ? revocation[i] : 0, now, flags);
    nodes[i] = pack_node(node_of(certs[i].issuer, own, issuer_rule(p.flags, p.key_usage), p.path_len, anchor[i] != 0));
}

__global__ __launch_bounds__(PATH_BLOCK) void k_path_climb(const uint64_t* __restrict__ nodes, uint32_t n, mldsa_path_result* __restrict__ results) {
    const uint32_t i = blockIdx.x * PATH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Result r = climb(Nodes{nodes}, i, n);
    mldsa_path_result out = {};
    out.where = r.where;
    out.verdict = (uint8_t)r.verdict;
    out.depth = (uint8_t)r.depth;
    results[i] = out;
}

// ------------------------------------------------------------------------------------------------------------ host side
// the checks the entry points share; the message names what failed
int check_batch(const char* fn, const mldsa_ctx* ctx, size_t n, size_t cap, const char* cap_what) {
    if (n > cap) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than " + cap_what);
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    return MLDSA_OK;
}

int check_flags(const char* fn, unsigned flags, unsigned known) {
    if ((flags & ~known) != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown flag");
    return MLDSA_OK;
}

unsigned grid(size_t n) { return (unsigned)((n + PATH_BLOCK - 1) / PATH_BLOCK); }

}  // namespace

extern "C" {

int mldsa_path_abi_version(void) { return MLDSA_PATH_ABI_VERSION; }

const char* mldsa_path_last_error(void) { return g_err.c_str(); }

size_t mldsa_path_scratch_bytes(size_t n) { return scratch_bytes(n); }

int mldsa_path_times(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const uint64_t* offs, size_t n, int64_t* seconds, uint8_t* status,
                     void* stream) {
    const char* fn = "mldsa_path_times";
    if (n == 0) return MLDSA_OK;
    const int rc = check_batch(fn, ctx, n, MLDSA_PATH_MAX_CERTS, "MLDSA_PATH_MAX_CERTS Times");
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !offs || !seconds || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(offs, 8) || !aligned(seconds, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": offs and seconds must be 8-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_path_times, dim3(grid(n)), dim3(PATH_BLOCK), 0, (hipStream_t)stream, blob, blob_len, offs, (uint32_t)n, seconds, status);
    LAYER_LAUNCHED("k_path_times launch");
    return MLDSA_OK;
}

int mldsa_path_parse(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, size_t n, unsigned flags,
                     mldsa_path_fields* fields, void* stream) {
    const char* fn = "mldsa_path_parse";
    if (n == 0) return MLDSA_OK;
    int rc = check_batch(fn, ctx, n, MLDSA_PATH_MAX_CERTS, "MLDSA_PATH_MAX_CERTS certificates");
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !certs || !fields) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(fields, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs and fields must be 8-byte aligned");
    rc = check_flags(fn, flags, MLDSA_PATH_ALLOW_UNKNOWN_CRITICAL);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_path_parse, dim3(grid(n)), dim3(PATH_BLOCK), 0, (hipStream_t)stream, blob, blob_len, certs, (uint32_t)n, (uint32_t)flags,
                       fields);
    LAYER_LAUNCHED("k_path_parse launch");
    return MLDSA_OK;
}

int mldsa_path_crl_times(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_fields* crl_fields, const uint8_t* crl_status,
                         const uint8_t* crl_ok, size_t n_crls, int64_t now, unsigned flags, int64_t* this_s, int64_t* next_s, uint8_t* time_status,
                         uint8_t* fresh_ok, void* stream) {
    const char* fn = "mldsa_path_crl_times";
    if (n_crls == 0) return MLDSA_OK;
    int rc = check_batch(fn, ctx, n_crls, MLDSA_CRL_MAX_CRLS, "MLDSA_CRL_MAX_CRLS CRLs");
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !crl_fields || !crl_status || !this_s || !next_s || !time_status || !fresh_ok)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(crl_fields, 8) || !aligned(this_s, 8) || !aligned(next_s, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": crl_fields, this_s and next_s must be 8-byte aligned");
    rc = check_flags(fn, flags, MLDSA_PATH_REQUIRE_NEXT_UPDATE);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_path_crl_times, dim3(grid(n_crls)), dim3(PATH_BLOCK), 0, (hipStream_t)stream, blob, blob_len, crl_fields, crl_status, crl_ok,
                       (uint32_t)n_crls, now, (uint32_t)flags, this_s, next_s, time_status, fresh_ok);
    LAYER_LAUNCHED("k_path_crl_times launch");
    return MLDSA_OK;
}

int mldsa_path_chain(mldsa_ctx* ctx, const mldsa_x509_cert* certs, const mldsa_path_fields* policy, const uint8_t* cert_status,
                     const uint8_t* cert_ok, const uint8_t* revocation, const uint8_t* anchor, size_t n, int64_t now, unsigned flags,
                     mldsa_path_result* results, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_path_chain";
    if (n == 0) return MLDSA_OK;
    int rc = check_batch(fn, ctx, n, MLDSA_PATH_MAX_CERTS, "MLDSA_PATH_MAX_CERTS certificates");
    if (rc != MLDSA_OK) return rc;
    if (!certs || !policy || !cert_status || !cert_ok || !anchor || !results) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(policy, 8) || !aligned(results, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs, policy and results must be 8-byte aligned");
    rc = check_flags(fn, flags, MLDSA_PATH_ALLOW_NO_CRL);
    if (rc != MLDSA_OK) return rc;
    if (!scratch || !aligned(scratch, 256) || scratch_bytes < mldsa_path::scratch_bytes(n))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_path_scratch_bytes");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint64_t* nodes = static_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(k_path_node, dim3(grid(n)), dim3(PATH_BLOCK), 0, s, certs, policy, cert_status, cert_ok, revocation, anchor, (uint32_t)n, now,
                       (uint32_t)flags, nodes);
    LAYER_LAUNCHED("k_path_node launch");
    hipLaunchKernelGGL(k_path_climb, dim3(grid(n)), dim3(PATH_BLOCK), 0, s, nodes, (uint32_t)n, results);
    LAYER_LAUNCHED("k_path_climb launch");
    return MLDSA_OK;
}

}  // extern "C"
