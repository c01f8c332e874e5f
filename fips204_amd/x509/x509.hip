// libmldsa_x509.so (include/mldsa_x509.h): X.509 certificates in a blob to mldsa_rec_op descriptors -- the DER walk of every
// certificate and the link to its issuer's key on the device, in front of mldsa_rec_verify (which this library neither links nor calls).
//
// Two launches, ordered by the kernel boundary alone: no wave waits for another.
//   k_x509_parse  one certificate per lane, PARSE_BLOCK lanes per workgroup: the range check and the walk of x509_plan.h on the blob, one
//                 mldsa_x509_fields row per certificate.  The walk is a chain of about 14 dependent loads of a few bytes each; a lane
//                 has one such chain, so the launch keeps as many in flight as there are lanes.
//   k_x509_link   one certificate per wave, LINK_WAVES per workgroup: lane 0 reads the certificate's row and its issuer's row and
//                 decides by the link rule of x509_plan.h, the decision is broadcast, and with CHECK_NAMES the wave compares the two
//                 Name TLVs 64 bytes per step (one byte of each per lane, OR-reduced).  Lane 0 writes ops[i] and status[i].  The
//                 comparison and the op's write are those of x509_dev.h, which k_crl_link shares.
// What bounds them: latency of the dependent loads in k_x509_parse; k_x509_link reads two 56-byte rows and two Names and writes 41 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_x509.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"
#include "x509_dev.h"
#include "x509_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_x509;

static_assert(sizeof(mldsa_x509_cert) == 16 && sizeof(mldsa_x509_fields) == 56 && sizeof(mldsa_rec_op) == 40, "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_ALG == MLDSA_X509_ALG &&
                  ST_SIG == MLDSA_X509_SIG && ST_ISSUER == MLDSA_X509_ISSUER && ST_NAME == MLDSA_X509_NAME &&
                  ST_PARSE_ONLY == MLDSA_X509_PARSE_ONLY, "the status codes of include/mldsa_x509.h");
static_assert(FLAG_CHECK_NAMES == MLDSA_X509_CHECK_NAMES && NO_ISSUER == MLDSA_X509_NO_ISSUER && MLDSA_X509_MAX_CERTS < NO_ISSUER,
              "the flag and the issuer sentinel of include/mldsa_x509.h");

constexpr int PARSE_BLOCK = 256;  // certificates per workgroup of k_x509_parse
constexpr int LINK_WAVES = 4;     // certificates per workgroup of k_x509_link

__global__ __launch_bounds__(PARSE_BLOCK) void k_x509_parse(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                            const mldsa_x509_cert* __restrict__ certs, uint32_t n,
                                                            mldsa_x509_fields* __restrict__ fields) {
    const uint32_t i = blockIdx.x * PARSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const mldsa_x509_cert c = certs[i];
    mldsa_x509_fields r = {};
    r.status = ST_RANGE;
    if (in_range(c.off, c.len, blob_len) && c.len >= 2) {
        const Walk w = walk(BlobBytes{blob + c.off}, c.len);
        r.status = (uint8_t)w.status;
        if (w.status != ST_DER) {
            r.tbs_off = c.off + w.tbs_off;
            r.tbs_len = w.tbs_len;
            r.issuer_off = c.off + w.issuer_off;
            r.issuer_len = w.issuer_len;
            r.subject_off = c.off + w.subject_off;
            r.subject_len = w.subject_len;
            r.sig_set = (uint8_t)w.sig_set;
            r.key_set = (uint8_t)w.key_set;
            if (w.sig_set != 0) r.sig_off = c.off + w.sig_off;
            if (w.key_set != 0) r.key_off = c.off + w.key_off;
        }
    }
    fields[i] = r;
}

__global__ __launch_bounds__(64 * LINK_WAVES) void k_x509_link(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                               const mldsa_x509_cert* __restrict__ certs,
                                                               const mldsa_x509_fields* __restrict__ fields, uint32_t n, uint32_t flags,
                                                               mldsa_rec_op* __restrict__ ops, uint8_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * LINK_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave: one certificate per wave)
    int st = ST_OK;
    uint64_t mine = 0, theirs = 0;  // the two Names, where they are to be compared
    uint32_t name_len = 0;
    uint64_t pk_off = 0, sig_off = 0, tbs_off = 0;  // the op of an accepted certificate
    uint32_t tbs_len = 0, set = 0;
    if (lane == 0) {
        const mldsa_x509_fields& own = fields[i];
        const uint32_t issuer = certs[i].issuer;
        const mldsa_x509_fields& iss = fields[issuer < n ? issuer : i];  // the issuer's row, never its DER; read only where issuer < n
        set = own.sig_set;
        st = link_status(own.status, set, issuer, n, issuer < n ? iss.status : 0, issuer < n ? iss.key_set : 0);
        if (st == ST_OK) {
            pk_off = iss.key_off;
            sig_off = own.sig_off;
            tbs_off = own.tbs_off;
            tbs_len = own.tbs_len;
            if ((flags & FLAG_CHECK_NAMES) != 0) {
                const uint64_t a = own.issuer_off, b = iss.subject_off;
                const uint32_t a_len = own.issuer_len, b_len = iss.subject_len;
                // a row that points outside the blob is not followed: it counts as a mismatch, like Names of different lengths
                if (a_len != b_len || !in_range(a, a_len, blob_len) || !in_range(b, b_len, blob_len)) {
                    st = ST_NAME;
                } else {
                    mine = a;
                    theirs = b;
                    name_len = a_len;
                }
            }
        }
    }
    st = __shfl(st, 0, 64);
    mine = __shfl((unsigned long long)mine, 0, 64);
    theirs = __shfl((unsigned long long)theirs, 0, 64);
    name_len = (uint32_t)__shfl((int)name_len, 0, 64);
    if (wave_names_differ(blob, mine, theirs, name_len, lane)) st = ST_NAME;
    if (lane == 0) {
        write_link_op(ops[i], st == ST_OK, pk_off, sig_off, tbs_off, tbs_len, set);  // every other certificate's op is all zero
        status[i] = (uint8_t)st;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
// the checks the entry points share; the message names what failed
int check_certs(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, size_t n,
                const mldsa_x509_fields* fields) {
    if (n > MLDSA_X509_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_X509_MAX_CERTS certificates");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if ((!blob && blob_len != 0) || !certs || !fields) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(fields, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs and fields must be 8-byte aligned");
    return MLDSA_OK;
}

int check_link(const char* fn, unsigned flags, const mldsa_rec_op* ops, const uint8_t* status) {
    if (!ops || !status) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(ops, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": ops must be 8-byte aligned");
    if ((flags & ~MLDSA_X509_CHECK_NAMES) != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown flag");
    return MLDSA_OK;
}

// every check is the caller's: 1 <= n <= MLDSA_X509_MAX_CERTS, the current device is the context's
int launch_parse(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, size_t n, mldsa_x509_fields* fields,
                 hipStream_t s) {
    hipLaunchKernelGGL(k_x509_parse, dim3((unsigned)((n + PARSE_BLOCK - 1) / PARSE_BLOCK)), dim3(PARSE_BLOCK), 0, s, blob, blob_len, certs,
                       (uint32_t)n, fields);
    LAYER_LAUNCHED("k_x509_parse launch");
    return MLDSA_OK;
}

int launch_link(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields,
                size_t n, unsigned flags, mldsa_rec_op* ops, uint8_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_x509_link, dim3((unsigned)((n + LINK_WAVES - 1) / LINK_WAVES)), dim3(64 * LINK_WAVES), 0, s, blob, blob_len, certs,
                       fields, (uint32_t)n, (uint32_t)flags, ops, status);
    LAYER_LAUNCHED("k_x509_link launch");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_x509_abi_version(void) { return MLDSA_X509_ABI_VERSION; }

const char* mldsa_x509_last_error(void) { return g_err.c_str(); }

int mldsa_x509_parse(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, size_t n, mldsa_x509_fields* fields,
                     void* stream) {
    const char* fn = "mldsa_x509_parse";
    if (n == 0) return MLDSA_OK;
    const int rc = check_certs(fn, ctx, blob, blob_len, certs, n, fields);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_parse(fn, blob, blob_len, certs, n, fields, (hipStream_t)stream);
}

int mldsa_x509_link(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields,
                    size_t n, unsigned flags, mldsa_rec_op* ops, uint8_t* status, void* stream) {
    const char* fn = "mldsa_x509_link";
    if (n == 0) return MLDSA_OK;
    int rc = check_certs(fn, ctx, blob, blob_len, certs, n, fields);
    if (rc == MLDSA_OK) rc = check_link(fn, flags, ops, status);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_link(fn, blob, blob_len, certs, fields, n, flags, ops, status, (hipStream_t)stream);
}

int mldsa_x509_ops(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, size_t n, unsigned flags,
                   mldsa_x509_fields* fields, mldsa_rec_op* ops, uint8_t* status, void* stream) {
    const char* fn = "mldsa_x509_ops";
    if (n == 0) return MLDSA_OK;
    int rc = check_certs(fn, ctx, blob, blob_len, certs, n, fields);
    if (rc == MLDSA_OK) rc = check_link(fn, flags, ops, status);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    rc = launch_parse(fn, blob, blob_len, certs, n, fields, (hipStream_t)stream);
    if (rc != MLDSA_OK) return rc;
    return launch_link(fn, blob, blob_len, certs, fields, n, flags, ops, status, (hipStream_t)stream);
}

}  // extern "C"
