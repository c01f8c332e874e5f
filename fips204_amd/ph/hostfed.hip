// HashML-DSA from host memory (include/mldsa_ph.h: mldsa_ph_host_*, mldsa_hash_verify_host, mldsa_hash_sign_host).
//
// The raw message bytes [msg_off[0], msg_off[n_ops]) stream through the layers' host-memory feed (../layer/host_feed.h): two
// staging chunks of `staging_bytes` each, cut at arbitrary byte positions; chunk i + 1 is uploaded on the copy stream while
// k_ph_update absorbs chunk i on the compute stream.  The ops that have bytes in a chunk are a contiguous range of ops; the update is launched for that range only,
// with the chunk as the window of message offsets (launch_update), so a chunk costs the waves of its own ops and the one
// offset table uploaded at the start of the call serves every chunk.  The host waits only to get a staging chunk back.
// After mldsa_ph_final the rows OID || PH(M) (43 / 75 bytes per op) come to the host and the core's own host-memory call
// does the rest in MLDSA_MODE_PREHASH: verdicts, signatures, statuses and refusals are the core's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/mldsa_ph.h"
#include "../layer/host_feed.h"
#include "ph_internal.h"

struct mldsa_ph_host {
    mldsa_ctx* ctx = nullptr;
    std::mutex mu;  // one call at a time
    mldsa_layer::HostFeed feed;
    // per-call buffers, kept and grown: offsets, states, rows on the device; rows and their offsets on the host
    size_t cap_ops = 0;
    uint64_t* d_off = nullptr;
    uint32_t* d_state = nullptr;
    uint8_t* d_rows = nullptr;
    uint8_t* h_rows = nullptr;
    uint64_t* h_row_off = nullptr;
};

namespace {

using mldsa_layer::Chunk;
using mldsa_ph::core_failed;
using mldsa_ph::fail;
using mldsa_ph::row_len_of;

constexpr int MAX_ROW = 75;

// a failed HIP runtime call, into this library's error slot (the scaffold's hip_failed writes the scaffold's)
int hip_failed(const char* fn, const char* what, hipError_t e) {
    return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
}

void release_rows(mldsa_ph_host* h) {
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->h_rows) (void)hipHostFree(h->h_rows);
    if (h->h_row_off) (void)hipHostFree(h->h_row_off);
    h->d_off = nullptr, h->d_state = nullptr, h->d_rows = nullptr, h->h_rows = nullptr, h->h_row_off = nullptr;
    h->cap_ops = 0;
}

// buffers for n_ops operations of any PH (rows are sized for the longest row)
int reserve(mldsa_ph_host* h, size_t n_ops) {
    size_t need_state = 0;
    for (int ph : mldsa_ph::ALL_PH) need_state = std::max(need_state, mldsa_ph::state_bytes_of(ph, n_ops));
    if (need_state == 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_*_host: n_ops too large");
    if (n_ops <= h->cap_ops) return MLDSA_OK;
    release_rows(h);
    if (hipMalloc((void**)&h->d_off, 8 * (n_ops + 1)) != hipSuccess || hipMalloc((void**)&h->d_state, need_state) != hipSuccess ||
        hipMalloc((void**)&h->d_rows, n_ops * MAX_ROW) != hipSuccess ||
        hipHostMalloc((void**)&h->h_rows, n_ops * MAX_ROW, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&h->h_row_off, 8 * (n_ops + 1), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MLDSA_ERR_NOMEM, "mldsa_hash_*_host: allocation of the per-call buffers failed");
    }
    h->cap_ops = n_ops;
    return MLDSA_OK;
}

int stream_rows(const char* fn, mldsa_ph_host* h, int ph, const uint8_t* msgs, const uint64_t* msg_off, size_t n_ops) {
    int rc = reserve(h, n_ops);
    if (rc != MLDSA_OK) return rc;
    const hipStream_t s = h->feed.compute;
    const size_t rl = (size_t)row_len_of(ph);
    hipError_t e = hipMemcpyAsync(h->d_off, msg_off, 8 * (n_ops + 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_failed(fn, "upload of msg_off", e);
    rc = mldsa_ph::launch_init(ph, h->d_state, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    // every chunk is the window of message offsets for the ops that have bytes in it (the table was checked by the caller)
    const mldsa_layer::FeedEnd end = h->feed.run(msgs, msg_off, n_ops, [&](const Chunk& c, const uint8_t* d_chunk) {
        return mldsa_ph::launch_update(ph, h->d_state, d_chunk, h->d_off, n_ops, c.first, c.last - c.first, c.lo, c.hi, c.lo, s);
    });
    if (end.hip != hipSuccess) return hip_failed(fn, end.step, end.hip);
    if (end.rc != MLDSA_OK) return end.rc;
    rc = mldsa_ph::launch_final(ph, h->d_state, h->d_rows, nullptr, nullptr, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    e = hipMemcpyAsync(h->h_rows, h->d_rows, n_ops * rl, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return hip_failed(fn, "download of the rows", e);
    for (size_t i = 0; i <= n_ops; i++) h->h_row_off[i] = (uint64_t)i * rl;  // beside the device work
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_failed(fn, "hipStreamSynchronize", e);
    return MLDSA_OK;
}

// rows[n_ops][row_len] = OID || PH(M_i) in h->h_rows, their offsets in h->h_row_off; nothing of a failed call stays in flight
int prehash_rows(const char* fn, mldsa_ph_host* h, int ph, const uint8_t* msgs, const uint64_t* msg_off, size_t n_ops) {
    const int rc = stream_rows(fn, h, ph, msgs, msg_off, n_ops);
    if (rc != MLDSA_OK) h->feed.drain();
    return rc;
}

// the checks of both calls, before a message byte is read
int check_host_call(const char* fn, mldsa_ph_host* h, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* ctx_off,
                    size_t n_ops) {
    if (!h) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL mldsa_ph_host");
    if (!msg_off) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (mldsa_check_offsets(msg_off, n_ops) != MLDSA_OK) return core_failed(fn, MLDSA_ERR_PARAM);
    if (ctx_off && mldsa_check_offsets(ctx_off, n_ops) != MLDSA_OK) return core_failed(fn, MLDSA_ERR_PARAM);
    if (!msgs && msg_off[n_ops] != msg_off[0]) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": msg_off names bytes of a NULL msgs");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_ph_host_create(mldsa_ctx* ctx, size_t staging_bytes, mldsa_ph_host** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(MLDSA_ERR_PARAM, "mldsa_ph_host_create: NULL pointer");
    const int dev = mldsa_ctx_device(ctx);
    if (dev < 0) return fail(MLDSA_ERR_PARAM, "mldsa_ph_host_create: bad context");
    mldsa_ph::DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_ph_host_create: hipSetDevice failed");
    mldsa_ph_host* h = new mldsa_ph_host;
    h->ctx = ctx;
    if (!h->feed.create(dev, staging_bytes)) {
        delete h;
        return fail(MLDSA_ERR_NOMEM, "mldsa_ph_host_create: streams, events or staging memory could not be allocated");
    }
    *out = h;
    return MLDSA_OK;
}

void mldsa_ph_host_destroy(mldsa_ph_host* h) {
    if (!h) return;
    const int dev = h->feed.dev;
    h->feed.destroy();  // waits for both streams
    {
        mldsa_ph::DeviceScope ds(dev);
        release_rows(h);
    }
    delete h;
}

int mldsa_hash_verify_host(mldsa_ph_host* h, int set, int ph, const uint8_t* pk, size_t n_keys, const uint32_t* key_idx,
                           const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off,
                           const uint8_t* sigs, uint8_t* ok, size_t n_ops) {
    const char* fn = "mldsa_hash_verify_host";
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    int rc = check_host_call(fn, h, msgs, msg_off, ctx_off, n_ops);
    if (rc != MLDSA_OK) return rc;
    if (!pk || !sigs || !ok) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    std::lock_guard<std::mutex> lock(h->mu);
    {
        mldsa_ph::DeviceScope ds(h->feed.dev);
        if (!ds.ok) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": hipSetDevice failed");
        rc = prehash_rows(fn, h, ph, msgs, msg_off, n_ops);
        if (rc != MLDSA_OK) return rc;
    }
    rc = mldsa_verify_host(h->ctx, set, MLDSA_MODE_PREHASH, pk, n_keys, key_idx, h->h_rows, h->h_row_off, ctxs, ctx_off, sigs, ok, n_ops);
    if (rc != MLDSA_OK) return core_failed(fn, rc);
    return MLDSA_OK;
}

int mldsa_hash_sign_host(mldsa_ph_host* h, int set, int ph, const uint8_t* sk, size_t n_keys, const uint32_t* key_idx,
                         const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off,
                         const uint8_t* rnd, uint8_t* sigs, int32_t* status, size_t n_ops) {
    const char* fn = "mldsa_hash_sign_host";
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    int rc = check_host_call(fn, h, msgs, msg_off, ctx_off, n_ops);
    if (rc != MLDSA_OK) return rc;
    if (!sk || !rnd || !sigs) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    std::lock_guard<std::mutex> lock(h->mu);
    {
        mldsa_ph::DeviceScope ds(h->feed.dev);
        if (!ds.ok) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": hipSetDevice failed");
        rc = prehash_rows(fn, h, ph, msgs, msg_off, n_ops);
        if (rc != MLDSA_OK) return rc;
    }
    rc = mldsa_sign_host(h->ctx, set, MLDSA_MODE_PREHASH, sk, n_keys, key_idx, h->h_rows, h->h_row_off, ctxs, ctx_off, rnd, sigs, status,
                         n_ops);
    if (rc != MLDSA_OK) return core_failed(fn, rc);
    return MLDSA_OK;
}

}  // extern "C"
