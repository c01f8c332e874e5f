// HashML-DSA from host memory (include/mldsa_ph.h: mldsa_ph_host_*, mldsa_hash_verify_host, mldsa_hash_sign_host).
//
// The raw message bytes [msg_off[0], msg_off[n_ops]) stream through two staging chunks of `staging_bytes` each, cut at
// arbitrary byte positions: chunk i + 1 is uploaded on the copy stream while k_ph_update absorbs chunk i on the compute
// stream.  The ops that have bytes in a chunk are a contiguous range of ops; the update is launched for that range only,
// with the chunk as the window of message offsets (launch_update), so a chunk costs the waves of its own ops and the one
// offset table uploaded at the start of the call serves every chunk.  The host waits only to get a staging chunk back.
// After mldsa_ph_final the rows OID || PH(M) (43 / 75 bytes per op) come to the host and the core's own host-memory call
// does the rest in MLDSA_MODE_PREHASH: verdicts, signatures, statuses and refusals are the core's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/mldsa_ph.h"
#include "ph_internal.h"

struct mldsa_ph_host {
    mldsa_ctx* ctx = nullptr;
    int dev = -1;
    size_t staging = 0;
    std::mutex mu;  // one call at a time
    hipStream_t copy = nullptr, compute = nullptr;
    uint8_t* d_stage[2] = {nullptr, nullptr};
    uint8_t* h_stage[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};  // chunk is in d_stage[b]
    hipEvent_t freed[2] = {nullptr, nullptr};   // the update that read d_stage[b] has finished
    bool in_flight[2] = {false, false};
    // per-call buffers, kept and grown: offsets, states, rows on the device; rows and their offsets on the host
    size_t cap_ops = 0;
    uint64_t* d_off = nullptr;
    uint32_t* d_state = nullptr;
    uint8_t* d_rows = nullptr;
    uint8_t* h_rows = nullptr;
    uint64_t* h_row_off = nullptr;
};

namespace {

using mldsa_ph::core_failed;
using mldsa_ph::fail;
using mldsa_ph::row_len_of;

constexpr size_t DEFAULT_STAGING = (size_t)64 << 20;  // the knee of the sweep recorded in profiles/prehash_stream_bench.jsonl
constexpr int MAX_ROW = 75;

int hip_failed(const char* what, hipError_t e) { return fail(MLDSA_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

void release(mldsa_ph_host* h) {
    for (int b = 0; b < 2; b++) {
        if (h->d_stage[b]) (void)hipFree(h->d_stage[b]);
        if (h->h_stage[b]) (void)hipHostFree(h->h_stage[b]);
        if (h->copied[b]) (void)hipEventDestroy(h->copied[b]);
        if (h->freed[b]) (void)hipEventDestroy(h->freed[b]);
    }
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->h_rows) (void)hipHostFree(h->h_rows);
    if (h->h_row_off) (void)hipHostFree(h->h_row_off);
    if (h->copy) (void)hipStreamDestroy(h->copy);
    if (h->compute) (void)hipStreamDestroy(h->compute);
}

// buffers for n_ops operations of any PH (rows are sized for the longest row)
int reserve(mldsa_ph_host* h, size_t n_ops) {
    size_t need_state = 0;
    for (int ph : mldsa_ph::ALL_PH) need_state = std::max(need_state, mldsa_ph::state_bytes_of(ph, n_ops));
    if (need_state == 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_*_host: n_ops too large");
    if (n_ops <= h->cap_ops) return MLDSA_OK;
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->h_rows) (void)hipHostFree(h->h_rows);
    if (h->h_row_off) (void)hipHostFree(h->h_row_off);
    h->d_off = nullptr, h->d_state = nullptr, h->d_rows = nullptr, h->h_rows = nullptr, h->h_row_off = nullptr;
    h->cap_ops = 0;
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

// page-locked (or otherwise known to the runtime) host memory is copied by DMA where it lies; anything else goes through
// the page-locked bounce chunk
bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

int stream_rows(const char* fn, mldsa_ph_host* h, int ph, const uint8_t* msgs, const uint64_t* msg_off, size_t n_ops) {
    int rc = reserve(h, n_ops);
    if (rc != MLDSA_OK) return rc;
    const size_t rl = (size_t)row_len_of(ph);
    hipError_t e = hipMemcpyAsync(h->d_off, msg_off, 8 * (n_ops + 1), hipMemcpyHostToDevice, h->compute);
    if (e != hipSuccess) return hip_failed(fn, e);
    rc = mldsa_ph::launch_init(ph, h->d_state, n_ops, h->compute);
    if (rc != MLDSA_OK) return rc;

    const uint64_t lo = msg_off[0], hi = msg_off[n_ops];
    const bool pinned = hi > lo && is_pinned(msgs + lo);
    h->in_flight[0] = h->in_flight[1] = false;
    size_t first = 0;  // first op that may still have bytes at or after the chunk's start
    int b = 0;
    for (uint64_t c0 = lo; c0 < hi; b ^= 1) {
        const uint64_t c1 = std::min<uint64_t>(hi, c0 + h->staging);
        const size_t len = (size_t)(c1 - c0);
        if (h->in_flight[b]) {  // the only wait of the loop: the update two chunks back must be done with this buffer
            e = hipEventSynchronize(h->freed[b]);
            if (e != hipSuccess) return hip_failed(fn, e);
        }
        const uint8_t* src = msgs + c0;
        if (!pinned) {
            memcpy(h->h_stage[b], src, len);
            src = h->h_stage[b];
        }
        e = hipMemcpyAsync(h->d_stage[b], src, len, hipMemcpyHostToDevice, h->copy);
        if (e == hipSuccess) e = hipEventRecord(h->copied[b], h->copy);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->compute, h->copied[b], 0);
        if (e != hipSuccess) return hip_failed(fn, e);
        // ops [first, last) have bytes in [c0, c1): the table is non-decreasing (checked by the caller of this function)
        while (first < n_ops && msg_off[first + 1] <= c0) first++;
        const size_t last = (size_t)(std::lower_bound(msg_off + first, msg_off + n_ops, c1) - msg_off);
        rc = mldsa_ph::launch_update(ph, h->d_state, h->d_stage[b], h->d_off, n_ops, first, last - first, c0, c1, c0, h->compute);
        if (rc != MLDSA_OK) return rc;
        e = hipEventRecord(h->freed[b], h->compute);
        if (e != hipSuccess) return hip_failed(fn, e);
        h->in_flight[b] = true;
        c0 = c1;
    }
    rc = mldsa_ph::launch_final(ph, h->d_state, h->d_rows, nullptr, nullptr, n_ops, h->compute);
    if (rc != MLDSA_OK) return rc;
    e = hipMemcpyAsync(h->h_rows, h->d_rows, n_ops * rl, hipMemcpyDeviceToHost, h->compute);
    if (e != hipSuccess) return hip_failed(fn, e);
    for (size_t i = 0; i <= n_ops; i++) h->h_row_off[i] = (uint64_t)i * rl;  // beside the device work
    e = hipStreamSynchronize(h->compute);
    if (e != hipSuccess) return hip_failed(fn, e);
    return MLDSA_OK;
}

// rows[n_ops][row_len] = OID || PH(M_i) in h->h_rows, their offsets in h->h_row_off; nothing of a failed call stays in flight
int prehash_rows(const char* fn, mldsa_ph_host* h, int ph, const uint8_t* msgs, const uint64_t* msg_off, size_t n_ops) {
    const int rc = stream_rows(fn, h, ph, msgs, msg_off, n_ops);
    if (rc != MLDSA_OK) {
        (void)hipStreamSynchronize(h->copy);
        (void)hipStreamSynchronize(h->compute);
    }
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
    h->dev = dev;
    h->staging = staging_bytes ? staging_bytes : DEFAULT_STAGING;
    bool ok = hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&h->compute, hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; b < 2 && ok; b++)
        ok = hipMalloc((void**)&h->d_stage[b], h->staging) == hipSuccess &&
             hipHostMalloc((void**)&h->h_stage[b], h->staging, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&h->copied[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&h->freed[b], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        release(h);
        delete h;
        return fail(MLDSA_ERR_NOMEM, "mldsa_ph_host_create: streams, events or staging memory could not be allocated");
    }
    *out = h;
    return MLDSA_OK;
}

void mldsa_ph_host_destroy(mldsa_ph_host* h) {
    if (!h) return;
    {
        mldsa_ph::DeviceScope ds(h->dev);
        if (h->compute) (void)hipStreamSynchronize(h->compute);
        if (h->copy) (void)hipStreamSynchronize(h->copy);
        release(h);
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
        mldsa_ph::DeviceScope ds(h->dev);
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
        mldsa_ph::DeviceScope ds(h->dev);
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
