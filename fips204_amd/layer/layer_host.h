// The host scaffold of a library layered on the core's C ABI (keys/, mu/, seed/, keycheck/, mus/; ph/ takes DeviceScope alone): the error slot
// behind the library's mldsa_*_last_error, the device scope of a call, the scratch-layout helpers, and the checks that open and the
// clearing that closes an entry point.
// Everything here has internal linkage (the unnamed namespace).  The layered libraries are loaded into one process: a thread_local or
// inline variable with external linkage would be exported weakly by each of them and bound to whichever was loaded first, and every
// mldsa_*_last_error would read one slot.  So each library that includes this header gets an error slot of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_hip.h"

namespace mldsa_layer {
namespace {

// ---------------------------------------------------------------------------------------------------------------- errors
thread_local std::string g_err;  // what the library's mldsa_*_last_error returns

int fail(int rc, const std::string& msg) {
    g_err = msg;
    return rc;
}

int core_failed(const char* fn, const char* core_fn, int rc) {
    const char* m = mldsa_last_error();
    return fail(rc, std::string(fn) + ": " + core_fn + ": " + (m ? m : "(no message)"));
}

int hip_failed(const char* fn, const char* what, hipError_t e) {
    return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
}

// inside a function that has `const char* fn`: a core call / the launches since the last check, or return the error
#define LAYER_CORE(call, name)                                   \
    do {                                                         \
        const int rc_ = (call);                                  \
        if (rc_ != MLDSA_OK) return core_failed(fn, name, rc_);  \
    } while (0)

#define LAYER_LAUNCHED(what)                                    \
    do {                                                        \
        const hipError_t e_ = hipGetLastError();                \
        if (e_ != hipSuccess) return hip_failed(fn, what, e_);  \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------- device
// the context's device for the call, the caller's current device afterwards
struct DeviceScope {
    int prev = -1;
    bool ok = false;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// inside an entry point that has `const char* fn`, behind its argument checks: `ds`, the entry point's own DeviceScope on the context's
// device, or return the error
#define LAYER_ON_DEVICE(ctx)                                                                      \
    const int dev_ = mldsa_ctx_device(ctx);                                                       \
    if (dev_ < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": bad context");                \
    DeviceScope ds(dev_);                                                                         \
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": hipSetDevice failed")

// --------------------------------------------------------------------------------------------------------------- scratch
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// An output buffer does not overlap the blob it is filled from: decided from the two pointer ranges as integers (nothing is added to a
// pointer that might not hold it).  An empty range overlaps nothing.
bool ranges_apart(const void* blob, uint64_t blob_len, const void* out, uint64_t out_len) {
    const uintptr_t b = (uintptr_t)blob, o = (uintptr_t)out;
    return blob_len == 0 || out_len == 0 || (b >= o && b - o >= out_len) || (o >= b && o - b >= blob_len);
}

// Bump allocator of a scratch layout: take() returns the part's offset; every part is rounded up to `round` bytes.
struct Taker {
    size_t at = 0, round = 1;
    size_t take(size_t bytes) {
        const size_t here = at;
        at += (bytes + round - 1) / round * round;
        return here;
    }
};

// the largest pass P <= n whose scratch (bytes_of(P), growing with P) fits; 0 when not even that of min(n, 64) does
template <class Bytes>
size_t largest_pass(size_t n, size_t scratch_bytes, Bytes bytes_of) {
    const size_t min_n = n < 64 ? n : 64;
    if (bytes_of(min_n) > scratch_bytes) return 0;
    size_t lo = min_n, hi = n;  // bytes_of(lo) fits
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (bytes_of(mid) <= scratch_bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The end of a call whose scratch held secrets: the scratch is cleared behind the call's last kernel whatever rc says, and with `sync`
// the stream is waited for.  Returns rc if that is an error, else the clearing's, reported under `what`.
int cleared(const char* fn, int rc, void* scratch, size_t scratch_bytes, hipStream_t s, bool sync, const char* what) {
    int zrc = mldsa_memset(scratch, 0, scratch_bytes, (void*)s);
    if (zrc == MLDSA_OK && sync) zrc = mldsa_stream_sync((void*)s);
    if (rc != MLDSA_OK) return rc;
    return zrc == MLDSA_OK ? MLDSA_OK : core_failed(fn, what, zrc);
}

// ---------------------------------------------------------------------------------------------------------------- checks
// the argument checks that open an entry point over n items, of which the library takes at most `cap` (cap_what: the cap's name and the
// items', for the message); *p is filled
int check_common(const char* fn, const mldsa_ctx* ctx, int set, size_t n, size_t cap, const char* cap_what, mldsa_params* p) {
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (mldsa_get_params(set, p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (n > cap) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than " + cap_what);
    return MLDSA_OK;
}

}  // namespace
}  // namespace mldsa_layer
