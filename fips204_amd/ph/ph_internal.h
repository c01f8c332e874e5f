// What the objects of libmldsa_ph.so share: the per-PH constants, the error slot behind mldsa_ph_last_error and the
// launch helpers of the incremental pre-hash that the host-memory entry points drive.  Everything here has C++ linkage
// inside mldsa_ph:: -- the library's C ABI is include/mldsa_ph.h and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_ph.h"

namespace mldsa_ph {

constexpr int OID_LEN = 11;
constexpr uint8_t OID_PREFIX[10] = {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x02};

template <int PH> struct PhTraits;
template <> struct PhTraits<MLDSA_PH_SHA256> { static constexpr int BLOCK = 64, TAIL = 9, DIGEST = 32; static constexpr uint8_t OID_LAST = 0x01; };
template <> struct PhTraits<MLDSA_PH_SHA512> { static constexpr int BLOCK = 128, TAIL = 17, DIGEST = 64; static constexpr uint8_t OID_LAST = 0x03; };
// SHAKE128: rate 168; the pad (0x1F ... 0x80) always fits in the block that holds the message's end
template <> struct PhTraits<MLDSA_PH_SHAKE128> { static constexpr int BLOCK = 168, TAIL = 1, DIGEST = 32; static constexpr uint8_t OID_LAST = 0x0b; };

// ---- host side (prehash.hip) ----
int fail(int rc, const std::string& msg);          // sets the thread's message, returns rc
int core_failed(const char* fn, int rc);           // the same with the core's message
int row_len_of(int ph);                            // negative for an unknown ph

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

// ---- incremental pre-hash (stream.hip) ----
size_t state_bytes_of(int ph, size_t n_ops);       // 0 for an unknown ph or a size that does not fit
int launch_init(int ph, uint32_t* state, size_t n_ops, hipStream_t s);
// Ops [first, first + count) of a batch of n_ops absorb the part of their piece pieces[off[i], off[i + 1]) that lies in
// the window [win_lo, win_hi) of offsets; byte x of the window is read at pieces[x - sub].  The public update is the
// whole batch with the window [0, 2^64) and sub = 0; the host-memory calls pass one staging chunk as the window.
int launch_update(int ph, uint32_t* state, const uint8_t* pieces, const uint64_t* off, size_t n_ops, size_t first, size_t count,
                  uint64_t win_lo, uint64_t win_hi, uint64_t sub, hipStream_t s);
int launch_final(int ph, const uint32_t* state, uint8_t* out, uint64_t* out_off, uint8_t* bad, size_t n_ops, hipStream_t s);

}  // namespace mldsa_ph
