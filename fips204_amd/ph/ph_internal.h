// What the objects of libmldsa_ph.so share: the table of the twelve pre-hash functions, the error slot behind mldsa_ph_last_error and the
// launch helpers of the incremental pre-hash that the host-memory entry points drive.  Everything here has C++ linkage
// inside mldsa_ph:: -- the library's C ABI is include/mldsa_ph.h and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/mldsa_ph.h"
#include "../layer/layer_host.h"

namespace mldsa_ph {

constexpr int OID_LEN = 11;
constexpr uint8_t OID_PREFIX[10] = {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x02};

// The twelve functions are three compression functions.  The one-shot kernels (prehash.hip) are compiled once per (family,
// block): SHA-2 with 32-bit words (block 64), SHA-2 with 64-bit words (block 128) and Keccak-f[1600] at the rates 168 / 144 /
// 136 / 104 / 72; the incremental kernels (stream.hip) once per family, with Keccak's rate as data.  What separates the
// functions of one instance -- initial value, digest length, the last OID byte, the first pad byte -- is data too and travels
// as a kernel argument (PhVar).
constexpr int FAM_SHA2_32 = 0, FAM_SHA2_64 = 1, FAM_KECCAK = 2;

template <int FAM, int BLOCK_> struct FamTraits;
template <> struct FamTraits<FAM_SHA2_32, 64> { static constexpr int BLOCK = 64, TAIL = 9, MAX_DIGEST = 32; };     // 0x80, 64-bit length
template <> struct FamTraits<FAM_SHA2_64, 128> { static constexpr int BLOCK = 128, TAIL = 17, MAX_DIGEST = 64; };  // 0x80, 128-bit length
// Keccak: the pad (first byte ... 0x80) always fits in the block that holds the message's end
template <int RATE> struct FamTraits<FAM_KECCAK, RATE> {
    static_assert(RATE % 8 == 0 && RATE >= 72 && RATE <= 168, "rate");
    static constexpr int BLOCK = RATE, TAIL = 1, MAX_DIGEST = RATE < 64 ? RATE : 64;
};

struct PhVar {
    uint8_t oid_last;  // last byte of the OID 2.16.840.1.101.3.4.2.x
    uint8_t digest;    // bytes of PH(M) in a row
    uint8_t padb;      // the byte behind the message: 0x80 (SHA-2), 0x06 (SHA-3), 0x1F (SHAKE)
    uint8_t iv;        // SHA-2: which initial value (sha2_dev.h: IV256_* / IV512_*)
    uint8_t block;     // block / rate in bytes: read by the kernels that are not compiled per block (stream.hip)
};

struct PhInfo {
    int fam;
    PhVar var;
};

// the table of include/mldsa_ph.h; false for an unknown ph
inline bool ph_info(int ph, PhInfo* o) {
    switch (ph) {
        case MLDSA_PH_SHA256: *o = {FAM_SHA2_32, {0x01, 32, 0x80, 0, 64}}; return true;
        case MLDSA_PH_SHA224: *o = {FAM_SHA2_32, {0x04, 28, 0x80, 1, 64}}; return true;
        case MLDSA_PH_SHA512: *o = {FAM_SHA2_64, {0x03, 64, 0x80, 0, 128}}; return true;
        case MLDSA_PH_SHA384: *o = {FAM_SHA2_64, {0x02, 48, 0x80, 1, 128}}; return true;
        case MLDSA_PH_SHA512_224: *o = {FAM_SHA2_64, {0x05, 28, 0x80, 2, 128}}; return true;
        case MLDSA_PH_SHA512_256: *o = {FAM_SHA2_64, {0x06, 32, 0x80, 3, 128}}; return true;
        case MLDSA_PH_SHA3_224: *o = {FAM_KECCAK, {0x07, 28, 0x06, 0, 144}}; return true;
        case MLDSA_PH_SHA3_256: *o = {FAM_KECCAK, {0x08, 32, 0x06, 0, 136}}; return true;
        case MLDSA_PH_SHA3_384: *o = {FAM_KECCAK, {0x09, 48, 0x06, 0, 104}}; return true;
        case MLDSA_PH_SHA3_512: *o = {FAM_KECCAK, {0x0a, 64, 0x06, 0, 72}}; return true;
        case MLDSA_PH_SHAKE128: *o = {FAM_KECCAK, {0x0b, 32, 0x1F, 0, 168}}; return true;
        case MLDSA_PH_SHAKE256: *o = {FAM_KECCAK, {0x0c, 64, 0x1F, 0, 136}}; return true;
        default: return false;
    }
}

// every function the library knows, for code that sizes a buffer for any of them
constexpr int ALL_PH[12] = {MLDSA_PH_SHA256, MLDSA_PH_SHA512, MLDSA_PH_SHAKE128, MLDSA_PH_SHA384, MLDSA_PH_SHA224, MLDSA_PH_SHA512_224,
                            MLDSA_PH_SHA512_256, MLDSA_PH_SHA3_224, MLDSA_PH_SHA3_256, MLDSA_PH_SHA3_384, MLDSA_PH_SHA3_512,
                            MLDSA_PH_SHAKE256};

// Calls f(std::integral_constant<int, FAM>, std::integral_constant<int, BLOCK>) for the kernel instance of `info`.
template <typename F>
inline void dispatch_instance(const PhInfo& info, F&& f) {
    using std::integral_constant;
    if (info.fam == FAM_SHA2_32) return f(integral_constant<int, FAM_SHA2_32>{}, integral_constant<int, 64>{});
    if (info.fam == FAM_SHA2_64) return f(integral_constant<int, FAM_SHA2_64>{}, integral_constant<int, 128>{});
    switch (info.var.block) {
        case 168: return f(integral_constant<int, FAM_KECCAK>{}, integral_constant<int, 168>{});
        case 144: return f(integral_constant<int, FAM_KECCAK>{}, integral_constant<int, 144>{});
        case 136: return f(integral_constant<int, FAM_KECCAK>{}, integral_constant<int, 136>{});
        case 104: return f(integral_constant<int, FAM_KECCAK>{}, integral_constant<int, 104>{});
        default: return f(integral_constant<int, FAM_KECCAK>{}, integral_constant<int, 72>{});
    }
}

// ---- host side (prehash.hip) ----
int fail(int rc, const std::string& msg);          // sets the thread's message, returns rc
int core_failed(const char* fn, int rc);           // the same with the core's message
int row_len_of(int ph);                            // negative for an unknown ph

// the context's device for the call, the caller's current device afterwards: the layers' one (layer/layer_host.h).  Nothing else of that
// scaffold is used here: the three objects of this library share one error slot, which prehash.hip defines
using mldsa_layer::DeviceScope;

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
