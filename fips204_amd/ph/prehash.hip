// HashML-DSA pre-hash on the GPU (include/mldsa_ph.h): PH(M) of each raw message for the twelve functions of the NIST hash
// OID arc (the reference's three, src/hashing.rs:316-354, and the nine others FIPS 204 §5.4 allows), then the core's
// MLDSA_MODE_PREHASH call on the rows OID || PH(M).
//
// k_prehash<FAM, BLOCK, PH>: one message per lane, 64 per wave (the layout of the core's k_mu).  Each lane absorbs its own blocks
// and pads its own message; the wave loops to its longest message.  Whole dwords of the message come from one
// byte-granular dword load each; only the dwords around the message's end are assembled from bytes.  The same launch
// writes each op's row and the offset table the core call reads (off[i] = i row_len).  One instance per compression function
// and block size (ph_internal.h); initial value, pad byte, digest length and OID byte are arguments (PhVar), except in the
// instances of the reference's three functions, which keep them as constants.
// k_prehash_wave<RATE>: the small-call form of the Keccak family, one message per WAVE on the bit-interleaved cooperative
// sponge of csrc/keccak_coop2.h, the way mu_coop2 (csrc/verify_dev.h) computes mu for small calls.  Calls of at most
// MLDSA_PH_COOP_MAX_OPS operations take it; checks, refusals, rows and offset table are k_prehash's, byte for byte.
// k_ph_refuse: after the core call, the per-op refusal of ops whose message pair was malformed (the core saw a
// well-formed table of rows, so it cannot know).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_ph.h"
#include "../csrc/keccak.h"
#include "../csrc/keccak_coop2.h"
#include "ph_internal.h"
#include "sha2_dev.h"

namespace {

using mldsa::Coop2Lane;
using mldsa::KeccakState;
using mldsa::load_le32;
using mldsa_ph::bswap32;
using mldsa_ph::static_for;

using mldsa_ph::core_failed;
using mldsa_ph::DeviceScope;
using mldsa_ph::fail;
using mldsa_ph::FAM_KECCAK;
using mldsa_ph::FAM_SHA2_32;
using mldsa_ph::FAM_SHA2_64;
using mldsa_ph::FamTraits;
using mldsa_ph::OID_LEN;
using mldsa_ph::OID_PREFIX;
using mldsa_ph::PhInfo;
using mldsa_ph::PhVar;
using mldsa_ph::row_len_of;

// little-endian dword at byte `pos` of the padded message: message bytes, then padb, then zeros
__device__ __forceinline__ uint32_t padded_le32(const uint8_t* mp, size_t mlen, size_t pos, uint32_t padb) {
    if (pos + 4 <= mlen) return load_le32(mp + pos);
    if (pos > mlen) return 0;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t p = pos + k;
        const uint32_t byte = p < mlen ? mp[p] : p == mlen ? padb : 0u;
        v |= byte << (8 * k);
    }
    return v;
}

// The checks of k_mu for op `op` of a call of n_ops: the call vouches for [off[0], off[n_ops]); a pair outside it in order is
// refused unread.  live: the op is hashed (mp, mlen valid); msg_bad: its message pair was malformed.
struct OpMsg {
    const uint8_t* mp;
    size_t mlen;
    bool msg_bad, live;
};

__device__ __forceinline__ OpMsg check_op(const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off,
                                          size_t op, size_t n_ops) {
    OpMsg o = {nullptr, 0, false, false};
    const uint64_t m0 = msg_off[op], m1 = msg_off[op + 1];
    o.msg_bad = !(msg_off[0] <= m0 && m0 <= m1 && m1 <= msg_off[n_ops]);
    o.msg_bad |= m1 != m0 && msgs == nullptr;
    bool ctx_bad = false;
    if (ctx_off) {
        const uint64_t c0 = ctx_off[op], c1 = ctx_off[op + 1];
        ctx_bad = !(ctx_off[0] <= c0 && c0 <= c1 && c1 <= ctx_off[n_ops]);
        ctx_bad |= c1 != c0 && ctxs == nullptr;
        ctx_bad |= !ctx_bad && c1 - c0 > 255;
    }
    o.live = !o.msg_bad && !ctx_bad;
    if (o.live) {
        o.mp = msgs + m0;
        o.mlen = (size_t)(m1 - m0);
    }
    return o;
}

// What PhVar holds for the reference's three functions, as constants: their instances (PH >= 0) are compiled with them, so that
// their code is what it was before the other nine came (with the four values as data the three measured 6-19 % slower at
// 65 536 x 1 KiB, profiles/prehash_fips_list_bench.jsonl).  PH = -1: the values are the kernel argument.
template <int PH> struct FixedVar { static constexpr int DIGEST = 0, IV = 0; static constexpr uint32_t OID_LAST = 0; };
template <> struct FixedVar<MLDSA_PH_SHA256> { static constexpr int DIGEST = 32, IV = 0; static constexpr uint32_t OID_LAST = 0x01; };
template <> struct FixedVar<MLDSA_PH_SHA512> { static constexpr int DIGEST = 64, IV = 0; static constexpr uint32_t OID_LAST = 0x03; };
template <> struct FixedVar<MLDSA_PH_SHAKE128> { static constexpr int DIGEST = 32, IV = 0; static constexpr uint32_t OID_LAST = 0x0b; };

template <int FAM, int BLOCK, int PH>
__global__ __launch_bounds__(64) void k_prehash(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ msg_off,
                                                const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off,
                                                uint8_t* __restrict__ out, uint64_t* __restrict__ out_off,
                                                uint8_t* __restrict__ bad, size_t n_ops, PhVar var) {
    using T = FamTraits<FAM, BLOCK>;
    using FV = FixedVar<PH>;
    constexpr int MAX_DIGEST = PH >= 0 ? FV::DIGEST : T::MAX_DIGEST;
    const int digest = PH >= 0 ? FV::DIGEST : (int)var.digest;
    const int iv = PH >= 0 ? FV::IV : (int)var.iv;
    const uint32_t oid_last = PH >= 0 ? FV::OID_LAST : (uint32_t)var.oid_last;
    const size_t row_len = (size_t)OID_LEN + digest;
    const int lane = threadIdx.x;
    const size_t op = (size_t)blockIdx.x * 64 + lane;
    const bool valid = op < n_ops;

    OpMsg o = {nullptr, 0, false, false};
    if (valid) o = check_op(msgs, msg_off, ctxs, ctx_off, op, n_ops);
    const uint8_t* mp = o.mp;
    const size_t mlen = o.mlen;
    const bool msg_bad = o.msg_bad, live = o.live;
    const size_t my_blocks = live ? (mlen + T::TAIL + T::BLOCK - 1) / T::BLOCK : 0;
    size_t max_blocks = my_blocks;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const size_t o2 = (size_t)__shfl_xor((unsigned long long)max_blocks, m);
        max_blocks = o2 > max_blocks ? o2 : max_blocks;
    }

    uint8_t dig[MAX_DIGEST];
    if constexpr (FAM == FAM_SHA2_32) {
        mldsa_ph::Sha256State st;
        mldsa_ph::sha256_init(st, iv);
        for (size_t b = 0; b < max_blocks; b++) {
            if (b < my_blocks) {
                const size_t base = b * 64;
                uint32_t w[16];
                if (base + 64 <= mlen) {
#pragma unroll
                    for (int i = 0; i < 16; i++) w[i] = bswap32(load_le32(mp + base + 4 * i));
                } else {
#pragma unroll
                    for (int i = 0; i < 16; i++) w[i] = bswap32(padded_le32(mp, mlen, base + 4 * i, 0x80));
                    if (b == my_blocks - 1) {  // 64-bit big-endian bit length
                        w[14] = (uint32_t)(mlen >> 29);
                        w[15] = (uint32_t)(mlen << 3);
                    }
                }
                mldsa_ph::sha256_block(st, w);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) dig[4 * i + k] = (uint8_t)(st.h[i] >> (24 - 8 * k));
    } else if constexpr (FAM == FAM_SHA2_64) {
        mldsa_ph::Sha512State st;
        mldsa_ph::sha512_init(st, iv);
        for (size_t b = 0; b < max_blocks; b++) {
            if (b < my_blocks) {
                const size_t base = b * 128;
                mldsa_ph::U64 w[16];
                if (base + 128 <= mlen) {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        w[i].hi = bswap32(load_le32(mp + base + 8 * i));
                        w[i].lo = bswap32(load_le32(mp + base + 8 * i + 4));
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        w[i].hi = bswap32(padded_le32(mp, mlen, base + 8 * i, 0x80));
                        w[i].lo = bswap32(padded_le32(mp, mlen, base + 8 * i + 4, 0x80));
                    }
                    if (b == my_blocks - 1) {  // 128-bit big-endian bit length, high half 0
                        w[14] = {0u, 0u};
                        w[15] = {(uint32_t)(mlen << 3), (uint32_t)(mlen >> 29)};
                    }
                }
                mldsa_ph::sha512_block(st, w);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                dig[8 * i + k] = (uint8_t)(st.h[i].hi >> (24 - 8 * k));
                dig[8 * i + 4 + k] = (uint8_t)(st.h[i].lo >> (24 - 8 * k));
            }
    } else {
        constexpr int RW = BLOCK / 8;  // 64-bit words of the rate
        const uint32_t padb = PH == MLDSA_PH_SHAKE128 ? 0x1Fu : (uint32_t)var.padb;
        KeccakState st;
        mldsa::keccak_zero(st);
        for (size_t b = 0; b < max_blocks; b++) {
            if (b < my_blocks) {
                const size_t base = b * BLOCK;
                if (base + BLOCK <= mlen) {
                    static_for<0, RW>([&](auto wc) {
                        constexpr int W = decltype(wc)::value;
                        st.lo[W] ^= load_le32(mp + base + 8 * W);
                        st.hi[W] ^= load_le32(mp + base + 8 * W + 4);
                    });
                } else {
                    static_for<0, RW>([&](auto wc) {
                        constexpr int W = decltype(wc)::value;
                        st.lo[W] ^= padded_le32(mp, mlen, base + 8 * W, padb);
                        st.hi[W] ^= padded_le32(mp, mlen, base + 8 * W + 4, padb);
                    });
                }
                if (b == my_blocks - 1) st.hi[RW - 1] ^= 0x80000000u;  // last byte of this rate's block
                mldsa::keccak_f1600(st);
            }
        }
#pragma unroll
        for (int i = 0; i < MAX_DIGEST / 8; i++)  // at most 64 bytes, inside the first block of every rate
#pragma unroll
            for (int k = 0; k < 4; k++) {
                dig[8 * i + k] = (uint8_t)(st.lo[i] >> (8 * k));
                dig[8 * i + 4 + k] = (uint8_t)(st.hi[i] >> (8 * k));
            }
    }

    if (valid) {
        uint8_t* row = out + op * row_len;
#pragma unroll
        for (int i = 0; i < 10; i++) row[i] = live ? OID_PREFIX[i] : 0;
        row[10] = live ? oid_last : 0;
#pragma unroll
        for (int i = 0; i < MAX_DIGEST; i++)  // a truncated digest ends the row: nothing behind it is written
            if (i < digest) row[OID_LEN + i] = live ? dig[i] : 0;
        if (bad) bad[op] = msg_bad ? 1 : 0;
        if (out_off) {
            out_off[op] = (uint64_t)op * row_len;
            if (op == n_ops - 1) out_off[n_ops] = (uint64_t)n_ops * row_len;
        }
    }
}

// One message per wave: block blockIdx.x hashes op blockIdx.x.  The lanes that hold a rate word load their own (lo, hi) of
// each block -- the whole block in one wave-wide load -- and the digest leaves through the lanes of words 0 .. 7.
template <int RATE>
__global__ __launch_bounds__(64) void k_prehash_wave(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ msg_off,
                                                     const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off,
                                                     uint8_t* __restrict__ out, uint64_t* __restrict__ out_off,
                                                     uint8_t* __restrict__ bad, size_t n_ops, PhVar var) {
    const int lane = threadIdx.x;
    const size_t op = blockIdx.x;  // the launch has exactly n_ops blocks
    const int digest = var.digest;
    const size_t row_len = (size_t)OID_LEN + digest;
    const uint32_t padb = var.padb;
    const Coop2Lane c = mldsa::coop2_lane(lane);
    const OpMsg o = check_op(msgs, msg_off, ctxs, ctx_off, op, n_ops);  // wave-uniform
    const size_t blocks = o.live ? o.mlen / RATE + 1 : 0;                // the pad always fits in the last block

    uint32_t v = 0;
    const bool absorbs = c.active && c.word < RATE / 8;
    for (size_t b = 0; b < blocks; b++) {
        if (absorbs) {
            const size_t pos = b * RATE + 8 * (size_t)c.word;
            const uint32_t lo = padded_le32(o.mp, o.mlen, pos, padb);
            uint32_t hi = padded_le32(o.mp, o.mlen, pos + 4, padb);
            if (b == blocks - 1 && c.word == RATE / 8 - 1) hi ^= 0x80000000u;
            v ^= mldsa::coop2_from_lohi(lo, hi, c);
        }
        mldsa::keccak_f1600_coop2(v, c);
    }
    uint32_t lo, hi;
    mldsa::coop2_to_lohi(v, lane, lo, hi);  // a refused op never entered the loop: v = 0, an all-zero digest

    uint8_t* row = out + op * row_len;
    if (lane < 32 && c.active && c.word < 8) {  // lanes 0 .. 7: digest bytes 8 word .. 8 word + 7 (digest lengths are multiples of 4)
        uint8_t* d = row + OID_LEN + 8 * c.word;
        if (8 * c.word < digest) {
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = (uint8_t)(lo >> (8 * k));
        }
        if (8 * c.word + 4 < digest) {
#pragma unroll
            for (int k = 0; k < 4; k++) d[4 + k] = (uint8_t)(hi >> (8 * k));
        }
    } else if (lane >= 32 && lane < 32 + OID_LEN) {
        const int i = lane - 32;
        uint32_t b = var.oid_last;
#pragma unroll
        for (int k = 0; k < 10; k++) b = i == k ? OID_PREFIX[k] : b;
        row[i] = o.live ? (uint8_t)b : 0;
    } else if (lane == 63) {
        if (bad) bad[op] = o.msg_bad ? 1 : 0;
        if (out_off) {
            out_off[op] = (uint64_t)op * row_len;
            if (op == n_ops - 1) out_off[n_ops] = (uint64_t)n_ops * row_len;
        }
    }
}

// ops whose message pair was malformed: ok = 0, status MLDSA_ERR_PARAM, an all-zero signature
__global__ __launch_bounds__(64) void k_ph_refuse(const uint8_t* __restrict__ bad, uint8_t* __restrict__ ok,
                                                  uint8_t* __restrict__ sigs, size_t sig_len, int32_t* __restrict__ status,
                                                  size_t n_ops) {
    const int lane = threadIdx.x;
    const size_t op0 = (size_t)blockIdx.x * 64;
    const size_t op = op0 + lane;
    const bool b = op < n_ops && bad[op] != 0;
    if (b) {
        if (ok) ok[op] = 0;
        if (status) status[op] = MLDSA_ERR_PARAM;
    }
    if (!sigs) return;
    uint64_t mask = __ballot(b);
    while (mask) {  // the wave clears the refused signatures one by one, consecutive lanes on consecutive bytes
        const int l = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        uint8_t* row = sigs + (op0 + l) * sig_len;
        for (size_t i = lane; i < sig_len; i += 64) row[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
thread_local std::string g_err;

// scratch = [offset table: 8 (n + 1)] [rows: n row_len] [bad: n]; 0 when it does not fit a size_t
size_t scratch_of(int ph, size_t n) {
    const int rl = row_len_of(ph);
    if (rl < 0) return 0;
    const size_t lim = ~(size_t)0 / 128;
    if (n >= lim) return 0;
    return 8 * (n + 1) + n * (size_t)rl + n;
}

int launch_prehash(int ph, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, uint8_t* out,
                   uint64_t* out_off, uint8_t* bad, size_t n_ops, hipStream_t s) {
    PhInfo info;
    if (!mldsa_ph::ph_info(ph, &info)) return fail(MLDSA_ERR_PARAM, "k_prehash launch: unknown ph");
    const bool wave = info.fam == FAM_KECCAK && n_ops <= (size_t)MLDSA_PH_COOP_MAX_OPS;
    const dim3 grid((unsigned)(wave ? n_ops : (n_ops + 63) / 64)), block(64);
    mldsa_ph::dispatch_instance(info, [&](auto fc, auto bc) {
        constexpr int FAM = decltype(fc)::value, BLOCK = decltype(bc)::value;
        if constexpr (FAM == FAM_KECCAK) {
            if (wave) {
                hipLaunchKernelGGL((k_prehash_wave<BLOCK>), grid, block, 0, s, msgs, msg_off, ctxs, ctx_off, out, out_off, bad, n_ops, info.var);
                return;
            }
        }
        // the reference's three have instances of their own (FixedVar); SHAKE128 is the only function at rate 168
        if (ph == MLDSA_PH_SHA256 || ph == MLDSA_PH_SHA512 || ph == MLDSA_PH_SHAKE128) {
            constexpr int PH = FAM == FAM_SHA2_32 ? MLDSA_PH_SHA256 : FAM == FAM_SHA2_64 ? MLDSA_PH_SHA512 : MLDSA_PH_SHAKE128;
            if constexpr (FAM != FAM_KECCAK || BLOCK == 168)
                hipLaunchKernelGGL((k_prehash<FAM, BLOCK, PH>), grid, block, 0, s, msgs, msg_off, ctxs, ctx_off, out, out_off, bad, n_ops, info.var);
        } else {
            if constexpr (FAM != FAM_KECCAK || BLOCK != 168)
                hipLaunchKernelGGL((k_prehash<FAM, BLOCK, -1>), grid, block, 0, s, msgs, msg_off, ctxs, ctx_off, out, out_off, bad, n_ops, info.var);
        }
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MLDSA_ERR_DEVICE, std::string("k_prehash launch: ") + hipGetErrorString(e));
    return MLDSA_OK;
}

int launch_refuse(const uint8_t* bad, uint8_t* ok, uint8_t* sigs, size_t sig_len, int32_t* status, size_t n_ops, hipStream_t s) {
    hipLaunchKernelGGL(k_ph_refuse, dim3((unsigned)((n_ops + 63) / 64)), dim3(64), 0, s, bad, ok, sigs, sig_len, status, n_ops);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MLDSA_ERR_DEVICE, std::string("k_ph_refuse launch: ") + hipGetErrorString(e));
    return MLDSA_OK;
}

// the checks shared by the op-level calls, all before anything is launched
struct Scratch {
    uint64_t* off;
    uint8_t* rows;
    uint8_t* bad;
};

int check_call(const char* fn, mldsa_ctx* ctx, int set, int ph, size_t n_keys, const uint32_t* key_idx, size_t n_ops, void* scratch,
               size_t scratch_bytes, mldsa_params* p, Scratch* sc) {
    const int rl = row_len_of(ph);
    if (rl < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown ph");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (mldsa_get_params(set, p) != MLDSA_OK) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown parameter set");
    if (key_idx ? n_keys == 0 : n_keys < n_ops) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys does not cover the batch");
    const size_t need = scratch_of(ph, n_ops);
    if (!scratch || need == 0 || scratch_bytes < need || ((uintptr_t)scratch & 7) != 0)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, misaligned or smaller than mldsa_ph_scratch_bytes");
    uint8_t* base = static_cast<uint8_t*>(scratch);
    sc->off = reinterpret_cast<uint64_t*>(base);
    sc->rows = base + 8 * (n_ops + 1);
    sc->bad = sc->rows + n_ops * (size_t)rl;
    return MLDSA_OK;
}

}  // namespace

namespace mldsa_ph {

int fail(int rc, const std::string& msg) {
    g_err = msg;
    return rc;
}

int core_failed(const char* fn, int rc) {
    const char* m = mldsa_last_error();
    return fail(rc, std::string(fn) + ": " + (m ? m : "(no message)"));
}

int row_len_of(int ph) {
    PhInfo info;
    return ph_info(ph, &info) ? OID_LEN + info.var.digest : -1;
}

}  // namespace mldsa_ph

extern "C" {

int mldsa_ph_abi_version(void) { return MLDSA_PH_ABI_VERSION; }

const char* mldsa_ph_last_error(void) { return g_err.c_str(); }

int mldsa_ph_row_len(int ph) { return row_len_of(ph); }

size_t mldsa_ph_scratch_bytes(int ph, size_t n_ops) { return scratch_of(ph, n_ops); }

int mldsa_prehash(mldsa_ctx* ctx, int ph, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* out, uint8_t* bad, size_t n_ops,
                  void* stream) {
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, "mldsa_prehash: unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx || !msg_off || !out) return fail(MLDSA_ERR_PARAM, "mldsa_prehash: NULL pointer");
    const int dev = mldsa_ctx_device(ctx);
    if (dev < 0) return fail(MLDSA_ERR_PARAM, "mldsa_prehash: bad context");
    DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_prehash: hipSetDevice failed");
    return launch_prehash(ph, msgs, msg_off, nullptr, nullptr, out, nullptr, bad, n_ops, (hipStream_t)stream);
}

int mldsa_hash_verify(mldsa_ctx* ctx, int set, int ph, const uint8_t* rho, const uint8_t* tr, const int32_t* t1_d2_hat_mont,
                      size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs,
                      const uint64_t* ctx_off, const uint8_t* sigs, uint8_t* ok, size_t n_ops, void* scratch, size_t scratch_bytes,
                      void* stream) {
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify: unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    if (!rho || !tr || !t1_d2_hat_mont || !msg_off || !sigs || !ok) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify: NULL pointer");
    mldsa_params p;
    Scratch sc;
    int rc = check_call("mldsa_hash_verify", ctx, set, ph, n_keys, key_idx, n_ops, scratch, scratch_bytes, &p, &sc);
    if (rc != MLDSA_OK) return rc;
    const int dev = mldsa_ctx_device(ctx);
    if (dev < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify: bad context");
    DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_hash_verify: hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    rc = launch_prehash(ph, msgs, msg_off, ctxs, ctx_off, sc.rows, sc.off, sc.bad, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    rc = mldsa_verify(ctx, set, MLDSA_MODE_PREHASH, rho, tr, t1_d2_hat_mont, n_keys, key_idx, sc.rows, sc.off, ctxs, ctx_off, sigs, ok,
                      n_ops, stream);
    if (rc != MLDSA_OK) return core_failed("mldsa_hash_verify", rc);
    return launch_refuse(sc.bad, ok, nullptr, 0, nullptr, n_ops, s);
}

int mldsa_hash_verify_pk(mldsa_ctx* ctx, int set, int ph, const uint8_t* pk, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                         const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, const uint8_t* sigs, uint8_t* ok,
                         size_t n_ops, void* scratch, size_t scratch_bytes, void* stream) {
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify_pk: unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    if (!pk || !msg_off || !sigs || !ok) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify_pk: NULL pointer");
    mldsa_params p;
    Scratch sc;
    int rc = check_call("mldsa_hash_verify_pk", ctx, set, ph, n_keys, key_idx, n_ops, scratch, scratch_bytes, &p, &sc);
    if (rc != MLDSA_OK) return rc;
    const int dev = mldsa_ctx_device(ctx);
    if (dev < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_verify_pk: bad context");
    DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_hash_verify_pk: hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    rc = launch_prehash(ph, msgs, msg_off, ctxs, ctx_off, sc.rows, sc.off, sc.bad, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    rc = mldsa_verify_pk(ctx, set, MLDSA_MODE_PREHASH, pk, n_keys, key_idx, sc.rows, sc.off, ctxs, ctx_off, sigs, ok, n_ops, stream);
    if (rc != MLDSA_OK) return core_failed("mldsa_hash_verify_pk", rc);
    return launch_refuse(sc.bad, ok, nullptr, 0, nullptr, n_ops, s);
}

int mldsa_hash_sign(mldsa_ctx* ctx, int set, int ph, const uint8_t* rho, const uint8_t* cap_k, const uint8_t* tr,
                    const int32_t* s_1_hat_mont, const int32_t* s_2_hat_mont, const int32_t* t_0_hat_mont, size_t n_keys,
                    const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off,
                    const uint8_t* rnd, uint8_t* sigs, int32_t* status, size_t n_ops, void* scratch, size_t scratch_bytes,
                    void* stream) {
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_sign: unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    if (!rho || !cap_k || !tr || !s_1_hat_mont || !s_2_hat_mont || !t_0_hat_mont || !msg_off || !rnd || !sigs)
        return fail(MLDSA_ERR_PARAM, "mldsa_hash_sign: NULL pointer");
    mldsa_params p;
    Scratch sc;
    int rc = check_call("mldsa_hash_sign", ctx, set, ph, n_keys, key_idx, n_ops, scratch, scratch_bytes, &p, &sc);
    if (rc != MLDSA_OK) return rc;
    const int dev = mldsa_ctx_device(ctx);
    if (dev < 0) return fail(MLDSA_ERR_PARAM, "mldsa_hash_sign: bad context");
    DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_hash_sign: hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    rc = launch_prehash(ph, msgs, msg_off, ctxs, ctx_off, sc.rows, sc.off, sc.bad, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    rc = mldsa_sign(ctx, set, MLDSA_MODE_PREHASH, rho, cap_k, tr, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont, n_keys, key_idx, sc.rows,
                    sc.off, ctxs, ctx_off, rnd, sigs, status, n_ops, stream);
    if (rc != MLDSA_OK) return core_failed("mldsa_hash_sign", rc);
    rc = launch_refuse(sc.bad, nullptr, sigs, (size_t)p.sig_len, status, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    const hipError_t e = hipStreamSynchronize(s);  // synchronous like mldsa_sign: statuses and signatures are final
    if (e != hipSuccess) return fail(MLDSA_ERR_DEVICE, std::string("mldsa_hash_sign: ") + hipGetErrorString(e));
    return MLDSA_OK;
}

}  // extern "C"
