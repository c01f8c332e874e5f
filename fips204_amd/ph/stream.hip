// Incremental HashML-DSA pre-hash (include/mldsa_ph.h: mldsa_ph_init / _update / _final): PH(M) of messages that arrive in
// pieces, one operation per lane like k_prehash, the hash state of every operation kept in caller-owned device memory
// between launches.
//
// State: 32-bit words, word-major -- word w of op i at state[w * n_ops + i] -- so that the 64 lanes of a wave load and
// store each word of their states as one coalesced access.
//   word 0, 1   bytes absorbed so far (64-bit count; count mod BLOCK bytes are buffered)
//   word 2      bad: a piece pair of this op was malformed (sticky)
//   SHA-224/256           8 chaining words, then the partial block as 16 little-endian dwords of message bytes
//   SHA-384/512, 512/t    8 chaining words as (lo, hi) pairs, then the partial block as 32 dwords
//   SHA-3, SHAKE          the 25 lanes of the sponge as (lo, hi) pairs; a partial block is XORed straight into them
// One instance of each kernel per family (SHA-2 with 32-bit words, SHA-2 with 64-bit words, Keccak): the functions of a family
// differ by the PhVar argument -- Keccak's rate included -- and share its state layout.
// The partial block never sits in a per-lane array (a run-time byte position into registers would land in scratch
// memory): it lies in the state as dwords of message bytes.  A piece that completes it is first appended to it there (byte
// and dword stores of the lane into its own words), then the 16 / 32 dwords are hashed as iteration 0 of the block loop;
// whole blocks inside a piece take the load_le32 path of k_prehash.  Each kernel holds one instance of its compression
// function.  (Assembling the completing block from two sources, state and piece, dword by dword was tried first: its 16 / 32
// nested branches cost 52 / 182 spilled SGPRs.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_ph.h"
#include "../csrc/keccak.h"
#include "../layer/layer_dev.h"
#include "ph_internal.h"
#include "sha2_dev.h"

namespace {

using mldsa::KeccakState;
using mldsa::load_le32;
using mldsa_layer::wave_max;
using mldsa_ph::bswap32;
using mldsa_ph::fail;
using mldsa_ph::OID_LEN;
using mldsa_ph::OID_PREFIX;
using mldsa_ph::FAM_KECCAK;
using mldsa_ph::FAM_SHA2_32;
using mldsa_ph::FAM_SHA2_64;
using mldsa_ph::FamTraits;
using mldsa_ph::PhInfo;
using mldsa_ph::PhVar;
using mldsa_ph::row_len_of;
using mldsa_ph::static_for;

constexpr int W_CNT = 0, W_BAD = 2, W_H = 3;

template <int FAM> struct StTraits;
template <> struct StTraits<FAM_SHA2_32> { static constexpr int H_WORDS = 8, BUF_WORDS = 16; };
template <> struct StTraits<FAM_SHA2_64> { static constexpr int H_WORDS = 16, BUF_WORDS = 32; };
template <> struct StTraits<FAM_KECCAK> { static constexpr int H_WORDS = 50, BUF_WORDS = 0; };  // every rate: the whole sponge
template <int FAM> constexpr int W_BUF = W_H + StTraits<FAM>::H_WORDS;
template <int FAM> constexpr int ST_WORDS = W_H + StTraits<FAM>::H_WORDS + StTraits<FAM>::BUF_WORDS;

int state_words(int ph) {
    PhInfo info;
    if (!mldsa_ph::ph_info(ph, &info)) return -1;
    switch (info.fam) {
        case FAM_SHA2_32: return ST_WORDS<FAM_SHA2_32>;
        case FAM_SHA2_64: return ST_WORDS<FAM_SHA2_64>;
        default: return ST_WORDS<FAM_KECCAK>;
    }
}

// ---- the chaining value between registers and the word-major state ----
__device__ __forceinline__ void load_h(mldsa_ph::Sha256State& h, const uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 8; i++) h.h[i] = sp[(W_H + i) * S];
}
__device__ __forceinline__ void store_h(const mldsa_ph::Sha256State& h, uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 8; i++) sp[(W_H + i) * S] = h.h[i];
}
__device__ __forceinline__ void load_h(mldsa_ph::Sha512State& h, const uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h.h[i].lo = sp[(W_H + 2 * i) * S];
        h.h[i].hi = sp[(W_H + 2 * i + 1) * S];
    }
}
__device__ __forceinline__ void store_h(const mldsa_ph::Sha512State& h, uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        sp[(W_H + 2 * i) * S] = h.h[i].lo;
        sp[(W_H + 2 * i + 1) * S] = h.h[i].hi;
    }
}
__device__ __forceinline__ void load_h(KeccakState& h, const uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 25; i++) {
        h.lo[i] = sp[(W_H + 2 * i) * S];
        h.hi[i] = sp[(W_H + 2 * i + 1) * S];
    }
}
__device__ __forceinline__ void store_h(const KeccakState& h, uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 25; i++) {
        sp[(W_H + 2 * i) * S] = h.lo[i];
        sp[(W_H + 2 * i + 1) * S] = h.hi[i];
    }
}

// Dword at byte `pos` of the padded last block: the buffered bytes below `fill`, the pad byte at `fill`, zeros after it
// (whatever the buffer holds from `fill` on is stale and masked off).
template <uint8_t PADB>
__device__ __forceinline__ uint32_t final_le32(const uint32_t* bufw, int fill, int pos) {
    // d = buffered bytes of this dword, clamped to -1 ... 4.  Shifts instead of compares: 32 of these are live side by side in
    // SHA-512, and every compare would hold an SGPR pair until its load returns (46 spilled SGPRs that way).
    const int d = min(max(fill - pos, -1), 4);
    const uint32_t keep = (uint32_t)(((1ull << (8 * (d + 1))) - 1ull) >> 8);   // low d bytes (none for d <= 0, all for d = 4)
    const uint32_t pad = (uint32_t)(((uint64_t)PADB << (8 * (d + 1))) >> 8);   // the pad byte behind them (only for d = 0 ... 3)
    return (*bufw & keep) | pad;
}

// Dword at byte `pos` of a rate block into which `take` bytes at src are absorbed from byte position `o` on; zero elsewhere.
__device__ __forceinline__ uint32_t window_le32(const uint8_t* src, int o, int take, int pos) {
    if (pos >= o && pos + 4 <= o + take) return load_le32(src + (pos - o));
    if (pos + 4 <= o || pos >= o + take) return 0;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = pos + k - o;
        if (p >= 0 && p < take) v |= (uint32_t)src[p] << (8 * k);
    }
    return v;
}

// `len` bytes at src behind the `pos` bytes the op's partial block already holds (pos + len < BLOCK): bytes up to a dword
// boundary, whole dwords, the last bytes
__device__ __forceinline__ void buf_append(uint32_t* buf0, size_t S, int pos, const uint8_t* src, int len) {
    while (len > 0 && (pos & 3)) {
        reinterpret_cast<uint8_t*>(buf0 + (size_t)(pos >> 2) * S)[pos & 3] = *src++;
        pos++;
        len--;
    }
    while (len >= 4) {
        buf0[(size_t)(pos >> 2) * S] = load_le32(src);
        src += 4;
        pos += 4;
        len -= 4;
    }
    while (len > 0) {
        reinterpret_cast<uint8_t*>(buf0 + (size_t)(pos >> 2) * S)[pos & 3] = *src++;
        pos++;
        len--;
    }
}

template <int FAM>
__global__ __launch_bounds__(64) void k_ph_init(uint32_t* __restrict__ st, size_t n_ops, PhVar var) {
    const size_t op = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (op >= n_ops) return;
    uint32_t* sp = st + op;
    const size_t S = n_ops;
    sp[W_CNT * S] = 0;
    sp[(W_CNT + 1) * S] = 0;
    sp[W_BAD * S] = 0;
    if constexpr (FAM == FAM_SHA2_32) {
        mldsa_ph::Sha256State h;
        mldsa_ph::sha256_init(h, var.iv);
        store_h(h, sp, S);
    } else if constexpr (FAM == FAM_SHA2_64) {
        mldsa_ph::Sha512State h;
        mldsa_ph::sha512_init(h, var.iv);
        store_h(h, sp, S);
    } else {
#pragma unroll
        for (int i = 0; i < 50; i++) sp[(W_H + i) * S] = 0;
    }
}

// the update of one lane's op for block size / rate B, a compile-time constant (k_ph_update below)
template <int FAM, int B>
__device__ __forceinline__ void update_body(uint32_t* __restrict__ st, const uint8_t* __restrict__ pieces,
                                            const uint64_t* __restrict__ off, size_t n_ops, size_t first, size_t count,
                                            uint64_t win_lo, uint64_t win_hi, uint64_t sub) {
    const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t S = n_ops;
    uint32_t* sp = st;
    const uint8_t* mp = nullptr;
    size_t plen = 0;
    int fill = 0;
    if (idx < count) {
        const size_t op = first + idx;
        sp = st + op;
        // the rule of k_prehash: the call vouches for [off[0], off[n_ops]); a pair outside it in order is refused unread
        const uint64_t p0 = off[op], p1 = off[op + 1];
        bool now_bad = !(off[0] <= p0 && p0 <= p1 && p1 <= off[n_ops]);
        now_bad |= p1 != p0 && pieces == nullptr;
        const bool was_bad = sp[W_BAD * S] != 0;
        if (now_bad && !was_bad) sp[W_BAD * S] = 1;
        if (!now_bad && !was_bad) {
            const uint64_t a = p0 > win_lo ? p0 : win_lo, b = p1 < win_hi ? p1 : win_hi;
            if (b > a) {
                mp = pieces + (a - sub);
                plen = (size_t)(b - a);
                const uint64_t cnt = ((uint64_t)sp[(W_CNT + 1) * S] << 32) | sp[W_CNT * S];
                fill = (int)(cnt % B);
                const uint64_t cnt2 = cnt + plen;
                sp[W_CNT * S] = (uint32_t)cnt2;
                sp[(W_CNT + 1) * S] = (uint32_t)(cnt2 >> 32);
            }
        }
    }
    const bool active = plen > 0;

    if constexpr (FAM == FAM_KECCAK) {
        constexpr int RW = B / 8;  // 64-bit words of the rate
        // iterations of this lane: [the bytes that continue a partial block] [whole blocks] [the bytes left over]
        const bool head = active && fill > 0;
        const int take0 = head ? (int)((size_t)(B - fill) < plen ? (size_t)(B - fill) : plen) : 0;
        const size_t rest = plen - take0;
        const size_t nblk = rest / B;
        const int rem = (int)(rest % B);
        const size_t my_iters = (head ? 1 : 0) + nblk + (rem ? 1 : 0);
        const size_t max_iters = wave_max(my_iters);
        KeccakState ks;
        if (active) load_h(ks, sp, S);
        for (size_t b = 0; b < max_iters; b++) {
            if (b < my_iters) {
                const bool is_head = head && b == 0;
                const size_t j = b - (head ? 1 : 0);
                const uint8_t* src = is_head ? mp : mp + take0 + j * B;
                const int o = is_head ? fill : 0;
                const int take = is_head ? take0 : j < nblk ? B : rem;
                if (take == B) {
                    static_for<0, RW>([&](auto wc) {
                        constexpr int W = decltype(wc)::value;
                        ks.lo[W] ^= load_le32(src + 8 * W);
                        ks.hi[W] ^= load_le32(src + 8 * W + 4);
                    });
                } else {
                    static_for<0, RW>([&](auto wc) {
                        constexpr int W = decltype(wc)::value;
                        ks.lo[W] ^= window_le32(src, o, take, 8 * W);
                        ks.hi[W] ^= window_le32(src, o, take, 8 * W + 4);
                    });
                }
                if (o + take == B) mldsa::keccak_f1600(ks);
            }
        }
        if (active) store_h(ks, sp, S);
    } else {
        // a lane whose piece completes its partial block first completes it where it lies, in the state; iteration 0 of that
        // lane hashes the 16 / 32 buffered dwords, the other iterations hash whole blocks of the piece
        const bool head = active && fill > 0 && (size_t)fill + plen >= (size_t)B;
        const int take0 = head ? B - fill : 0;
        const size_t nblk = (active && (fill == 0 || head)) ? (plen - take0) / B : 0;
        const size_t my_iters = (head ? 1 : 0) + nblk;
        const size_t max_iters = wave_max(my_iters);
        const uint8_t* body = mp + take0;
        uint32_t* buf0 = sp + (size_t)W_BUF<FAM> * S;
        if (head) buf_append(buf0, S, fill, mp, take0);
        if constexpr (FAM == FAM_SHA2_32) {
            mldsa_ph::Sha256State h;
            if (my_iters) load_h(h, sp, S);
            for (size_t b = 0; b < max_iters; b++) {
                if (b < my_iters) {
                    uint32_t w[16];
                    if (head && b == 0) {
#pragma unroll
                        for (int i = 0; i < 16; i++) w[i] = bswap32(buf0[(size_t)i * S]);
                    } else {
                        const uint8_t* p = body + (b - (head ? 1 : 0)) * 64;
#pragma unroll
                        for (int i = 0; i < 16; i++) w[i] = bswap32(load_le32(p + 4 * i));
                    }
                    mldsa_ph::sha256_block(h, w);
                }
            }
            if (my_iters) store_h(h, sp, S);
        } else {
            mldsa_ph::Sha512State h;
            if (my_iters) load_h(h, sp, S);
            for (size_t b = 0; b < max_iters; b++) {
                if (b < my_iters) {
                    mldsa_ph::U64 w[16];
                    if (head && b == 0) {
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            w[i].hi = bswap32(buf0[(size_t)(2 * i) * S]);
                            w[i].lo = bswap32(buf0[(size_t)(2 * i + 1) * S]);
                        }
                    } else {
                        const uint8_t* p = body + (b - (head ? 1 : 0)) * 128;
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            w[i].hi = bswap32(load_le32(p + 8 * i));
                            w[i].lo = bswap32(load_le32(p + 8 * i + 4));
                        }
                    }
                    mldsa_ph::sha512_block(h, w);
                }
            }
            if (my_iters) store_h(h, sp, S);
        }
        if (active) {  // what is left of the piece joins the partial block (which is empty after a completed one)
            const size_t used = take0 + nblk * B;
            buf_append(buf0, S, my_iters ? 0 : fill, mp + used, (int)(plen - used));
        }
    }
}

// One kernel per family.  Keccak's five rates are five inlined copies of the body behind a wave-uniform switch: with the rate
// as a run-time bound the absorbing loop's 42 guarded dwords cost 4 spilled SGPRs (38 unguarded).
template <int FAM>
__global__ __launch_bounds__(64) void k_ph_update(uint32_t* __restrict__ st, const uint8_t* __restrict__ pieces,
                                                  const uint64_t* __restrict__ off, size_t n_ops, size_t first, size_t count,
                                                  uint64_t win_lo, uint64_t win_hi, uint64_t sub, PhVar var) {
    if constexpr (FAM == FAM_SHA2_32) {
        update_body<FAM, 64>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub);
    } else if constexpr (FAM == FAM_SHA2_64) {
        update_body<FAM, 128>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub);
    } else {
        switch (var.block) {
            case 168: update_body<FAM, 168>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub); break;
            case 144: update_body<FAM, 144>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub); break;
            case 136: update_body<FAM, 136>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub); break;
            case 104: update_body<FAM, 104>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub); break;
            default: update_body<FAM, 72>(st, pieces, off, n_ops, first, count, win_lo, win_hi, sub); break;
        }
    }
}

template <int FAM>
__global__ __launch_bounds__(64) void k_ph_final(const uint32_t* __restrict__ st, uint8_t* __restrict__ out,
                                                 uint64_t* __restrict__ out_off, uint8_t* __restrict__ bad, size_t n_ops, PhVar var) {
    using T = FamTraits<FAM, FAM == FAM_SHA2_32 ? 64 : FAM == FAM_SHA2_64 ? 128 : 168>;  // TAIL and MAX_DIGEST: any rate's
    const int B = FAM == FAM_SHA2_32 ? 64 : FAM == FAM_SHA2_64 ? 128 : (int)var.block;
    const int digest = var.digest;
    const size_t row_len = (size_t)OID_LEN + digest;
    const size_t op = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (op >= n_ops) return;
    const size_t S = n_ops;
    const uint32_t* sp = st + op;
    const uint64_t cnt = ((uint64_t)sp[(W_CNT + 1) * S] << 32) | sp[W_CNT * S];
    const bool is_bad = sp[W_BAD * S] != 0;
    const int fill = (int)(cnt % B);
    const uint32_t* buf0 = sp + (size_t)W_BUF<FAM> * S;

    uint8_t dig[T::MAX_DIGEST];
    if constexpr (FAM == FAM_SHA2_32) {
        mldsa_ph::Sha256State h;
        load_h(h, sp, S);
        const int blocks = fill + T::TAIL > B ? 2 : 1;
#pragma unroll 1
        for (int b = 0; b < 2; b++) {  // one instance of the compression function
            if (b < blocks) {
                uint32_t w[16];
#pragma unroll
                for (int i = 0; i < 16; i++) w[i] = b == 0 ? bswap32(final_le32<0x80>(buf0 + (size_t)i * S, fill, 4 * i)) : 0u;
                if (b == blocks - 1) {  // 64-bit big-endian bit length
                    w[14] = (uint32_t)(cnt >> 29);
                    w[15] = (uint32_t)(cnt << 3);
                }
                mldsa_ph::sha256_block(h, w);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) dig[4 * i + k] = (uint8_t)(h.h[i] >> (24 - 8 * k));
    } else if constexpr (FAM == FAM_SHA2_64) {
        mldsa_ph::Sha512State h;
        load_h(h, sp, S);
        const int blocks = fill + T::TAIL > B ? 2 : 1;
#pragma unroll 1
        for (int b = 0; b < 2; b++) {  // one instance of the compression function
            if (b < blocks) {
                mldsa_ph::U64 w[16];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    w[i].hi = b == 0 ? bswap32(final_le32<0x80>(buf0 + (size_t)(2 * i) * S, fill, 8 * i)) : 0u;
                    w[i].lo = b == 0 ? bswap32(final_le32<0x80>(buf0 + (size_t)(2 * i + 1) * S, fill, 8 * i + 4)) : 0u;
                }
                if (b == blocks - 1) {  // 128-bit big-endian bit length
                    w[14] = {(uint32_t)(cnt >> 61), 0u};
                    w[15] = {(uint32_t)(cnt << 3), (uint32_t)(cnt >> 29)};
                }
                mldsa_ph::sha512_block(h, w);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                dig[8 * i + k] = (uint8_t)(h.h[i].hi >> (24 - 8 * k));
                dig[8 * i + 4 + k] = (uint8_t)(h.h[i].lo >> (24 - 8 * k));
            }
    } else {
        KeccakState ks;
        load_h(ks, sp, S);
        const int rw = B >> 3;
        const uint32_t pad = (uint32_t)var.padb << (8 * (fill & 3));
        static_for<0, 21>([&](auto wc) {  // the pad byte at `fill` (< rate), and 0x80 in the last byte of this rate's block
            constexpr int W = decltype(wc)::value;
            if ((fill >> 2) == 2 * W) ks.lo[W] ^= pad;
            if ((fill >> 2) == 2 * W + 1) ks.hi[W] ^= pad;
            if (W == rw - 1) ks.hi[W] ^= 0x80000000u;
        });
        mldsa::keccak_f1600(ks);
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                dig[8 * i + k] = (uint8_t)(ks.lo[i] >> (8 * k));
                dig[8 * i + 4 + k] = (uint8_t)(ks.hi[i] >> (8 * k));
            }
    }

    const bool live = !is_bad;
    uint8_t* row = out + op * row_len;
#pragma unroll
    for (int i = 0; i < 10; i++) row[i] = live ? OID_PREFIX[i] : 0;
    row[10] = live ? var.oid_last : 0;
#pragma unroll
    for (int i = 0; i < T::MAX_DIGEST; i++)  // a truncated digest ends the row: nothing behind it is written
        if (i < digest) row[OID_LEN + i] = live ? dig[i] : 0;
    if (bad) bad[op] = is_bad ? 1 : 0;
    if (out_off) {
        out_off[op] = (uint64_t)op * row_len;
        if (op == n_ops - 1) out_off[n_ops] = (uint64_t)n_ops * row_len;
    }
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MLDSA_ERR_DEVICE, std::string(what) + " launch: " + hipGetErrorString(e));
    return MLDSA_OK;
}

// the checks shared by init / update / final, all before anything is launched; *go = 0 for a successful empty call
int check_state(const char* fn, mldsa_ctx* ctx, int ph, const void* state, size_t state_bytes, size_t n_ops, int* dev, int* go) {
    *go = 0;
    if (row_len_of(ph) < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown ph");
    if (n_ops == 0) return MLDSA_OK;
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    const size_t need = mldsa_ph::state_bytes_of(ph, n_ops);
    if (!state || need == 0 || state_bytes < need || ((uintptr_t)state & 7) != 0)
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": state is NULL, misaligned or smaller than mldsa_ph_state_bytes");
    *dev = mldsa_ctx_device(ctx);
    if (*dev < 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": bad context");
    *go = 1;
    return MLDSA_OK;
}

}  // namespace

namespace mldsa_ph {

size_t state_bytes_of(int ph, size_t n_ops) {
    const int words = state_words(ph);
    if (words < 0) return 0;
    if (n_ops >= ~(size_t)0 / 256) return 0;
    return 4 * (size_t)words * n_ops;
}

int launch_init(int ph, uint32_t* state, size_t n_ops, hipStream_t s) {
    PhInfo info;
    if (!ph_info(ph, &info)) return fail(MLDSA_ERR_PARAM, "k_ph_init launch: unknown ph");
    const dim3 grid((unsigned)((n_ops + 63) / 64)), block(64);
    switch (info.fam) {
        case FAM_SHA2_32: hipLaunchKernelGGL(k_ph_init<FAM_SHA2_32>, grid, block, 0, s, state, n_ops, info.var); break;
        case FAM_SHA2_64: hipLaunchKernelGGL(k_ph_init<FAM_SHA2_64>, grid, block, 0, s, state, n_ops, info.var); break;
        default: hipLaunchKernelGGL(k_ph_init<FAM_KECCAK>, grid, block, 0, s, state, n_ops, info.var); break;
    }
    return launched("k_ph_init");
}

int launch_update(int ph, uint32_t* state, const uint8_t* pieces, const uint64_t* off, size_t n_ops, size_t first, size_t count,
                  uint64_t win_lo, uint64_t win_hi, uint64_t sub, hipStream_t s) {
    PhInfo info;
    if (!ph_info(ph, &info)) return fail(MLDSA_ERR_PARAM, "k_ph_update launch: unknown ph");
    if (count == 0) return MLDSA_OK;
    const dim3 grid((unsigned)((count + 63) / 64)), block(64);
    switch (info.fam) {
        case FAM_SHA2_32:
            hipLaunchKernelGGL(k_ph_update<FAM_SHA2_32>, grid, block, 0, s, state, pieces, off, n_ops, first, count, win_lo, win_hi, sub, info.var);
            break;
        case FAM_SHA2_64:
            hipLaunchKernelGGL(k_ph_update<FAM_SHA2_64>, grid, block, 0, s, state, pieces, off, n_ops, first, count, win_lo, win_hi, sub, info.var);
            break;
        default:
            hipLaunchKernelGGL(k_ph_update<FAM_KECCAK>, grid, block, 0, s, state, pieces, off, n_ops, first, count, win_lo, win_hi, sub, info.var);
            break;
    }
    return launched("k_ph_update");
}

int launch_final(int ph, const uint32_t* state, uint8_t* out, uint64_t* out_off, uint8_t* bad, size_t n_ops, hipStream_t s) {
    PhInfo info;
    if (!ph_info(ph, &info)) return fail(MLDSA_ERR_PARAM, "k_ph_final launch: unknown ph");
    const dim3 grid((unsigned)((n_ops + 63) / 64)), block(64);
    switch (info.fam) {
        case FAM_SHA2_32: hipLaunchKernelGGL(k_ph_final<FAM_SHA2_32>, grid, block, 0, s, state, out, out_off, bad, n_ops, info.var); break;
        case FAM_SHA2_64: hipLaunchKernelGGL(k_ph_final<FAM_SHA2_64>, grid, block, 0, s, state, out, out_off, bad, n_ops, info.var); break;
        default: hipLaunchKernelGGL(k_ph_final<FAM_KECCAK>, grid, block, 0, s, state, out, out_off, bad, n_ops, info.var); break;
    }
    return launched("k_ph_final");
}

}  // namespace mldsa_ph

extern "C" {

size_t mldsa_ph_state_bytes(int ph, size_t n_ops) { return mldsa_ph::state_bytes_of(ph, n_ops); }

int mldsa_ph_init(mldsa_ctx* ctx, int ph, void* state, size_t state_bytes, size_t n_ops, void* stream) {
    int dev, go;
    const int rc = check_state("mldsa_ph_init", ctx, ph, state, state_bytes, n_ops, &dev, &go);
    if (!go) return rc;
    mldsa_ph::DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_ph_init: hipSetDevice failed");
    return mldsa_ph::launch_init(ph, static_cast<uint32_t*>(state), n_ops, (hipStream_t)stream);
}

int mldsa_ph_update(mldsa_ctx* ctx, int ph, void* state, size_t state_bytes, const uint8_t* pieces, const uint64_t* piece_off,
                    size_t n_ops, void* stream) {
    int dev, go;
    const int rc = check_state("mldsa_ph_update", ctx, ph, state, state_bytes, n_ops, &dev, &go);
    if (!go) return rc;
    if (!piece_off) return fail(MLDSA_ERR_PARAM, "mldsa_ph_update: NULL pointer");
    mldsa_ph::DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_ph_update: hipSetDevice failed");
    return mldsa_ph::launch_update(ph, static_cast<uint32_t*>(state), pieces, piece_off, n_ops, 0, n_ops, 0, ~(uint64_t)0, 0,
                                   (hipStream_t)stream);
}

int mldsa_ph_final(mldsa_ctx* ctx, int ph, void* state, size_t state_bytes, uint8_t* out, uint64_t* out_off, uint8_t* bad,
                   size_t n_ops, void* stream) {
    int dev, go;
    const int rc = check_state("mldsa_ph_final", ctx, ph, state, state_bytes, n_ops, &dev, &go);
    if (!go) return rc;
    if (!out) return fail(MLDSA_ERR_PARAM, "mldsa_ph_final: NULL pointer");
    mldsa_ph::DeviceScope ds(dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, "mldsa_ph_final: hipSetDevice failed");
    return mldsa_ph::launch_final(ph, static_cast<const uint32_t*>(state), out, out_off, bad, n_ops, (hipStream_t)stream);
}

}  // extern "C"
