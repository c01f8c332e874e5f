// libmldsa_mus.so (include/mldsa_mus.h): mu = H(tr | M', 64) of messages that arrive in pieces, and of raw messages of any size in host
// memory, layered on the core's C ABI.  One SHAKE256 sponge per op lives in caller-owned device memory between the launches:
//   52 32-bit words per op, word-major -- word w of op i at state[w * n_ops + i], so the 64 lanes of a wave load and store each word of
//   their states as one coalesced access --: word 0 the bytes in the current rate block, word 1 the op's flag, words 2 ... 51 the 25
//   lanes of the sponge as (lo, hi) pairs.  A partial block is XORed straight into the sponge words: SHAKE needs no total length.
// Each of init / update / final has two kernels on that one layout:
//   k_mus_*_lane   one op per lane on mldsa::keccak_f1600.  update: the bytes that complete a partial block and the bytes left over
//                  behind the last whole block are XORed into the op's state words where they lie, in memory (a run-time byte position
//                  into registers would land in scratch memory); whole rate blocks inside a piece load as unaligned dwords.  The block
//                  loop runs to the wave's maximum with the lanes masked past their own count.
//   k_mus_*_wave   one op per wave on the core's bit-interleaved cooperative sponge (../csrc/keccak_coop2.h), taken by calls of at
//                  most MLDSA_MUS_WAVE_MAX_OPS ops: such a call is a serial chain of permutations, and the cooperative permutation is
//                  the shorter one.  The lanes that hold a rate word load their own (lo, hi) of each block; (lo, hi) <-> (E, O) at
//                  load, absorb and store.  Every cross-lane step is executed by the whole wave: what decides a branch around one is
//                  the same in all 64 lanes.
// mldsa_mus_host_compute streams [msg_off[0], msg_off[n_ops]) through the layers' host-memory feed (../layer/host_feed.h): chunk i + 1 is
// uploaded on the copy stream while the update absorbs chunk i on the compute stream, launched for the ops that have bytes in the chunk
// only, with the chunk as the window of message offsets, so the one offset table uploaded at the start serves every chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/mldsa_mus.h"
#include "../csrc/keccak_coop2.h"
#include "../layer/host_chunks.h"
#include "../layer/host_feed.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"

struct mldsa_mus_host {
    std::mutex lock;  // one call at a time
    mldsa_layer::HostFeed feed;
    // per-batch buffers, kept and grown: the message offsets, the ctx offsets and ctxs (at most 256 bytes kept per op), the states
    size_t cap_ops = 0;
    uint64_t* d_off = nullptr;
    uint64_t* d_coff = nullptr;
    uint8_t* d_ctxs = nullptr;
    uint32_t* d_state = nullptr;
    std::vector<uint64_t> h_coff;
    std::vector<uint8_t> h_ctxs;
};

namespace {

using namespace mldsa_layer;
using mldsa::Coop2Lane;
using mldsa::load_le32;
using mldsa_layer::piece_hi;
using mldsa_layer::piece_lo;

constexpr int RATE = mldsa::SHAKE256_RATE;  // 136
constexpr int RATE_W = RATE / 8;            // 17 64-bit words
constexpr int W_FILL = 0, W_FLAG = 1, W_ST = 2, ST_WORDS = 52;
constexpr int MAX_CTX_KEPT = 256;  // of a longer ctx the host-memory call uploads this much: still longer than 255, flag 1

// ------------------------------------------------------------------------------------------------------------------ prefix
// What precedes the message: tr (MLDSA_MODE_INTERNAL) or tr | domain | len(ctx) | ctx.  The checks and their precedence are k_mu_ext's
// (mu/mu.hip): a ctx pair not in order inside [ctx_off[0], ctx_off[n_ops]] or naming bytes of a NULL ctxs (flag 2), then a ctx longer
// than 255 bytes (flag 1), then a key index outside the table (flag 2).  Nothing of a flagged op is read.
struct Prefix {
    const uint8_t* trp;
    const uint8_t* cp;
    int total;  // bytes: 64, or 66 + len(ctx); 0 for a flagged op
    int flag;
    uint32_t domain;
};

__device__ __forceinline__ Prefix check_prefix(const uint8_t* __restrict__ tr, uint32_t n_keys, const uint32_t* __restrict__ key_idx, int mode,
                                               const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off, size_t op, size_t n_ops) {
    Prefix p = {nullptr, nullptr, 0, 0, mode == MLDSA_MODE_PREHASH ? 1u : 0u};
    bool bad_off = false;
    uint64_t c0 = 0, clen = 0;
    if (ctx_off) {
        c0 = ctx_off[op];
        const uint64_t c1 = ctx_off[op + 1];
        bad_off = !(ctx_off[0] <= c0 && c0 <= c1 && c1 <= ctx_off[n_ops]);
        clen = c1 - c0;
        bad_off |= clen != 0 && ctxs == nullptr;
    }
    const size_t key = key_idx ? (size_t)key_idx[op] : op;
    p.flag = bad_off ? 2 : clen > 255 ? 1 : key >= n_keys ? 2 : 0;
    if (p.flag == 0) {
        p.trp = tr + key * 64;
        p.cp = ctxs + c0;
        p.total = mode == MLDSA_MODE_INTERNAL ? 64 : 66 + (int)clen;
    }
    return p;
}

__device__ __forceinline__ uint32_t prefix_byte(const Prefix& p, int pos) {
    if (pos >= p.total) return 0u;
    if (pos < 64) return p.trp[pos];
    return pos == 64 ? p.domain : pos == 65 ? (uint32_t)(p.total - 66) : p.cp[pos - 66];
}

// the dword at byte `pos` of the prefix, zero behind its end; whole dwords of tr and of the ctx are one byte-granular load each
__device__ __forceinline__ uint32_t prefix_le32(const Prefix& p, int pos) {
    if (pos + 4 <= 64) return load_le32(p.trp + pos);
    if (pos >= p.total) return 0u;
    if (pos >= 66 && pos + 4 <= p.total) return load_le32(p.cp + (pos - 66));
    return prefix_byte(p, pos) | (prefix_byte(p, pos + 1) << 8) | (prefix_byte(p, pos + 2) << 16) | (prefix_byte(p, pos + 3) << 24);
}

// ------------------------------------------------------------------------------------------------------ lane form: helpers
__device__ __forceinline__ void load_state(mldsa::KeccakState& ks, const uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 25; i++) {
        ks.lo[i] = sp[(size_t)(W_ST + 2 * i) * S];
        ks.hi[i] = sp[(size_t)(W_ST + 2 * i + 1) * S];
    }
}

__device__ __forceinline__ void store_state(const mldsa::KeccakState& ks, uint32_t* sp, size_t S) {
#pragma unroll
    for (int i = 0; i < 25; i++) {
        sp[(size_t)(W_ST + 2 * i) * S] = ks.lo[i];
        sp[(size_t)(W_ST + 2 * i + 1) * S] = ks.hi[i];
    }
}

// `len` bytes at src are XORed into the op's sponge words in memory from byte `pos` of the rate block on (pos + len <= RATE): bytes
// up to a dword boundary, whole dwords, the last bytes.  Byte `pos` of the block lies in state word W_ST + pos / 4.
__device__ __forceinline__ void xor_into_state(uint32_t* sp, size_t S, int pos, const uint8_t* src, int len) {
    while (len > 0 && (pos & 3)) {
        sp[(size_t)(W_ST + (pos >> 2)) * S] ^= (uint32_t)*src++ << (8 * (pos & 3));
        pos++;
        len--;
    }
    while (len >= 4) {
        sp[(size_t)(W_ST + (pos >> 2)) * S] ^= load_le32(src);
        src += 4;
        pos += 4;
        len -= 4;
    }
    while (len > 0) {
        sp[(size_t)(W_ST + (pos >> 2)) * S] ^= (uint32_t)*src++ << (8 * (pos & 3));
        pos++;
        len--;
    }
}

// the pad of SHAKE256 on a state that holds `fill` bytes of the current block: 0x1F at byte `fill`, 0x80 on the block's last byte
__device__ __forceinline__ void pad_state(mldsa::KeccakState& ks, int fill) {
    const uint32_t pad = 0x1Fu << (8 * (fill & 3));
    const int dw = fill >> 2;
#pragma unroll
    for (int w = 0; w < RATE_W; w++) {
        ks.lo[w] ^= dw == 2 * w ? pad : 0u;  // selects: a guarded store per word would be turned into one indexed store, in scratch
        ks.hi[w] ^= dw == 2 * w + 1 ? pad : 0u;
    }
    ks.hi[RATE_W - 1] ^= 0x80000000u;
}

// ------------------------------------------------------------------------------------------------------ lane form: kernels
__global__ __launch_bounds__(64) void k_mus_init_lane(const uint8_t* __restrict__ tr, uint32_t n_keys, const uint32_t* __restrict__ key_idx,
                                                      int mode, const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off,
                                                      uint32_t* __restrict__ st, size_t n_ops) {
    const size_t op = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (op >= n_ops) return;  // nothing below crosses lanes
    const Prefix p = check_prefix(tr, n_keys, key_idx, mode, ctxs, ctx_off, op, n_ops);
    const int full = p.total / RATE;  // whole blocks of the prefix: 0 ... 2; 0 for a flagged op
    mldsa::KeccakState ks;
    mldsa::keccak_zero(ks);
#pragma unroll 1
    for (int b = 0; b < 3; b++) {  // one instance of the permutation
        if (b * RATE < p.total) {
#pragma unroll
            for (int w = 0; w < RATE_W; w++) {
                ks.lo[w] ^= prefix_le32(p, b * RATE + 8 * w);
                ks.hi[w] ^= prefix_le32(p, b * RATE + 8 * w + 4);
            }
        }
        if (b < full) mldsa::keccak_f1600(ks);
    }
    uint32_t* sp = st + op;
    sp[(size_t)W_FILL * n_ops] = (uint32_t)(p.total % RATE);
    sp[(size_t)W_FLAG * n_ops] = (uint32_t)p.flag;
    store_state(ks, sp, n_ops);
}

// ops [first, first + count) absorb the bytes of their pair that fall into the window [win_lo, win_hi) of offsets; offset `sub` is
// byte 0 of `pieces`.  The public call: every op, the whole range of offsets, sub = 0.
__global__ __launch_bounds__(64) void k_mus_update_lane(uint32_t* __restrict__ st, const uint8_t* __restrict__ pieces,
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
        const uint64_t p0 = off[op], p1 = off[op + 1];
        const bool now_bad = !(off[0] <= p0 && p0 <= p1 && p1 <= off[n_ops]) || (p1 != p0 && pieces == nullptr);
        const bool flagged = sp[(size_t)W_FLAG * S] != 0;  // sticky: a flagged op reads no further byte, and its first flag stays
        if (now_bad && !flagged) sp[(size_t)W_FLAG * S] = 2u;
        if (!now_bad && !flagged) {
            const uint64_t a = piece_lo(p0, win_lo), b = piece_hi(p1, win_hi);
            if (b > a) {
                mp = pieces + (a - sub);
                plen = (size_t)(b - a);
                fill = (int)sp[(size_t)W_FILL * S];
            }
        }
    }
    // this lane's piece: [take0 bytes that continue the partial block] [nblk whole blocks] [rem bytes left over]
    const int take0 = fill > 0 ? (int)((size_t)(RATE - fill) < plen ? (size_t)(RATE - fill) : plen) : 0;
    const bool completes = fill > 0 && fill + take0 == RATE;
    const size_t rest = plen - take0;  // not 0 only behind a block boundary
    const size_t nblk = rest / RATE;
    const int rem = (int)(rest % RATE);
    if (take0) xor_into_state(sp, S, fill, mp, take0);
    const size_t my_iters = (completes ? 1 : 0) + nblk;
    const size_t max_iters = wave_max(my_iters);  // by the whole wave
    const uint8_t* body = mp + take0;
    mldsa::KeccakState ks;
    if (my_iters) load_state(ks, sp, S);
    for (size_t b = 0; b < max_iters; b++) {
        if (b < my_iters) {
            if (!(completes && b == 0)) {  // iteration 0 of a completed block permutes what the state already holds
                const uint8_t* src = body + (b - (completes ? 1 : 0)) * RATE;
#pragma unroll
                for (int w = 0; w < RATE_W; w++) {
                    ks.lo[w] ^= load_le32(src + 8 * w);
                    ks.hi[w] ^= load_le32(src + 8 * w + 4);
                }
            }
            mldsa::keccak_f1600(ks);
        }
    }
    if (my_iters) store_state(ks, sp, S);
    if (rem) xor_into_state(sp, S, 0, body + nblk * RATE, rem);
    if (plen) sp[(size_t)W_FILL * S] = (uint32_t)((fill + plen) % RATE);
}

__global__ __launch_bounds__(64) void k_mus_final_lane(const uint32_t* __restrict__ st, uint8_t* __restrict__ mu, int32_t* __restrict__ mu_flag,
                                                       size_t n_ops) {
    const size_t op = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (op >= n_ops) return;
    const uint32_t* sp = st + op;
    const int fill = (int)sp[(size_t)W_FILL * n_ops];
    const int flag = (int)sp[(size_t)W_FLAG * n_ops];
    mldsa::KeccakState ks;  // a copy: the state in memory stays as it is
    load_state(ks, sp, n_ops);
    pad_state(ks, fill);
    mldsa::keccak_f1600(ks);
    u32_any* out = reinterpret_cast<u32_any*>(mu + op * 64);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        out[2 * i] = flag == 0 ? ks.lo[i] : 0u;
        out[2 * i + 1] = flag == 0 ? ks.hi[i] : 0u;
    }
    if (mu_flag) mu_flag[op] = flag;
}

// ------------------------------------------------------------------------------------------------------ wave form: helpers
// the lane's half word of the op's state / the state from the lanes' half words.  Both lanes of a word load its (lo, hi); the lane of
// the even half stores them.  By the whole wave.
__device__ __forceinline__ uint32_t wave_load(const uint32_t* sp, size_t S, const Coop2Lane& c) {
    uint32_t lo = 0, hi = 0;
    if (c.active) {
        lo = sp[(size_t)(W_ST + 2 * c.word) * S];
        hi = sp[(size_t)(W_ST + 2 * c.word + 1) * S];
    }
    return mldsa::coop2_from_lohi(lo, hi, c);
}

__device__ __forceinline__ void wave_store(uint32_t v, int lane, const Coop2Lane& c, uint32_t* sp, size_t S) {
    uint32_t lo, hi;
    mldsa::coop2_to_lohi(v, lane, lo, hi);
    if (lane < 32 && c.active) {
        sp[(size_t)(W_ST + 2 * c.word) * S] = lo;
        sp[(size_t)(W_ST + 2 * c.word + 1) * S] = hi;
    }
}

// Dword at byte `pos` of a rate block into which `take` bytes at src are absorbed from byte `o` of the block on; zero elsewhere.
__device__ __forceinline__ uint32_t block_le32(const uint8_t* src, int o, int take, int pos) {
    const int rel = pos - o;
    if (rel >= 0 && rel + 4 <= take) return load_le32(src + rel);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = rel + k;
        if (q >= 0 && q < take) v |= (uint32_t)src[q] << (8 * k);
    }
    return v;
}

// ------------------------------------------------------------------------------------------------------ wave form: kernels
// One op per wave: block blockIdx.x works on op first + blockIdx.x (the launch has exactly as many blocks as ops).  The op's pair, fill
// and flag are the same in all 64 lanes, so is every branch taken on them.
__global__ __launch_bounds__(64) void k_mus_init_wave(const uint8_t* __restrict__ tr, uint32_t n_keys, const uint32_t* __restrict__ key_idx,
                                                      int mode, const uint8_t* __restrict__ ctxs, const uint64_t* __restrict__ ctx_off,
                                                      uint32_t* __restrict__ st, size_t n_ops) {
    const int lane = threadIdx.x;
    const size_t op = blockIdx.x;
    const Coop2Lane c = mldsa::coop2_lane(lane);
    const Prefix p = check_prefix(tr, n_keys, key_idx, mode, ctxs, ctx_off, op, n_ops);
    const int full = p.total / RATE;
    const bool absorbs = c.active && c.word < RATE_W;
    uint32_t v = 0;
    for (int b = 0; b * RATE < p.total; b++) {
        if (absorbs) v ^= mldsa::coop2_from_lohi(prefix_le32(p, b * RATE + 8 * c.word), prefix_le32(p, b * RATE + 8 * c.word + 4), c);
        if (b < full) mldsa::keccak_f1600_coop2(v, c);
    }
    uint32_t* sp = st + op;
    wave_store(v, lane, c, sp, n_ops);
    if (lane == 63) {
        sp[(size_t)W_FILL * n_ops] = (uint32_t)(p.total % RATE);
        sp[(size_t)W_FLAG * n_ops] = (uint32_t)p.flag;
    }
}

__global__ __launch_bounds__(64) void k_mus_update_wave(uint32_t* __restrict__ st, const uint8_t* __restrict__ pieces,
                                                        const uint64_t* __restrict__ off, size_t n_ops, size_t first, uint64_t win_lo,
                                                        uint64_t win_hi, uint64_t sub) {
    const int lane = threadIdx.x;
    const size_t op = first + blockIdx.x;
    const size_t S = n_ops;
    uint32_t* sp = st + op;
    const Coop2Lane c = mldsa::coop2_lane(lane);
    const uint64_t p0 = off[op], p1 = off[op + 1];
    const bool now_bad = !(off[0] <= p0 && p0 <= p1 && p1 <= off[n_ops]) || (p1 != p0 && pieces == nullptr);
    const bool flagged = sp[(size_t)W_FLAG * S] != 0;
    const uint64_t a = piece_lo(p0, win_lo), b = piece_hi(p1, win_hi);
    if (now_bad || flagged || b <= a) {  // the whole wave leaves
        if (now_bad && !flagged && lane == 63) sp[(size_t)W_FLAG * S] = 2u;
        return;
    }
    const uint8_t* src = pieces + (a - sub);
    size_t left = (size_t)(b - a);
    int o = (int)sp[(size_t)W_FILL * S];
    const bool absorbs = c.active && c.word < RATE_W;
    uint32_t v = wave_load(sp, S, c);
    while (left > 0) {
        const int take = (size_t)(RATE - o) < left ? RATE - o : (int)left;
        if (absorbs) v ^= mldsa::coop2_from_lohi(block_le32(src, o, take, 8 * c.word), block_le32(src, o, take, 8 * c.word + 4), c);
        o += take;
        if (o == RATE) {
            mldsa::keccak_f1600_coop2(v, c);
            o = 0;
        }
        src += take;
        left -= take;
    }
    wave_store(v, lane, c, sp, S);
    if (lane == 63) sp[(size_t)W_FILL * S] = (uint32_t)o;
}

__global__ __launch_bounds__(64) void k_mus_final_wave(const uint32_t* __restrict__ st, uint8_t* __restrict__ mu, int32_t* __restrict__ mu_flag,
                                                       size_t n_ops) {
    const int lane = threadIdx.x;
    const size_t op = blockIdx.x;
    const uint32_t* sp = st + op;
    const Coop2Lane c = mldsa::coop2_lane(lane);
    const int fill = (int)sp[(size_t)W_FILL * n_ops];
    const int flag = (int)sp[(size_t)W_FLAG * n_ops];
    uint32_t v = wave_load(sp, n_ops, c);  // a copy: the state in memory stays as it is
    if (c.active) {  // the pad is linear in the interleaved form too: 0x1F at byte `fill`, 0x80 on the block's last byte
        uint32_t plo = 0, phi = 0;
        if (c.word == (fill >> 3)) {
            const int sh = 8 * (fill & 7);
            plo = sh < 32 ? 0x1Fu << sh : 0u;
            phi = sh < 32 ? 0u : 0x1Fu << (sh - 32);
        }
        if (c.word == RATE_W - 1) phi ^= 0x80000000u;
        v ^= mldsa::coop2_from_lohi(plo, phi, c);
    }
    mldsa::keccak_f1600_coop2(v, c);
    uint32_t lo, hi;
    mldsa::coop2_to_lohi(v, lane, lo, hi);
    if (lane < 32 && c.active && c.word < 8) {  // lanes 0 ... 7: bytes 8 word ... 8 word + 7 of mu
        u32_any* out = reinterpret_cast<u32_any*>(mu + op * 64 + 8 * c.word);
        out[0] = flag == 0 ? lo : 0u;
        out[1] = flag == 0 ? hi : 0u;
    }
    if (lane == 63 && mu_flag) mu_flag[op] = flag;
}

// ------------------------------------------------------------------------------------------------------------ host side
bool wave_form(size_t n) { return n <= (size_t)MLDSA_MUS_WAVE_MAX_OPS; }

size_t state_bytes_of(size_t n_ops) { return n_ops > MLDSA_MUS_MAX_OPS ? 0 : 4 * (size_t)ST_WORDS * n_ops; }

int launch_init(const char* fn, int mode, const uint8_t* tr, size_t n_keys, const uint32_t* key_idx, const uint8_t* ctxs,
                const uint64_t* ctx_off, uint32_t* state, size_t n_ops, hipStream_t s) {
    if (wave_form(n_ops))
        hipLaunchKernelGGL(k_mus_init_wave, dim3((unsigned)n_ops), dim3(64), 0, s, tr, (uint32_t)n_keys, key_idx, mode, ctxs, ctx_off, state, n_ops);
    else
        hipLaunchKernelGGL(k_mus_init_lane, dim3((unsigned)((n_ops + 63) / 64)), dim3(64), 0, s, tr, (uint32_t)n_keys, key_idx, mode, ctxs,
                           ctx_off, state, n_ops);
    LAYER_LAUNCHED("k_mus_init launch");
    return MLDSA_OK;
}

// ops [first, first + count) of the n_ops states, the window [win_lo, win_hi) of offsets, `sub` = the offset of pieces[0]
int launch_update(const char* fn, uint32_t* state, const uint8_t* pieces, const uint64_t* off, size_t n_ops, size_t first, size_t count,
                  uint64_t win_lo, uint64_t win_hi, uint64_t sub, hipStream_t s) {
    if (count == 0) return MLDSA_OK;
    if (wave_form(count))
        hipLaunchKernelGGL(k_mus_update_wave, dim3((unsigned)count), dim3(64), 0, s, state, pieces, off, n_ops, first, win_lo, win_hi, sub);
    else
        hipLaunchKernelGGL(k_mus_update_lane, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, state, pieces, off, n_ops, first, count,
                           win_lo, win_hi, sub);
    LAYER_LAUNCHED("k_mus_update launch");
    return MLDSA_OK;
}

int launch_final(const char* fn, const uint32_t* state, uint8_t* mu, int32_t* mu_flag, size_t n_ops, hipStream_t s) {
    if (wave_form(n_ops))
        hipLaunchKernelGGL(k_mus_final_wave, dim3((unsigned)n_ops), dim3(64), 0, s, state, mu, mu_flag, n_ops);
    else
        hipLaunchKernelGGL(k_mus_final_lane, dim3((unsigned)((n_ops + 63) / 64)), dim3(64), 0, s, state, mu, mu_flag, n_ops);
    LAYER_LAUNCHED("k_mus_final launch");
    return MLDSA_OK;
}

bool known_mode(int mode) { return mode == MLDSA_MODE_PURE || mode == MLDSA_MODE_INTERNAL || mode == MLDSA_MODE_PREHASH; }

// the checks the three calls share, behind the empty call's return
int check_state(const char* fn, const mldsa_ctx* ctx, const void* state, size_t state_bytes, size_t n_ops) {
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if (n_ops > MLDSA_MUS_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_MUS_MAX_OPS ops");
    if (!state) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(state, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": state is not 8-byte aligned");
    if (state_bytes < state_bytes_of(n_ops)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": state_bytes is below mldsa_mus_state_bytes(n_ops)");
    return MLDSA_OK;
}

// ---------------------------------------------------------------------------------------------------------- host-memory call
void release_batch(mldsa_mus_host* h) {
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->d_coff) (void)hipFree(h->d_coff);
    if (h->d_ctxs) (void)hipFree(h->d_ctxs);
    if (h->d_state) (void)hipFree(h->d_state);
    h->d_off = h->d_coff = nullptr, h->d_ctxs = nullptr, h->d_state = nullptr;
    h->cap_ops = 0;
}

int reserve(const char* fn, mldsa_mus_host* h, size_t n_ops) {
    if (n_ops <= h->cap_ops) return MLDSA_OK;
    release_batch(h);
    if (hipMalloc((void**)&h->d_off, 8 * (n_ops + 1)) != hipSuccess || hipMalloc((void**)&h->d_coff, 8 * (n_ops + 1)) != hipSuccess ||
        hipMalloc((void**)&h->d_ctxs, n_ops * MAX_CTX_KEPT) != hipSuccess || hipMalloc((void**)&h->d_state, state_bytes_of(n_ops)) != hipSuccess) {
        (void)hipGetLastError();
        release_batch(h);
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": allocation of the per-batch buffers failed");
    }
    h->cap_ops = n_ops;
    return MLDSA_OK;
}

#define MUS_HIP(call, what)                                     \
    do {                                                        \
        const hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_failed(fn, what, e_);  \
    } while (0)

int stream_mu(const char* fn, mldsa_mus_host* h, int mode, const uint8_t* tr, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
              const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, uint8_t* mu, int32_t* mu_flag, size_t n_ops) {
    int rc = reserve(fn, h, n_ops);
    if (rc != MLDSA_OK) return rc;
    const hipStream_t s = h->feed.compute;
    MUS_HIP(hipMemcpyAsync(h->d_off, msg_off, 8 * (n_ops + 1), hipMemcpyHostToDevice, s), "upload of msg_off");
    if (ctx_off) {  // the ctxs packed anew, at most MAX_CTX_KEPT bytes of each: what the device holds of them is bounded by n_ops
        h->h_coff.resize(n_ops + 1);
        h->h_ctxs.clear();
        for (size_t i = 0; i < n_ops; i++) {
            const uint64_t len = ctx_off[i + 1] - ctx_off[i];
            const size_t keep = len < (uint64_t)MAX_CTX_KEPT ? (size_t)len : (size_t)MAX_CTX_KEPT;
            h->h_coff[i] = h->h_ctxs.size();
            if (keep) h->h_ctxs.insert(h->h_ctxs.end(), ctxs + ctx_off[i], ctxs + ctx_off[i] + keep);
        }
        h->h_coff[n_ops] = h->h_ctxs.size();
        MUS_HIP(hipMemcpyAsync(h->d_coff, h->h_coff.data(), 8 * (n_ops + 1), hipMemcpyHostToDevice, s), "upload of ctx_off");
        if (!h->h_ctxs.empty())
            MUS_HIP(hipMemcpyAsync(h->d_ctxs, h->h_ctxs.data(), h->h_ctxs.size(), hipMemcpyHostToDevice, s), "upload of ctxs");
    }
    rc = launch_init(fn, mode, tr, n_keys, key_idx, ctx_off ? h->d_ctxs : nullptr, ctx_off ? h->d_coff : nullptr, h->d_state, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    const FeedEnd end = h->feed.run(msgs, msg_off, n_ops, [&](const Chunk& c, const uint8_t* d_chunk) {
        return launch_update(fn, h->d_state, d_chunk, h->d_off, n_ops, c.first, c.last - c.first, c.lo, c.hi, c.lo, s);
    });
    if (end.hip != hipSuccess) return hip_failed(fn, end.step, end.hip);
    if (end.rc != MLDSA_OK) return end.rc;
    rc = launch_final(fn, h->d_state, mu, mu_flag, n_ops, s);
    if (rc != MLDSA_OK) return rc;
    MUS_HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_mus_abi_version(void) { return MLDSA_MUS_ABI_VERSION; }

const char* mldsa_mus_last_error(void) { return g_err.c_str(); }

size_t mldsa_mus_state_bytes(size_t n_ops) { return state_bytes_of(n_ops); }

int mldsa_mus_init(mldsa_ctx* ctx, int mode, const uint8_t* tr, size_t n_keys, const uint32_t* key_idx, const uint8_t* ctxs,
                   const uint64_t* ctx_off, void* state, size_t state_bytes, size_t n_ops, void* stream) {
    const char* fn = "mldsa_mus_init";
    if (!known_mode(mode)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (n_ops == 0) return MLDSA_OK;
    const int rc = check_state(fn, ctx, state, state_bytes, n_ops);
    if (rc != MLDSA_OK) return rc;
    if (!tr) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (n_keys == 0 || n_keys > 0xFFFFFFFFu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0 or does not fit 32 bits");
    LAYER_ON_DEVICE(ctx);
    return launch_init(fn, mode, tr, n_keys, key_idx, ctxs, ctx_off, static_cast<uint32_t*>(state), n_ops, (hipStream_t)stream);
}

int mldsa_mus_update(mldsa_ctx* ctx, void* state, size_t state_bytes, const uint8_t* pieces, const uint64_t* piece_off, size_t n_ops,
                     void* stream) {
    const char* fn = "mldsa_mus_update";
    if (n_ops == 0) return MLDSA_OK;
    const int rc = check_state(fn, ctx, state, state_bytes, n_ops);
    if (rc != MLDSA_OK) return rc;
    if (!piece_off) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    LAYER_ON_DEVICE(ctx);
    return launch_update(fn, static_cast<uint32_t*>(state), pieces, piece_off, n_ops, 0, n_ops, 0, ~(uint64_t)0, 0, (hipStream_t)stream);
}

int mldsa_mus_final(mldsa_ctx* ctx, const void* state, size_t state_bytes, uint8_t* mu, int32_t* mu_flag, size_t n_ops, void* stream) {
    const char* fn = "mldsa_mus_final";
    if (n_ops == 0) return MLDSA_OK;
    const int rc = check_state(fn, ctx, state, state_bytes, n_ops);
    if (rc != MLDSA_OK) return rc;
    if (!mu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    LAYER_ON_DEVICE(ctx);
    return launch_final(fn, static_cast<const uint32_t*>(state), mu, mu_flag, n_ops, (hipStream_t)stream);
}

int mldsa_mus_host_create(mldsa_ctx* ctx, size_t staging_bytes, mldsa_mus_host** out) {
    const char* fn = "mldsa_mus_host_create";
    if (out) *out = nullptr;
    if (!ctx || !out) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    LAYER_ON_DEVICE(ctx);
    mldsa_mus_host* h = new mldsa_mus_host;
    if (!h->feed.create(dev_, staging_bytes)) {
        delete h;
        return fail(MLDSA_ERR_NOMEM, std::string(fn) + ": streams, events or staging memory could not be allocated");
    }
    *out = h;
    return MLDSA_OK;
}

void mldsa_mus_host_destroy(mldsa_mus_host* h) {
    if (!h) return;
    const int dev = h->feed.dev;
    h->feed.destroy();  // waits for both streams
    {
        DeviceScope ds(dev);
        release_batch(h);
    }
    delete h;
}

int mldsa_mus_host_compute(mldsa_mus_host* h, int mode, const uint8_t* tr, size_t n_keys, const uint32_t* key_idx, const uint8_t* msgs,
                           const uint64_t* msg_off, const uint8_t* ctxs, const uint64_t* ctx_off, uint8_t* mu, int32_t* mu_flag,
                           size_t n_ops) {
    const char* fn = "mldsa_mus_host_compute";
    if (!known_mode(mode)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown mode");
    if (n_ops == 0) return MLDSA_OK;
    if (!h) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL mldsa_mus_host");
    if (n_ops > MLDSA_MUS_MAX_OPS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_MUS_MAX_OPS ops");
    if (!tr || !msg_off || !mu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (n_keys == 0 || n_keys > 0xFFFFFFFFu) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": n_keys is 0 or does not fit 32 bits");
    // both tables before a byte is read: the chunk plan and the packing of the ctxs walk them on the host
    LAYER_CORE(mldsa_check_offsets(msg_off, n_ops), "mldsa_check_offsets(msg_off)");
    if (ctx_off) LAYER_CORE(mldsa_check_offsets(ctx_off, n_ops), "mldsa_check_offsets(ctx_off)");
    if (!msgs && msg_off[n_ops] != msg_off[0]) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": msg_off names bytes of a NULL msgs");
    if (ctx_off && !ctxs && ctx_off[n_ops] != ctx_off[0]) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": ctx_off names bytes of a NULL ctxs");
    std::lock_guard<std::mutex> guard(h->lock);
    DeviceScope ds(h->feed.dev);
    if (!ds.ok) return fail(MLDSA_ERR_DEVICE, std::string(fn) + ": hipSetDevice failed");
    const int rc = stream_mu(fn, h, mode, tr, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, mu, mu_flag, n_ops);
    if (rc != MLDSA_OK) h->feed.drain();  // nothing of a failed call stays in flight
    return rc;
}

}  // extern "C"
