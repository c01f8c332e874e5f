// The descriptor check of libmldsa_recsign.so (fips204_amd/recsign/recsign_plan.h) and the copy plan in the scatter direction, on their
// own: pure host code, compiled with -fsanitize=address,undefined and run as a child process by tests/test_recsign_cpu.py.
// The scatter is replayed as k_scatter does it: the source window is a heap block of exactly n * SIG_LEN bytes (a class's dense sigs
// array, `mis` bytes past a 16-byte boundary), the destination a heap block of exactly out_len bytes, so that the sanitizer sees any byte
// read or written outside them.  For the three SIG_LEN, the slots 0, 1 and last, every destination residue 0 ... 15, and holes in the
// middle, at offset 0 and flush with out_len: every load lies inside the source window, every store inside the op's range, the
// destination equals the row and the bytes around it are unchanged.  Then the descriptor check: the wrap cases and the order of the
// refusal codes.  Exit status 0 and "recsign_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fips204_amd/recsign/recsign_plan.h"

using namespace mldsa_recsign;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

// Row `slot` of sigs[n][len] (frame position x is sigs[x - mis]) to out + sig_off, whose address mod 16 is dst_res.
static void replay(const uint8_t* sigs, uint64_t n, uint32_t len, uint32_t mis, uint64_t slot, uint8_t* out, uint64_t out_len, uint64_t sig_off,
                   uint32_t dst_res) {
    const uint64_t lo = mis, hi = mis + n * len, src = mis + slot * len;
    const CopyPlan p = copy_plan(src, len, dst_res, lo, hi);
    g_cases++;
    CHECK(p.head <= 31 && p.tail <= 31 && p.shift <= 15);
    CHECK(p.head + 16 * p.body + p.tail == len);
    CHECK(p.body == 0 || ((dst_res + p.head) & 15) == 0);  // the body's stores are aligned
    CHECK(p.body >= len / 16 - 3);                         // the body carries all but the ends
    uint8_t* dst = out + sig_off;
    for (uint32_t b = 0; b < p.head; b++) dst[b] = sigs[slot * len + b];
    for (uint64_t c = 0; c < p.body; c++) {
        const uint64_t at = chunk_src(p, src, c);
        const int loads = p.shift ? 2 : 1;
        const bool load_ok = (at & 15) == 0 && at >= lo && at + 16 * loads <= hi;
        const uint64_t to = p.head + 16 * c;  // the store [to, to + 16) of the op's range [0, len), inside [0, out_len) of the buffer
        const bool store_ok = to + 16 <= len && sig_off + to + 16 <= out_len;
        CHECK(load_ok && store_ok);
        if (!load_ok || !store_ok) return;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[4];
        std::memcpy(w, sigs + (at - mis), 16 * loads);
        funnel16(w, p.shift, o);
        std::memcpy(dst + to, o, 16);
    }
    const uint64_t done = p.head + 16 * p.body;
    for (uint32_t b = 0; b < p.tail; b++) dst[done + b] = sigs[slot * len + done + b];
}

static void one_case(uint64_t n, uint32_t len, uint32_t mis, uint64_t slot, uint64_t before, uint64_t behind, uint32_t dst_res) {
    // exactly n * len and out_len bytes from the heap: a byte touched before or behind them is the sanitizer's to report
    uint8_t* sigs = static_cast<uint8_t*>(std::malloc(n * len));
    for (uint64_t i = 0; i < n * len; i++) sigs[i] = (uint8_t)(i * 131 + (i >> 8) * 17 + 7);
    const uint64_t out_len = before + len + behind;
    uint8_t* out = static_cast<uint8_t*>(std::malloc(out_len));
    std::memset(out, 0xEE, out_len);
    CHECK(in_range(before, len, out_len) && slot < n);
    replay(sigs, n, len, mis, slot, out, out_len, before, dst_res);
    CHECK(std::memcmp(out + before, sigs + slot * len, len) == 0);
    for (uint64_t i = 0; i < before; i++) CHECK(out[i] == 0xEE);
    for (uint64_t i = before + len; i < out_len; i++) CHECK(out[i] == 0xEE);
    std::free(out);
    std::free(sigs);
}

static void scatter_cases() {
    for (int c = CLASS_44; c <= CLASS_87; c++)
        for (uint64_t n : {1u, 2u, 5u})
            for (uint64_t slot : {(uint64_t)0, (uint64_t)1, n - 1}) {
                if (slot >= n) continue;
                for (uint32_t mis : {0u, 3u, 8u, 13u})  // the arena keeps sigs 256-byte aligned (mis = 0); a caller's own array need not be
                    for (uint32_t dst_res = 0; dst_res < 16; dst_res++) {
                        one_case(n, sig_len(c), mis, slot, 37, 41, dst_res);  // in the middle
                        one_case(n, sig_len(c), mis, slot, 0, 41, dst_res);   // the hole at offset 0
                        one_case(n, sig_len(c), mis, slot, 37, 0, dst_res);   // flush with out_len
                        one_case(n, sig_len(c), mis, slot, 0, 0, dst_res);    // the hole is the buffer
                    }
            }
}

static Verdict ck(uint64_t msg_off, uint64_t ctx_off, uint64_t rnd_off, uint64_t sig_off, uint32_t msg_len, uint32_t key, uint32_t ctx_len,
                  uint32_t set, uint32_t flags, uint32_t reserved) {
    return check_op(msg_off, ctx_off, rnd_off, sig_off, msg_len, key, ctx_len, set, flags, reserved, /*blob_len*/ 20000, /*out_len*/ 30000,
                    /*n_keys*/ 4, 0, 7);
}

static void descriptor_checks() {
    const uint64_t top = ~(uint64_t)0, B = 20000, O = 30000;
    Verdict v = ck(100, 200, 300, 400, 10, 3, 5, 44, FLAG_RND, 0);
    CHECK(v.cls == CLASS_44 && v.status == ST_OK);
    v = ck(100, 200, 300, 400, 10, 6, 5, 87, 0, 0);
    CHECK(v.cls == CLASS_87 && v.status == ST_OK);
    // 1. set, flags, reserved
    for (uint32_t set : {0u, 43u, 45u, 66u, 86u, 255u}) CHECK(ck(100, 200, 300, 400, 10, 0, 5, set, 0, 0).cls == CLASS_REFUSED);
    for (uint32_t flags : {2u, 3u, 4u, 0x80u, 0xFFu}) {
        v = ck(100, 200, 300, 400, 10, 0, 5, 44, flags, 0);
        CHECK(v.cls == CLASS_REFUSED && v.status == ST_PARAM);
    }
    v = ck(100, 200, 300, 400, 10, 0, 5, 44, 0, 1);
    CHECK(v.cls == CLASS_REFUSED && v.status == ST_PARAM);
    CHECK(ck(100, 200, 300, 400, 10, 0, 5, 44, 0, 0x80000000u).cls == CLASS_REFUSED);
    // 2. the context's length: the core's code, and before the later rules
    CHECK(ck(100, 200, 300, 400, 10, 0, 255, 44, 0, 0).status == ST_OK);
    v = ck(100, 200, 300, 400, 10, 0, 256, 44, 0, 0);
    CHECK(v.cls == CLASS_REFUSED && v.status == ST_CTX_LEN);
    CHECK(ck(top, top, top, top, 10, 99, 256, 44, FLAG_RND, 0).status == ST_CTX_LEN);  // rules 3, 4, 5 broken too
    CHECK(ck(100, 200, 300, 400, 10, 0, 256, 43, 0, 0).status == ST_PARAM);            // rule 1 first
    CHECK(ck(100, 200, 300, 400, 10, 0, 256, 44, 2, 0).status == ST_PARAM);
    CHECK(ck(100, 200, 300, 400, 10, 0, 0xFFFF, 44, 0, 7).status == ST_PARAM);
    // 3. the key's row; a set with no keys is not served
    CHECK(ck(100, 200, 300, 400, 10, 3, 5, 44, 0, 0).status == ST_OK && ck(100, 200, 300, 400, 10, 4, 5, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, 300, 400, 10, 0, 5, 65, 0, 0).cls == CLASS_REFUSED && ck(100, 200, 300, 400, 10, 0xFFFFFFFFu, 5, 87, 0, 0).cls == CLASS_REFUSED);
    // 4. the ranges in the blob; rnd_off only with the flag
    CHECK(ck(B - 10, 200, 300, 400, 10, 0, 5, 44, 0, 0).status == ST_OK && ck(B - 9, 200, 300, 400, 10, 0, 5, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(B, B, 300, 400, 0, 0, 0, 44, 0, 0).status == ST_OK && ck(B + 1, 0, 300, 400, 0, 0, 0, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(top - 7, 200, 300, 400, 64, 0, 5, 44, 0, 0).cls == CLASS_REFUSED);  // off + len wraps to 56
    CHECK(ck(100, top, 300, 400, 10, 0, 1, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, B - 32, 400, 10, 0, 5, 44, FLAG_RND, 0).status == ST_OK);
    CHECK(ck(100, 200, B - 31, 400, 10, 0, 5, 44, FLAG_RND, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, top - 3, 400, 10, 0, 5, 44, FLAG_RND, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, top - 3, 400, 10, 0, 5, 44, 0, 0).status == ST_OK);  // not followed, not checked
    // 5. the hole in out: its own length
    CHECK(ck(100, 200, 300, O - 2420, 10, 0, 5, 44, 0, 0).status == ST_OK && ck(100, 200, 300, O - 2419, 10, 0, 5, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, 300, O - 4627, 10, 0, 5, 87, 0, 0).status == ST_OK && ck(100, 200, 300, O - 4626, 10, 0, 5, 87, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, 300, top, 10, 0, 5, 44, 0, 0).cls == CLASS_REFUSED && ck(100, 200, 300, top - 2419, 10, 0, 5, 44, 0, 0).cls == CLASS_REFUSED);
    CHECK(ck(100, 200, 300, B, 10, 0, 5, 44, 0, 0).status == ST_OK);  // beyond blob_len, inside out_len: the two lengths are apart
    CHECK(check_op(0, 0, 0, 0, 0, 0, 0, 65, 0, 0, 0, 3309, 0, 1, 0).status == ST_OK && check_op(0, 0, 0, 0, 0, 0, 0, 65, 0, 0, 0, 3308, 0, 1, 0).cls == CLASS_REFUSED);
    CHECK(sig_len(CLASS_44) == 2420 && sig_len(CLASS_65) == 3309 && sig_len(CLASS_87) == 4627);
}

int main() {
    scatter_cases();
    descriptor_checks();
    if (g_fail) {
        std::fprintf(stderr, "recsign_plan: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("recsign_plan OK (%ld copies)\n", g_cases);
    return 0;
}
