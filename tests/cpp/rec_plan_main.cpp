// The copy plan and the range check of libmldsa_rec.so (fips204_amd/rec/rec_plan.h) on their own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_records_cpu.py.  Exhaustive over source and destination residues
// 0 ... 15, the blob's own misalignment, the lengths 0 ... 70 and the key and signature lengths +- 1, with the field in the middle of the
// blob, flush against offset 0 and flush against blob_len.  For every case: each planned 16-byte load lies inside the blob's window and is
// 16-byte aligned, head and tail are at most 31 bytes, and replaying the plan as k_pack does -- on a heap block of exactly blob_len bytes,
// so that the sanitizer sees any byte read outside it -- reproduces the field.  Then the range check: wrap-around, off = blob_len, and
// the descriptor rules.  Exit status 0 and "rec_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fips204_amd/rec/rec_plan.h"

using namespace mldsa_rec;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

// Replays the plan as the kernel does.  `blob` holds blob_len bytes; frame position x is blob[x - mis].  An aligned 16-byte load at frame
// position `at` is checked against the window and then read with memcpy from the heap block.
static void replay(const uint8_t* blob, uint64_t blob_len, uint32_t mis, uint64_t off, uint64_t len, uint8_t* dst_row, uint32_t dst_res) {
    const uint64_t lo = mis, hi = mis + blob_len, src = mis + off;
    const CopyPlan p = copy_plan(src, len, dst_res, lo, hi);
    g_cases++;
    CHECK(p.head <= 31 && p.tail <= 31 && p.shift <= 15);
    CHECK(p.head + 16 * p.body + p.tail == len);
    CHECK(p.shift == ((src - dst_res) & 15));
    CHECK(p.body == 0 || ((dst_res + p.head) & 15) == 0);  // the body's stores are aligned
    CHECK(len < 64 || p.body >= len / 16 - 3);             // the body carries all but the ends
    for (uint32_t b = 0; b < p.head; b++) dst_row[b] = blob[off + b];
    for (uint64_t c = 0; c < p.body; c++) {
        const uint64_t at = chunk_src(p, src, c);
        const int loads = p.shift ? 2 : 1;
        CHECK((at & 15) == 0 && at >= lo && at + 16 * loads <= hi);
        if (!((at & 15) == 0 && at >= lo && at + 16 * loads <= hi)) return;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[4];
        std::memcpy(w, blob + (at - mis), 16 * loads);
        funnel16(w, p.shift, o);
        std::memcpy(dst_row + p.head + 16 * c, o, 16);
    }
    const uint64_t done = p.head + 16 * p.body;
    for (uint32_t b = 0; b < p.tail; b++) dst_row[done + b] = blob[off + done + b];
}

static void one_case(uint64_t blob_len, uint32_t mis, uint64_t off, uint64_t len, uint32_t dst_res) {
    // exactly blob_len bytes from the heap: a byte read before or behind them is the sanitizer's to report
    uint8_t* blob = static_cast<uint8_t*>(std::malloc(blob_len ? blob_len : 1));
    for (uint64_t i = 0; i < blob_len; i++) blob[i] = (uint8_t)(i * 131 + (i >> 8) * 17 + 7);
    std::vector<uint8_t> dst(len + 2, 0xEE);
    CHECK(in_range(off, len, blob_len));
    replay(blob, blob_len, mis, off, len, dst.data() + 1, dst_res);
    CHECK(dst[0] == 0xEE && dst[len + 1] == 0xEE);
    CHECK(len == 0 || std::memcmp(dst.data() + 1, blob + off, len) == 0);
    std::free(blob);
}

static void sweep_lengths(const std::vector<uint64_t>& lens, const std::vector<uint32_t>& mises) {
    for (uint64_t len : lens)
        for (uint32_t mis : mises)
            for (uint32_t src_res = 0; src_res < 16; src_res++)
                for (uint32_t dst_res = 0; dst_res < 16; dst_res++) {
                    // the field's frame residue is src_res: its blob offset is that minus the blob's misalignment, mod 16
                    const uint64_t off_mid = 48 + ((src_res + 16 - mis) & 15);
                    one_case(off_mid + len + 40, mis, off_mid, len, dst_res);  // in the middle
                    one_case(off_mid + len, mis, off_mid, len, dst_res);       // flush against blob_len
                    const uint64_t off_low = (src_res + 16 - mis) & 15;
                    one_case(off_low + len, mis, off_low, len, dst_res);       // within 15 bytes of offset 0 and flush against blob_len
                    if (src_res == 0) {
                        one_case(len + 33, mis, 0, len, dst_res);  // flush against offset 0
                        one_case(len, mis, 0, len, dst_res);       // the field is the blob
                    }
                }
}

static void range_checks() {
    const uint64_t top = ~(uint64_t)0;
    CHECK(!in_range(top, 2, 1000));            // off + len wraps to 1
    CHECK(!in_range(top - 5, 10, top));        // wraps with a huge blob_len too
    CHECK(!in_range(1000, 1, 1000));           // off = blob_len, len > 0
    CHECK(in_range(1000, 0, 1000));            // the empty range at the end
    CHECK(!in_range(1001, 0, 1000));
    CHECK(in_range(0, 1000, 1000) && !in_range(0, 1001, 1000) && !in_range(1, 1000, 1000));
    CHECK(in_range(0, 0, 0) && !in_range(0, 1, 0));
    CHECK(!in_range(5, top, 1000) && !in_range(top, top, top - 1));
    const uint64_t L = 20000;
    CHECK(classify(0, 3000, 8000, 9000, 10, 3, 44, 0, L) == CLASS_44);
    CHECK(classify(0, 3000, 8000, 9000, 10, 3, 65, 0, L) == CLASS_65);
    CHECK(classify(0, 3000, 8000, 9000, 10, 3, 87, 0, L) == CLASS_87);
    for (uint32_t set : {0u, 43u, 45u, 66u, 86u, 255u}) CHECK(classify(0, 3000, 8000, 9000, 10, 3, set, 0, L) == CLASS_REFUSED);
    CHECK(classify(0, 3000, 8000, 9000, 10, 3, 65, 1, L) == CLASS_REFUSED);
    CHECK(classify(0, 3000, 8000, 9000, 10, 255, 65, 0, L) == CLASS_65 && classify(0, 3000, 8000, 9000, 10, 256, 65, 0, L) == CLASS_REFUSED);
    CHECK(classify(L - 1952, 0, 0, 0, 0, 0, 65, 0, L) == CLASS_65 && classify(L - 1951, 0, 0, 0, 0, 0, 65, 0, L) == CLASS_REFUSED);
    CHECK(classify(0, L - 3309, 0, 0, 0, 0, 65, 0, L) == CLASS_65 && classify(0, L - 3308, 0, 0, 0, 0, 65, 0, L) == CLASS_REFUSED);
    CHECK(classify(0, top, 0, 0, 0, 0, 65, 0, L) == CLASS_REFUSED);
    CHECK(classify(0, 0, top - 3, 0, 8, 0, 65, 0, L) == CLASS_REFUSED && classify(0, 0, 0, top, 0, 1, 65, 0, L) == CLASS_REFUSED);
    CHECK(classify(0, 0, L, L, 0, 0, 65, 0, L) == CLASS_65 && classify(0, 0, L + 1, 0, 0, 0, 65, 0, L) == CLASS_REFUSED);
    CHECK(pk_len(CLASS_44) == 1312 && pk_len(CLASS_65) == 1952 && pk_len(CLASS_87) == 2592);
    CHECK(sig_len(CLASS_44) == 2420 && sig_len(CLASS_65) == 3309 && sig_len(CLASS_87) == 4627);
    CHECK(set_of_class(CLASS_44) == 44 && set_of_class(CLASS_65) == 65 && set_of_class(CLASS_87) == 87);
}

int main() {
    std::vector<uint64_t> small, fields = {1311, 1312, 1313, 2419, 2420, 2421, 3308, 3309, 3310, 4626, 4627, 4628, 1952, 2592};
    for (uint64_t len = 0; len <= 70; len++) small.push_back(len);
    sweep_lengths(small, {0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15});
    sweep_lengths(fields, {0, 3, 8, 13});
    range_checks();
    if (g_fail) {
        std::fprintf(stderr, "rec_plan: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("rec_plan OK (%ld copies)\n", g_cases);
    return 0;
}
