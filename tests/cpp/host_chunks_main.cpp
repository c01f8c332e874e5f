// The chunk plan of the host-memory feed (fips204_amd/layer/host_chunks.h) on its own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_mu_stream_cpu.py.  Over seeded offset tables and staging sizes
// 1, 7, 136, 4096 it checks that every byte of [off[0], off[n]) lies in exactly one chunk, in order; that no chunk exceeds `staging`;
// that the per-chunk piece offsets are monotone and start at 0; that the op range of a chunk is exactly the ops with bytes in it; that an
// empty message on a chunk boundary gets no launch; that a message of 5 staging + 3 bytes spans six chunks; that n_ops = 0 and all-empty
// batches give no chunk.  Exit status 0 and "mus_chunks OK" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fips204_amd/layer/host_chunks.h"

using mldsa_layer::Chunk;
using mldsa_layer::ChunkPlan;
using mldsa_layer::piece_off_in_chunk;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

// the chunks of a table, each checked against the table byte range by byte range; launches[op] = chunks in whose op range the op lies
static std::vector<Chunk> run_plan(const std::vector<uint64_t>& off, uint64_t staging, std::vector<int>* launches) {
    const size_t n = off.size() - 1;
    std::vector<Chunk> chunks;
    std::vector<uint64_t> absorbed(n, 0);  // bytes of each op the chunks have handed to it so far
    if (launches) launches->assign(n, 0);
    ChunkPlan plan(off.data(), n, staging);
    Chunk c;
    uint64_t at = off[0];
    while (plan.next(&c)) {
        CHECK(c.lo == at && c.hi > c.lo && c.hi - c.lo <= staging && c.hi <= off[n]);  // in order, gapless, never above staging
        CHECK(c.hi - c.lo == staging || c.hi == off[n]);                                // only the last chunk is short
        CHECK(c.first < c.last && c.last <= n);
        // the op range is exactly the ops with bytes in the chunk: its two ends have bytes, nothing outside it has
        for (size_t i = 0; i < n; i++) {
            const uint64_t a = off[i] > c.lo ? off[i] : c.lo, b = off[i + 1] < c.hi ? off[i + 1] : c.hi;
            const bool has = b > a;
            if (has) CHECK(i >= c.first && i < c.last);
            if (i == c.first || i + 1 == c.last) CHECK(has);
            if (i >= c.first && i < c.last) {
                if (launches) (*launches)[i]++;
                const uint64_t r0 = piece_off_in_chunk(off.data(), i, c), r1 = piece_off_in_chunk(off.data(), i + 1, c);
                CHECK(r0 <= r1 && r1 <= c.hi - c.lo);  // monotone, inside the chunk
                CHECK(r1 - r0 == (has ? b - a : 0));
                if (has) CHECK(c.lo + r0 == off[i] + absorbed[i]);  // the op's bytes arrive in order, none twice, none skipped
                absorbed[i] += r1 - r0;
            }
        }
        CHECK(piece_off_in_chunk(off.data(), c.first, c) == 0);              // the pieces start at byte 0 of the chunk
        CHECK(piece_off_in_chunk(off.data(), c.last, c) == c.hi - c.lo);     // ... and fill it
        at = c.hi;
        chunks.push_back(c);
    }
    CHECK(at == off[n]);
    for (size_t i = 0; i < n; i++) CHECK(absorbed[i] == off[i + 1] - off[i]);
    return chunks;
}

int main() {
    const uint64_t stagings[4] = {1, 7, 136, 4096};
    // seeded tables: a mix of empty, short and long messages, a non-zero first offset
    for (int t = 0; t < 200; t++) {
        const size_t n = 1 + (size_t)(rnd() % 40);
        std::vector<uint64_t> off(n + 1);
        off[0] = rnd() % 3 ? 0 : rnd() % 1000;
        for (size_t i = 0; i < n; i++) {
            const uint64_t kind = rnd() % 8;
            const uint64_t len = kind < 2 ? 0 : kind < 5 ? rnd() % 20 : kind < 7 ? rnd() % 600 : rnd() % 20000;
            off[i + 1] = off[i] + len;
        }
        for (uint64_t staging : stagings) {
            if (staging == 1 && off[n] - off[0] > 3000) continue;  // one chunk per byte: keep the quadratic check small
            std::vector<int> launches;
            run_plan(off, staging, &launches);
            for (size_t i = 0; i < n; i++)
                if (off[i] == off[i + 1] && (off[i] - off[0]) % staging == 0) CHECK(launches[i] == 0);  // an empty message on a boundary
        }
    }
    for (uint64_t staging : stagings) {
        // an empty message exactly on a chunk boundary gets no launch: ops 1 and 3 here
        std::vector<uint64_t> off = {0, staging, staging, 2 * staging, 2 * staging, 2 * staging + 1};
        std::vector<int> launches;
        const std::vector<Chunk> ch = run_plan(off, staging, &launches);
        CHECK(ch.size() == 3 && launches[0] == 1 && launches[1] == 0 && launches[2] == 1 && launches[3] == 0 && launches[4] == 1);
        // a message of 5 staging + 3 bytes spans six chunks (eight of one byte each with staging = 1: 5 + ceil(3 / staging))
        off = {10, 10 + 5 * staging + 3};
        const size_t spans = staging == 1 ? 8 : 6;
        CHECK(run_plan(off, staging, &launches).size() == spans && launches[0] == (int)spans);
        // ... also behind a short one that shifts it off the boundaries
        off = {0, 2, 2 + 5 * staging + 3, 2 + 5 * staging + 4};
        CHECK(run_plan(off, staging, &launches).size() == (staging == 1 ? 11u : 6u) && launches[1] == (staging == 1 ? 8 : 6));
        // all-empty batches and n_ops = 0: no chunk
        off = {5, 5, 5, 5};
        CHECK(run_plan(off, staging, &launches).empty());
        const uint64_t none[1] = {0};
        ChunkPlan empty(none, 0, staging);
        Chunk c;
        CHECK(!empty.next(&c));
        ChunkPlan null_table(nullptr, 0, staging);
        CHECK(!null_table.next(&c));
    }
    if (g_fail) {
        std::fprintf(stderr, "mus_chunks: %d checks failed\n", g_fail);
        return 1;
    }
    std::puts("mus_chunks OK");
    return 0;
}
