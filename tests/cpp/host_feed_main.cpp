// The host-memory feed of the layers (fips204_amd/layer/host_feed.h) on the CPU: compiled host-only with -fsanitize=address,undefined,
// linked against the stand-in HIP runtime of tests/cpp/stub_hip_full.cpp ("device" memory is heap memory of exactly the requested size,
// copies are memcpy, streams and events are tags) and run as a child process by tests/test_layer_common_cpu.py.
// HostFeed::run is driven with an update that copies each op's piece of the chunk out of the "device" chunk.  Over a pageable and a
// page-locked source, staging sizes 1, 7, 64, 4096, one fixed offset table and 200 seeded ones it checks that every message is
// reassembled byte for byte, that no chunk exceeds `staging`, that the op range of every chunk is the one a brute-force scan finds, that
// a page-locked source never touches the bounce chunks, that an update failing at the first, a middle and the last chunk ends the run
// with its rc and leaves the feed fit for the next run, and that create / destroy and a create that runs out of memory leave nothing
// allocated (the stand-in's count, and ASan's leak check at exit).  Exit status 0 and "host_feed OK" on success.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fips204_amd/layer/host_feed.h"

extern "C" size_t stub_live_allocations(void);
extern "C" void stub_set_mem_limit(size_t bytes);

using mldsa_layer::Chunk;
using mldsa_layer::FeedEnd;
using mldsa_layer::HostFeed;
using mldsa_layer::piece_hi;
using mldsa_layer::piece_lo;

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

constexpr int RC_UPDATE = -77;  // what the failing update returns: no code of the library's

// One run over msgs / off.  fail_at < 0: the run must succeed and reassemble every message.  Otherwise the update of chunk `fail_at`
// returns RC_UPDATE: the run must end there with that rc and no HIP error.  Returns the number of chunks the update saw.
static size_t run_once(HostFeed& feed, const uint8_t* msgs, const std::vector<uint64_t>& off, long fail_at) {
    const size_t n = off.size() - 1;
    std::vector<std::vector<uint8_t>> got(n);
    size_t chunks = 0;
    uint64_t at = off[0];
    const FeedEnd end = feed.run(msgs, off.data(), n, [&](const Chunk& c, const uint8_t* d_chunk) {
        CHECK(c.lo == at && c.hi > c.lo && c.hi - c.lo <= feed.staging && c.hi <= off[n]);  // in order, gapless, never above staging
        CHECK(d_chunk == feed.d_stage[chunks & 1]);                                         // the two chunks in turn
        at = c.hi;
        // the op range against a brute-force scan: the first and the last op that have bytes in [c.lo, c.hi)
        size_t first = n, last = 0;
        for (size_t i = 0; i < n; i++)
            if (piece_hi(off[i + 1], c.hi) > piece_lo(off[i], c.lo)) {
                if (first == n) first = i;
                last = i + 1;
            }
        CHECK(c.first == first && c.last == last);
        for (size_t i = c.first; i < c.last && i < n; i++) {
            const uint64_t a = piece_lo(off[i], c.lo), b = piece_hi(off[i + 1], c.hi);
            if (b > a) got[i].insert(got[i].end(), d_chunk + (a - c.lo), d_chunk + (b - c.lo));
        }
        return (long)chunks++ == fail_at ? RC_UPDATE : MLDSA_OK;
    });
    CHECK(end.hip == hipSuccess);
    if (fail_at < 0) {
        CHECK(end.rc == MLDSA_OK && at == off[n]);
        for (size_t i = 0; i < n; i++) {
            const size_t len = (size_t)(off[i + 1] - off[i]);
            CHECK(got[i].size() == len && (len == 0 || std::memcmp(got[i].data(), msgs + off[i], len) == 0));
        }
    } else {
        CHECK(end.rc == RC_UPDATE && chunks == (size_t)fail_at + 1);
        feed.drain();  // what the layers do after a failed call
    }
    return chunks;
}

// the table from a pageable and from a page-locked source; with `failures`, an update that fails at chunk 0, a middle and the last one
static void run_table(HostFeed& feed, const std::vector<uint64_t>& off, bool failures) {
    const size_t total = (size_t)off.back();
    std::vector<uint8_t> pageable(total);  // exactly the bytes the table names: a read past them is ASan's
    for (size_t i = 0; i < total; i++) pageable[i] = (uint8_t)(rnd() >> 32);
    uint8_t* locked = nullptr;
    CHECK(hipHostMalloc((void**)&locked, total, hipHostMallocDefault) == hipSuccess);
    if (total) std::memcpy(locked, pageable.data(), total);
    const uint8_t* sources[2] = {pageable.data(), locked};
    for (int s = 0; s < 2; s++) {
        for (int b = 0; b < 2; b++) std::memset(feed.h_stage[b], 0xEE, feed.staging);
        const size_t chunks = run_once(feed, sources[s], off, -1);
        CHECK(chunks == (total - (size_t)off[0] + feed.staging - 1) / feed.staging);
        if (s == 1)  // a page-locked source is copied where it lies
            for (int b = 0; b < 2; b++)
                for (size_t i = 0; i < feed.staging; i++) CHECK(feed.h_stage[b][i] == 0xEE);
        if (failures && chunks) {
            const long at[3] = {0, (long)(chunks / 2), (long)chunks - 1};
            for (long f : at) {
                run_once(feed, sources[s], off, f);
                CHECK(run_once(feed, sources[s], off, -1) == chunks);  // the same feed, the whole batch again
            }
        }
    }
    CHECK(hipHostFree(locked) == hipSuccess);
}

int main() {
    const size_t stagings[4] = {1, 7, 64, 4096};
    const size_t idle = stub_live_allocations();
    for (size_t staging : stagings) {
        HostFeed feed;
        CHECK(feed.create(0, staging) && feed.staging == staging && feed.dev == 0);
        CHECK(stub_live_allocations() == idle + 4);
        // empty messages at the start, on a chunk end (at 64 with staging 64) and at the end; a one-byte message; one of many chunks
        run_table(feed, {0, 0, 64, 64, 64, 194, 195, 195}, true);
        run_table(feed, {5, 5, 5, 5}, true);  // all empty: no chunk, no update
        g_rng = 0x9E3779B97F4A7C15ull + staging;
        for (int t = 0; t < 200; t++) {
            const size_t n = 1 + (size_t)(rnd() % 40);
            std::vector<uint64_t> off(n + 1);
            off[0] = rnd() % 3 ? 0 : rnd() % 1000;
            for (size_t i = 0; i < n; i++) {
                const uint64_t kind = rnd() % 8;
                const uint64_t len = kind < 2 ? 0 : kind < 5 ? rnd() % 20 : kind < 7 ? rnd() % 300 : rnd() % 3000;
                off[i + 1] = off[i] + len;
            }
            if (staging == 1 && off[n] - off[0] > 3000) continue;  // one chunk per byte: keep the quadratic scan small
            run_table(feed, off, staging == 64 && t < 40);
        }
        feed.destroy();
        CHECK(stub_live_allocations() == idle && feed.copy == nullptr && feed.d_stage[0] == nullptr && feed.h_stage[1] == nullptr);
    }
    {  // 0 selects the default; a create that runs out of "device" memory leaves nothing behind
        HostFeed feed;
        stub_set_mem_limit(mldsa_layer::DEFAULT_STAGING - 1);
        CHECK(!feed.create(0, 0) && stub_live_allocations() == idle && feed.compute == nullptr);
        stub_set_mem_limit((size_t)1 << 40);
        CHECK(feed.create(0, 0) && feed.staging == mldsa_layer::DEFAULT_STAGING);
        feed.destroy();
        CHECK(stub_live_allocations() == idle);
    }
    if (g_fail) {
        std::fprintf(stderr, "host_feed: %d checks failed\n", g_fail);
        return 1;
    }
    std::puts("host_feed OK");
    return 0;
}
