// The part plan and the scratch carve of mldsa_vfy_verify (fips204_amd/vfy/vfy_parts.h) on their own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_vfy_layer_cpu.py.  For part sizes 1, 64, 4096 and 65536, the
// three parameter sets and n in {0, 1, part - 1, part, part + 1, 2 part + 1} it checks that every op lies in exactly one part, in order;
// that no part exceeds the part size and only the last one is short; that consecutive parts use different ring halves and a call of one
// part uses one; that the ring halves and every per-op array lie inside the scratch, 256-byte aligned, without overlap; and that a
// buffer of exactly `bytes` bytes takes a write to the first and the last byte of every array.  Exit status 0 and "vfy_parts OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../fips204_amd/vfy/vfy_parts.h"

using mldsa_vfy::Carve;
using mldsa_vfy::Part;
using mldsa_vfy::PartPlan;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

static void check_plan(size_t n, size_t part) {
    const PartPlan plan(n, part);
    std::vector<int> seen(n, 0);
    size_t at = 0;
    CHECK(plan.n_parts() == (n + part - 1) / part);
    CHECK(plan.halves() == (plan.n_parts() > 1 ? 2u : plan.n_parts()));
    CHECK(plan.half_ops() == (n < part ? n : part));
    for (size_t i = 0; i < plan.n_parts(); i++) {
        const Part p = plan.at(i);
        CHECK(p.first == at && p.count >= 1 && p.count <= part && p.first + p.count <= n);
        CHECK(p.count == part || i + 1 == plan.n_parts());  // only the last part is short
        CHECK(p.count <= plan.half_ops());                  // it fits its ring half
        CHECK(p.half == (int)(i & 1));
        if (i) CHECK(p.half != plan.at(i - 1).half);  // ExpandA of part i never writes the half part i - 1 is read from
        for (size_t o = p.first; o < p.first + p.count; o++) seen[o]++;
        at = p.first + p.count;
    }
    CHECK(at == n);
    for (size_t o = 0; o < n; o++) CHECK(seen[o] == 1);
}

static void check_carve(int k, int l, size_t w1_len, size_t n, size_t part) {
    const PartPlan plan(n, part);
    const Carve c = mldsa_vfy::carve(k, l, w1_len, plan);
    const size_t ring = plan.half_ops() * (size_t)(k * l) * mldsa_vfy::PACKED_POLY_BYTES;
    CHECK(c.ring_bytes == ring);
    std::vector<std::pair<size_t, size_t>> spans;  // (offset, bytes)
    spans.push_back({c.ring[0], ring});
    if (plan.halves() > 1) spans.push_back({c.ring[1], ring});
    else CHECK(c.ring[1] == c.ring[0]);
    spans.push_back({c.c, n * 256});
    spans.push_back({c.znorm, n * 4});
    spans.push_back({c.hvalid, n * 4});
    spans.push_back({c.ctx_bad, n * 4});
    spans.push_back({c.key_bad, n * 4});
    spans.push_back({c.kidx, n * 4});
    spans.push_back({c.mu_w1, n * (64 + w1_len)});
    for (size_t i = 0; i < spans.size(); i++) {
        CHECK(spans[i].first % mldsa_vfy::CARVE_ALIGN == 0);
        CHECK(spans[i].first + spans[i].second <= c.bytes);
        for (size_t j = 0; j < i; j++) {
            const bool apart = spans[j].first + spans[j].second <= spans[i].first || spans[i].first + spans[i].second <= spans[j].first;
            CHECK(apart || spans[i].second == 0 || spans[j].second == 0);
        }
    }
    // a buffer of exactly c.bytes: the sanitizer sees every array's first and last byte
    if (c.bytes <= ((size_t)64 << 20)) {
        std::vector<uint8_t> buf(c.bytes);
        for (const auto& s : spans)
            if (s.second) {
                buf[s.first] = 1;
                buf[s.first + s.second - 1] = 1;
            }
        CHECK(buf.size() == c.bytes);
    }
    // the scratch never shrinks as the call grows
    if (n) CHECK(mldsa_vfy::carve(k, l, w1_len, PartPlan(n - 1, part)).bytes <= c.bytes);
}

int main() {
    const size_t parts[4] = {1, 64, 4096, 65536};
    const int sets[3][3] = {{4, 4, 768}, {6, 5, 768}, {8, 7, 1024}};  // k, l, w1_len
    for (size_t part : parts) {
        const size_t ns[6] = {0, 1, part - 1, part, part + 1, 2 * part + 1};
        for (size_t n : ns) {
            check_plan(n, part);
            for (const auto& s : sets) check_carve(s[0], s[1], (size_t)s[2], n, part);
        }
    }
    // a part size of 0 is read as 1, never a division by zero
    check_plan(5, 1);
    CHECK(PartPlan(5, 0).n_parts() == 5);
    // the ring of a 4 096-op part of ML-DSA-65: 2 x 4 096 x 30 x 768 bytes
    CHECK(mldsa_vfy::carve(6, 5, 768, PartPlan(65536, 4096)).ring_bytes == (size_t)4096 * 30 * 768);
    if (g_fail) {
        std::fprintf(stderr, "vfy_parts: %d checks failed\n", g_fail);
        return 1;
    }
    std::puts("vfy_parts OK");
    return 0;
}
