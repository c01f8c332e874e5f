// The Time reader, the policy walk and the climb of libmldsa_path.so (fips204_amd/path/path_plan.h) on their own: pure host code, compiled
// with -fsanitize=address,undefined and run as a child process by tests/test_path_cpu.py.  The test writes its cases as lines into the
// file PATH_CASES names:
//   T <hex>            one Time TLV and what follows it: parse_time on a heap block of exactly these bytes
//   W <flags> <hex>    one certificate: walk_policy on a heap block of EXACTLY the declared length, so that the sanitizer sees any byte
//                      read outside [off, off + len)
//   C <hex>            n packed nodes of 8 bytes: climb from every one of them
// For every case one row goes to the file PATH_ROWS names, which the test compares with the Python restatement of tests/path_cases.py.
// Every proper prefix of the first certificate must be malformed.  Then the edges that need no case: the calendar against a day
// count kept by stepping, the node's packing, the rules' order and the freshness rule.  Exit status 0 and "path_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fips204_amd/path/path_plan.h"

using namespace mldsa_path;
typedef std::vector<uint8_t> Bytes;

static int g_fail = 0;
static long g_runs = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

struct Heap {
    const uint8_t* p;
    uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

// a heap block of exactly the bytes, freed with the object
struct Block {
    uint8_t* p;
    Block(const uint8_t* src, size_t len) : p(static_cast<uint8_t*>(std::malloc(len ? len : 1))) {
        if (len) std::memcpy(p, src, len);
    }
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

static Bytes unhex(const std::string& s) {
    Bytes out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static Policy run_walk(const Bytes& b, size_t len, uint32_t flags) {
    const Block block(b.data(), len);
    g_runs++;
    return walk_policy(Heap{block.p}, (uint32_t)len, flags);
}

struct NodeWords {
    const uint64_t* p;
    uint64_t operator()(uint32_t a) const { return p[a]; }
};

static void calendar_edges() {
    // every day from 0001-01-01 to 9999-12-31 by stepping, against the closed form
    int64_t day = -719162;  // 0001-01-01
    for (uint32_t y = 1; y <= 9999; y++)
        for (uint32_t m = 1; m <= 12; m++) {
            const uint32_t dim = days_in_month(y, m);
            CHECK(dim == (m == 2 ? (leap_year(y) ? 29u : 28u) : (m == 4 || m == 6 || m == 9 || m == 11) ? 30u : 31u));
            CHECK(days_from_civil(y, m, 1) == day && days_from_civil(y, m, dim) == day + dim - 1);
            day += dim;
        }
    CHECK(days_from_civil(1970, 1, 1) == 0 && days_from_civil(2000, 3, 1) == 11017 && days_from_civil(2038, 1, 19) == 24855);
    CHECK(leap_year(2000) && leap_year(2400) && !leap_year(1900) && !leap_year(2100) && leap_year(2024) && !leap_year(2025));
    static_assert(days_from_civil(1970, 1, 2) == 1 && days_in_month(2024, 2) == 29, "the plan is constexpr");
}

static void rule_edges() {
    // the node's 8 bytes
    const Node nd = node_of(0x01020304u, V_EXPIRED, V_NOT_CA, 300, true);
    CHECK(pack_node(nd) == 0x01FE080501020304ull && unpack_node(pack_node(nd)).path_len == 254 && unpack_node(pack_node(nd)).anchor == 1);
    CHECK(node_of(7, 0, 0, NO_PATH_LEN, false).path_len == 255 && node_of(7, 0, 0, 254, false).path_len == 254 && node_of(7, 0, 0, 0, false).path_len == 0);
    // own_rule: the order of the header
    CHECK(own_rule(5, false, ST_DER, 10, 5, true, 1, 0, 0) == V_CERT && own_rule(0, false, ST_DER, 10, 5, true, 1, 0, 0) == V_SIG);
    CHECK(own_rule(0, true, ST_TIME, 10, 5, true, 1, 0, 0) == V_POLICY && own_rule(0, true, 0, 10, 5, true, 1, 7, 0) == V_NOT_YET);
    CHECK(own_rule(0, true, 0, 10, 20, true, 1, 21, 0) == V_EXPIRED && own_rule(0, true, 0, 10, 20, true, 1, 20, 0) == V_REVOKED);
    CHECK(own_rule(0, true, 0, 10, 20, true, 0, 10, 0) == 0 && own_rule(0, true, 0, 10, 20, false, 1, 15, 0) == 0);
    for (int rev = 2; rev < 9; rev++) CHECK(own_rule(0, true, 0, 10, 20, true, rev, 15, 0) == V_REVOCATION);
    CHECK(own_rule(0, true, 0, 10, 20, true, REV_NO_CRL, 15, FLAG_ALLOW_NO_CRL) == 0 && own_rule(0, true, 0, 10, 20, true, 3, 15, FLAG_ALLOW_NO_CRL) == V_REVOCATION);
    CHECK(own_rule(0, true, 0, INT64_MIN, INT64_MAX, false, 0, INT64_MIN, 0) == 0 && own_rule(0, true, 0, INT64_MIN, INT64_MAX, false, 0, INT64_MAX, 0) == 0);
    // issuer_rule
    const uint32_t ca = F_V3 | F_HAS_BC | F_IS_CA;
    CHECK(issuer_rule(ca, 0) == 0 && issuer_rule(ca | F_HAS_KU, KU_KEY_CERT_SIGN) == 0 && issuer_rule(ca | F_HAS_KU, ~KU_KEY_CERT_SIGN) == V_KEY_USAGE);
    CHECK(issuer_rule(ca & ~F_V3, 0) == V_NOT_CA && issuer_rule(ca & ~F_HAS_BC, 0) == V_NOT_CA && issuer_rule(ca & ~F_IS_CA, 0) == V_NOT_CA);
    CHECK(issuer_rule(F_HAS_KU, 0) == V_NOT_CA);
    // the freshness rule
    CHECK(crl_time_status(false, true, 5, true, 9, 7, 0) == CRL_REFUSED && crl_time_status(true, false, 5, true, 9, 7, 0) == CRL_TIME);
    CHECK(crl_time_status(true, true, 5, true, 9, 4, 0) == CRL_NOT_YET && crl_time_status(true, true, 5, true, 9, 5, 0) == CRL_FRESH);
    CHECK(crl_time_status(true, true, 5, true, 9, 9, 0) == CRL_FRESH && crl_time_status(true, true, 5, true, 9, 10, 0) == CRL_STALE);
    CHECK(crl_time_status(true, true, 5, false, 0, 10, 0) == CRL_FRESH && crl_time_status(true, true, 5, false, 0, 10, FLAG_REQUIRE_NEXT_UPDATE) == CRL_STALE);
    CHECK(crl_time_status(true, true, 5, true, 9, 7, FLAG_REQUIRE_NEXT_UPDATE) == CRL_FRESH);
    // the scratch
    CHECK(scratch_bytes(0) == 0 && scratch_bytes(1) == 256 && scratch_bytes(32) == 256 && scratch_bytes(33) == 512 && scratch_bytes(MAX_CERTS + 1) == 0);
    // the key usage bits: KeyUsage bit 0 is the first byte's highest
    CHECK(reversed8(0x80) == 0x01 && reversed8(0x04) == KU_KEY_CERT_SIGN && reversed8(0xA5) == 0xA5 && reversed8(0x01) == 0x80);
}

int main() {
    const char* cases = std::getenv("PATH_CASES");
    const char* rows = std::getenv("PATH_ROWS");
    if (!cases || !rows) {
        std::fprintf(stderr, "PATH_CASES and PATH_ROWS expected\n");
        return 2;
    }
    std::ifstream in(cases);
    std::FILE* out = std::fopen(rows, "w");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open the case or the row file\n");
        return 2;
    }
    std::string line;
    bool first_walk = true;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string kind, hex;
        fields >> kind;
        if (kind == "T") {
            fields >> hex;
            const Bytes b = unhex(hex);
            const Block block(b.data(), b.size());
            const Time t = parse_time(Heap{block.p}, 0, (uint32_t)b.size());
            g_runs++;
            CHECK(t.ok || (t.seconds == 0 && t.next == 0));
            std::fprintf(out, "%d %lld %u\n", t.ok ? 1 : 0, (long long)t.seconds, t.next);
        } else if (kind == "W") {
            uint32_t flags = 0;
            fields >> flags >> hex;
            const Bytes b = unhex(hex);
            const Policy p = run_walk(b, b.size(), flags);
            if (p.status == ST_DER)
                CHECK(p.not_before == 0 && p.not_after == 0 && p.ext_off == 0 && p.ext_len == 0 && p.crit_off == 0 && p.path_len == 0 &&
                      p.key_usage == 0 && p.flags == 0 && p.n_ext == 0);
            CHECK(p.n_ext <= MAX_EXTS && p.n_crit <= p.n_ext && (p.ext_off == 0 || p.ext_off + (uint64_t)p.ext_len <= b.size()));
            std::fprintf(out, "%d %lld %lld %u %u %u %u %u %u %u %u\n", p.status, (long long)p.not_before, (long long)p.not_after, p.ext_off, p.ext_len,
                         p.crit_off, p.path_len, p.key_usage, p.flags, p.n_ext, p.n_crit);
            if (first_walk) {  // every proper prefix of at least 2 bytes is malformed (shorter ones the range rule refuses before the walk)
                first_walk = false;
                CHECK(p.status == ST_OK);
                for (size_t len = 2; len < b.size(); len++) CHECK(run_walk(b, len, flags).status == ST_DER);
            }
        } else if (kind == "C") {
            fields >> hex;
            const Bytes b = unhex(hex);
            const uint32_t n = (uint32_t)(b.size() / 8);
            uint64_t* words = static_cast<uint64_t*>(std::malloc(n ? 8 * (size_t)n : 8));
            for (uint32_t i = 0; i < n; i++) {
                words[i] = 0;
                for (int j = 7; j >= 0; j--) words[i] = words[i] << 8 | b[8 * i + j];
            }
            for (uint32_t i = 0; i < n; i++) {
                const Result r = climb(NodeWords{words}, i, n);
                g_runs++;
                CHECK(r.where < n && r.depth <= MAX_DEPTH);
                std::fprintf(out, "%s%d:%u:%u", i ? " " : "", r.verdict, r.where, r.depth);
            }
            std::fprintf(out, "\n");
            std::free(words);
        } else {
            std::fprintf(stderr, "unknown case line\n");
            g_fail++;
        }
    }
    std::fclose(out);
    calendar_edges();
    rule_edges();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("path_plan OK (%ld runs)\n", g_runs);
    return 0;
}
