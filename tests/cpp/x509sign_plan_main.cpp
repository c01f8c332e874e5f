// The rules, the walk and the frame of libmldsa_x509sign.so (fips204_amd/x509sign/x509sign_plan.h) on their own: pure host code, compiled
// with -fsanitize=address,undefined and run as a child process by tests/test_x509sign_cpu.py.  The cases come from a table the Python
// side writes (its path in X509SIGN_TABLE), one per line:
//     W <set> <expected status> <hex of the TBS's declared bytes>        a TBS to walk: the defect list and the single-byte sweep
//     E <expected status> <off> <rnd_off> <len> <key> <set> <flags> <reserved> <blob_len> <n44> <n65> <n87>     an entry's rules
// Every walk reads a heap block of EXACTLY the declared length, so that the sanitizer sees any byte read at or behind len.  Each TBS is
// then framed on the host with the header's own functions -- into a heap block of exactly cert_len bytes -- and the certificate walked
// by mldsa_x509::walk: an accepted TBS must give ST_OK with tbs_off = 4, tbs_len = len and sig_off = the hole (the contract); a refused
// one, framed all the same, must NOT give ST_OK with the entry's set.  Then every proper prefix of the first accepted TBS of each set,
// and the frame's arithmetic at its bounds.  Exit status 0 and "x509sign_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fips204_amd/x509sign/x509sign_plan.h"

using namespace mldsa_x509sign;
typedef std::vector<uint8_t> Bytes;

static int g_fail = 0;
static long g_walks = 0, g_accepted = 0, g_entries = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

struct Heap {
    const uint8_t* p;
    uint32_t operator()(uint64_t pos) const { return p[pos]; }
};

static int run_walk(const Bytes& b, size_t len, uint32_t set) {
    uint8_t* block = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(block, b.data(), len);
    const int st = walk_tbs(Heap{block}, (uint32_t)len, set);
    std::free(block);
    g_walks++;
    return st;
}

// the certificate around the TBS, the hole filled with a pattern, walked by the verifying side's walk
static mldsa_x509::Walk framed_walk(const Bytes& tbs, uint32_t set, uint32_t* total) {
    const int c = class_of_set(set);
    const uint32_t len = (uint32_t)tbs.size(), n = cert_len(c, len);
    uint8_t* cert = static_cast<uint8_t*>(std::malloc(n));
    for (uint32_t j = 0; j < HEADER_LEN; j++) cert[j] = (uint8_t)header_byte(j, n);
    std::memcpy(cert + HEADER_LEN, tbs.data(), len);
    for (uint32_t j = 0; j < TRAILER_LEN; j++) cert[HEADER_LEN + len + j] = (uint8_t)trailer_byte(j, c);
    for (uint32_t j = 0; j < sig_len(c); j++) cert[len + FRAME_LEN + j] = (uint8_t)(j * 29 + 5);
    const mldsa_x509::Walk w = mldsa_x509::walk(Heap{cert}, n);
    std::free(cert);
    *total = n;
    return w;
}

static void walk_case(uint32_t set, int expected, const Bytes& tbs) {
    const int st = run_walk(tbs, tbs.size(), set);
    CHECK(st == expected);
    CHECK(st == ST_OK || st == ST_DER || st == ST_ALG);
    uint32_t total = 0;
    const mldsa_x509::Walk w = framed_walk(tbs, set, &total);
    if (st == ST_OK) {
        g_accepted++;
        CHECK(w.status == mldsa_x509::ST_OK && w.sig_set == set);
        CHECK(w.tbs_off == HEADER_LEN && w.tbs_len == tbs.size() && w.sig_off == tbs.size() + FRAME_LEN);
        CHECK(w.sig_off + sig_len(class_of_set(set)) == total);
    } else {
        CHECK(!(w.status == mldsa_x509::ST_OK && w.sig_set == set));
    }
}

static Bytes unhex(const std::string& s) {
    Bytes b(s.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return b;
}

static void arithmetic() {
    static_assert(max_tbs_len(CLASS_44) == 63097 && max_tbs_len(CLASS_65) == 62208 && max_tbs_len(CLASS_87) == 60890, "the LONG bounds");
    static_assert(cert_len(CLASS_44, 0) == 2442 && cert_len(CLASS_65, 1000) == 4331 && cert_len(CLASS_87, 60890) == 65539, "cert_len");
    for (int c = 0; c < 3; c++) {
        const uint32_t n = cert_len(c, max_tbs_len(c));
        CHECK(n == 65539 && header_byte(0, n) == 0x30 && header_byte(1, n) == 0x82 && header_byte(2, n) == 0xFF && header_byte(3, n) == 0xFF);
        const uint32_t m = cert_len(c, 2);  // the shortest content still needs two length bytes
        CHECK(m - HEADER_LEN >= 2438 && ((header_byte(2, m) << 8) | header_byte(3, m)) == m - HEADER_LEN);
        CHECK(((trailer_byte(15, c) << 8) | trailer_byte(16, c)) == 1 + sig_len(c) && trailer_byte(17, c) == 0 && trailer_byte(12, c) == 0x11u + c);
        CHECK(trailer_byte(0, c) == 0x30 && trailer_byte(1, c) == OID_LEN && trailer_byte(13, c) == 0x03 && trailer_byte(14, c) == 0x82);
        uint8_t oid[OID_LEN];
        for (uint32_t j = 0; j < OID_LEN; j++) oid[j] = (uint8_t)trailer_byte(2 + j, c);
        CHECK(oid_set(Heap{oid}, 0) == (uint32_t)mldsa_rec::set_of_class(c));
    }
    CHECK(plan_bytes(0) == 0 && plan_bytes(1) == 512 && plan_bytes(256) == 256 + 1024 && plan_bytes(257) == 256 + 1280);
    CHECK(plan_bytes(MAX_CERTS) != 0 && plan_bytes(MAX_CERTS + 1) == 0);
}

int main() {
    const char* path = std::getenv("X509SIGN_TABLE");
    if (!path) {
        std::fprintf(stderr, "X509SIGN_TABLE is not set\n");
        return 2;
    }
    std::ifstream in(path);
    std::string line;
    Bytes first[3];
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "W") {
            uint32_t set = 0;
            int expected = -1;
            std::string hex;
            ss >> set >> expected >> hex;
            const Bytes tbs = unhex(hex);
            CHECK(class_of_set(set) != CLASS_REFUSED && tbs.size() >= 2);
            walk_case(set, expected, tbs);
            if (expected == ST_OK && first[class_of_set(set)].empty()) first[class_of_set(set)] = tbs;
        } else if (kind == "E") {
            int expected = -1;
            uint64_t off = 0, rnd_off = 0, blob_len = 0, nk[3] = {0, 0, 0};
            uint32_t len = 0, key = 0, set = 0, flags = 0, reserved = 0;
            ss >> expected >> off >> rnd_off >> len >> key >> set >> flags >> reserved >> blob_len >> nk[0] >> nk[1] >> nk[2];
            CHECK(!ss.fail());
            CHECK(entry_status(off, rnd_off, len, key, set, flags, reserved, blob_len, nk[0], nk[1], nk[2]) == expected);
            g_entries++;
        } else if (!kind.empty()) {
            CHECK(false);
        }
    }
    CHECK(g_walks > 0 && g_accepted > 0 && g_entries > 0);
    for (int c = 0; c < 3; c++) {  // every proper prefix of at least 2 bytes is malformed
        CHECK(!first[c].empty());
        for (size_t len = 2; len < first[c].size(); len++) CHECK(run_walk(first[c], len, (uint32_t)mldsa_rec::set_of_class(c)) == ST_DER);
    }
    arithmetic();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("x509sign_plan OK (%ld walks, %ld accepted, %ld entries)\n", g_walks, g_accepted, g_entries);
    return 0;
}
