// The walk, the rules and the TBSCertificate bytes of libmldsa_csr.so (fips204_amd/csr/csr_plan.h) on their own: pure host code, compiled
// with -fsanitize=address,undefined and run as a child process by tests/test_csr_cpu.py.  The cases come from a table the Python side
// writes (its path in CSR_TABLE), one per line:
//     W <status> <cri_off> <cri_len> <subject_off> <subject_len> <spki_off> <spki_len> <sig_off> <key_off> <set> <hex of the declared bytes>
//                                          a request to walk, and everything the walk must find
//     B <hex>                              the blob of the T lines that follow
//     T <status> <ok> <row: status subject_off subject_len spki_off spki_len key_off set> <entry: serial_off issuer_off validity_off ext_off issuer_len
//       validity_len ext_len serial_len set flags reserved> <hex of the expected TBSCertificate, or ->
//                                          stage 2's rules up to LONG on the blob, and the bytes of an accepted request
// Every walk reads a heap block of EXACTLY the declared length and every rule a blob block of exactly its length, so that the
// sanitizer sees any byte read outside.  An accepted request's TBSCertificate is assembled with the header's own functions into a heap
// block of exactly tbs_len bytes, compared with the expected bytes, walked by mldsa_x509sign::walk_tbs under the entry's set (the
// contract), framed and walked by mldsa_x509::walk: subject and key are where the pieces were copied.  Then every proper prefix of the
// first accepted request of each set, and the arithmetic at its bounds.  Exit status 0 and "csr_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fips204_amd/csr/csr_plan.h"

using namespace mldsa_csr;
typedef std::vector<uint8_t> Bytes;

static int g_fail = 0;
static long g_walks = 0, g_rules = 0, g_written = 0;
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

// a heap block of exactly b.size() bytes (one byte for an empty one)
static uint8_t* block_of(const Bytes& b, size_t len) {
    uint8_t* block = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len) std::memcpy(block, b.data(), len);
    return block;
}

static Walk run_walk(const Bytes& b, size_t len) {
    uint8_t* block = block_of(b, len);
    const Walk w = walk(Heap{block}, (uint32_t)len);
    std::free(block);
    g_walks++;
    return w;
}

static Bytes unhex(const std::string& s) {
    const auto nibble = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    Bytes b(s.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)(nibble(s[2 * i]) << 4 | nibble(s[2 * i + 1]));
    return b;
}

// the TBSCertificate of an accepted request, as k_csr_tbs_write lays it down
static Bytes assemble(const uint8_t* blob, const mldsa_csr_fields& r, const mldsa_csr_issue& e) {
    const uint32_t len = (uint32_t)tbs_len(e, r);
    const Pieces p = pieces(e, r);
    uint8_t* t = static_cast<uint8_t*>(std::malloc(len));
    for (uint32_t j = 0; j < PREFIX_LEN; j++) t[j] = (uint8_t)prefix_byte(j, len, e.serial_len);
    for (uint32_t j = 0; j < ALG_LEN; j++) t[p.alg_at + j] = (uint8_t)alg_byte(j, class_of_set(e.set));
    for (int k = 0; k < 6; k++)
        if (p.len[k]) std::memcpy(t + p.at[k], blob + piece_off(e, r, k), p.len[k]);
    CHECK(p.at[5] + p.len[5] == len);
    Bytes out(t, t + len);
    std::free(t);
    return out;
}

static void tbs_case(const uint8_t* blob, uint64_t blob_len, const mldsa_csr_fields& r, const mldsa_csr_issue& e, uint32_t ok, int expected,
                     const std::string& hex) {
    const int st = tbs_status(Heap{blob}, blob_len, r, e, ok);
    g_rules++;
    CHECK(st == expected);
    if (st != ST_OK) {
        CHECK(hex == "-");
        return;
    }
    const Bytes tbs = assemble(blob, r, e), want = unhex(hex);
    g_written++;
    CHECK(tbs == want);
    const uint32_t len = (uint32_t)tbs.size();
    CHECK(write_allowed(r, e, 0, len, blob_len, len) && write_allowed(r, e, 7, len, blob_len, (uint64_t)len + 7));
    CHECK(!write_allowed(r, e, 0, len, blob_len, len - 1) && !write_allowed(r, e, 1, len, blob_len, len));
    CHECK(!write_allowed(r, e, 0, len - 1, blob_len, len) && !write_allowed(r, e, ~0ull - 3, len, blob_len, ~0ull));
    // the contract: x509sign's walk and its ALG rule accept the TBSCertificate for the entry's set
    uint8_t* block = block_of(tbs, len);
    CHECK(mldsa_x509sign::walk_tbs(Heap{block}, len, e.set) == mldsa_x509sign::ST_OK);
    std::free(block);
    // framed as x509sign frames it, the verifying side's walk finds subject and key where the request's pieces went
    const int c = class_of_set(e.set);
    const uint32_t n = mldsa_x509sign::cert_len(c, len);
    uint8_t* cert = static_cast<uint8_t*>(std::calloc(n, 1));
    for (uint32_t j = 0; j < 4; j++) cert[j] = (uint8_t)mldsa_x509sign::header_byte(j, n);
    std::memcpy(cert + 4, tbs.data(), len);
    for (uint32_t j = 0; j < 18; j++) cert[4 + len + j] = (uint8_t)mldsa_x509sign::trailer_byte(j, c);
    const mldsa_x509::Walk w = mldsa_x509::walk(Heap{cert}, n);
    CHECK(w.status == mldsa_x509::ST_OK && w.sig_set == e.set && w.tbs_off == 4 && w.tbs_len == len);
    CHECK(w.subject_len == r.subject_len && std::memcmp(cert + w.subject_off, blob + r.subject_off, r.subject_len) == 0);
    CHECK(w.issuer_len == e.issuer_len && std::memcmp(cert + w.issuer_off, blob + e.issuer_off, e.issuer_len) == 0);
    CHECK(w.key_set == r.set && w.key_off == 4 + pieces(e, r).at[4] + (uint32_t)(r.key_off - r.spki_off));
    std::free(cert);
}

static void arithmetic() {
    static_assert(PREFIX_LEN + ALG_LEN == 24 && max_tbs_len(CLASS_44) == 63097 && max_tbs_len(CLASS_87) == 60890, "the fixed bytes, the LONG bounds");
    mldsa_csr_issue e = {};
    mldsa_csr_fields r = {};
    e.serial_len = 255;
    e.issuer_len = e.validity_len = e.ext_len = r.subject_len = r.spki_len = 0xFFFFFFFFu;
    CHECK(tbs_len(e, r) == 24ull + 255 + 5ull * 0xFFFFFFFFull);  // 64 bits: nothing wraps
    for (int c = 0; c < 3; c++) {
        uint8_t oid[OID_LEN];
        for (uint32_t j = 0; j < OID_LEN; j++) oid[j] = (uint8_t)alg_byte(2 + j, c);
        CHECK(alg_byte(0, c) == 0x30 && alg_byte(1, c) == OID_LEN && oid_set(Heap{oid}, 0) == (uint32_t)mldsa_rec::set_of_class(c));
    }
    CHECK(prefix_byte(2, 0x1234 + 4, 9) == 0x12 && prefix_byte(3, 0x1234 + 4, 9) == 0x34 && prefix_byte(10, 300, 9) == 9);
    CHECK(plan_bytes(0) == 0 && plan_bytes(1) == 512 && plan_bytes(256) == 256 + 1024 && plan_bytes(257) == 256 + 1280);
    CHECK(plan_bytes(MAX_REQUESTS) != 0 && plan_bytes(MAX_REQUESTS + 1) == 0);
    CHECK(n_blocks(0) == 0 && n_blocks(256) == 1 && n_blocks(257) == 2 && plan_sums_bytes(16 * 256) == 256 && plan_sums_bytes(16 * 256 + 1) == 512);
    // same_alg, which the walk takes from the certificate's plan: a heap block of exactly the two contents, each byte in turn
    uint8_t* block = static_cast<uint8_t*>(std::malloc(2 * OID_LEN));
    for (uint32_t j = 0; j < 2 * OID_LEN; j++) block[j] = (uint8_t)alg_byte(2 + j % OID_LEN, 1);
    CHECK(same_alg(Heap{block}, 0, OID_LEN));
    for (uint32_t j = 0; j < OID_LEN; j++) {
        block[OID_LEN + j] ^= 0x01;
        CHECK(!same_alg(Heap{block}, 0, OID_LEN) && !same_alg(Heap{block}, OID_LEN, 0));
        block[OID_LEN + j] ^= 0x01;
    }
    std::free(block);
}

int main() {
    const char* path = std::getenv("CSR_TABLE");
    if (!path) {
        std::fprintf(stderr, "CSR_TABLE is not set\n");
        return 2;
    }
    std::ifstream in(path);
    std::string line;
    Bytes first[3];
    uint8_t* blob = nullptr;
    uint64_t blob_len = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, hex;
        ss >> kind;
        if (kind == "W") {
            int expected = -1;
            Walk x;
            ss >> expected >> x.cri_off >> x.cri_len >> x.subject_off >> x.subject_len >> x.spki_off >> x.spki_len >> x.sig_off >> x.key_off >>
                x.set >> hex;
            CHECK(!ss.fail());
            const Bytes der = unhex(hex);
            CHECK(der.size() >= 2);
            const Walk w = run_walk(der, der.size());
            CHECK(w.status == expected);
            CHECK(w.cri_off == x.cri_off && w.cri_len == x.cri_len && w.subject_off == x.subject_off && w.subject_len == x.subject_len);
            CHECK(w.spki_off == x.spki_off && w.spki_len == x.spki_len && w.sig_off == x.sig_off && w.key_off == x.key_off && w.set == x.set);
            if (expected == ST_OK && first[class_of_set(w.set)].empty()) first[class_of_set(w.set)] = der;
        } else if (kind == "B") {
            ss >> hex;
            const Bytes b = unhex(hex);
            std::free(blob);
            blob = block_of(b, b.size());
            blob_len = b.size();
        } else if (kind == "T") {
            int expected = -1;
            uint32_t ok = 0, row_status = 0, serial_len = 0, set = 0, flags = 0, reserved = 0;
            mldsa_csr_fields r = {};
            mldsa_csr_issue e = {};
            ss >> expected >> ok >> row_status >> r.subject_off >> r.subject_len >> r.spki_off >> r.spki_len >> r.key_off >> set;
            r.status = (uint8_t)row_status;
            r.set = (uint8_t)set;
            ss >> e.serial_off >> e.issuer_off >> e.validity_off >> e.ext_off >> e.issuer_len >> e.validity_len >> e.ext_len >> serial_len >> set >>
                flags >> reserved >> hex;
            e.serial_len = (uint8_t)serial_len;
            e.set = (uint8_t)set;
            e.flags = (uint8_t)flags;
            e.reserved = (uint8_t)reserved;
            CHECK(!ss.fail() && blob != nullptr);
            tbs_case(blob, blob_len, r, e, ok, expected, hex);
        } else if (!kind.empty()) {
            CHECK(false);
        }
    }
    std::free(blob);
    CHECK(g_walks > 0 && g_rules > 0 && g_written > 0);
    for (int c = 0; c < 3; c++) {  // every proper prefix of at least 2 bytes is malformed
        CHECK(!first[c].empty());
        for (size_t len = 2; len < first[c].size(); len++) CHECK(run_walk(first[c], len).status == ST_DER);
    }
    arithmetic();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("csr_plan OK (%ld walks, %ld rules, %ld TBSCertificates)\n", g_walks, g_rules, g_written);
    return 0;
}
