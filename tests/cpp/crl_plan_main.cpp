// The walks, the placement and the hash of libmldsa_crl.so (fips204_amd/crl/crl_plan.h) on their own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_crl_cpu.py.  The test writes its cases -- valid CRLs, every
// defect, single-byte mutants -- as lines of hex into the file CRL_CASES names; every run of walk_crl and walk_entry reads a heap
// block of EXACTLY the declared length, so that the sanitizer sees any byte read outside [off, off + len).  For every case one row goes
// to the file CRL_ROWS names -- the walk's fields, then the entries the hop finds with their serials, offsets and hashes -- which the
// test compares with the Python restatement of tests/crl_cases.py.  Every proper prefix of the first case must be malformed.  Then
// the edges that need no case: the serial rule, the table's size, the placement, the window's chunks, the certificate's serial, the
// link rule and the order of the lookup's answers.  Exit status 0 and "crl_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../fips204_amd/crl/crl_plan.h"

using namespace mldsa_crl;
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
    explicit Block(const uint8_t* src, size_t len) : p(static_cast<uint8_t*>(std::malloc(len ? len : 1))) {
        if (len) std::memcpy(p, src, len);
    }
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
};

static Bytes from_hex(const std::string& s) {
    Bytes b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return b;
}

// one case: the row of the walk, then the entries as the kernel finds them -- the hop from header to header, walk_entry on each, at
// most entries_bound of them, ending exactly at the list's end
static void run_case(uint32_t index, const Bytes& der, std::FILE* out) {
    const Block block(der.data(), der.size());
    const Heap f{block.p};
    CrlWalk w = walk_crl(f, (uint32_t)der.size());
    g_runs++;
    if (w.status == ST_DER)
        CHECK(w.tbs_off == 0 && w.tbs_len == 0 && w.issuer_len == 0 && w.revoked_len == 0 && w.ext_len == 0 && w.sig_set == 0 && w.sig_off == 0);
    CHECK((w.sig_off != 0) == (w.status == ST_OK) && (w.sig_set != 0) == (w.status == ST_OK));
    struct Found {
        Serial s;
        uint32_t at;
    };
    std::vector<Found> found;
    int status = w.status;
    if (status == ST_OK) {
        const uint64_t bound = entries_bound(w.revoked_len);
        uint32_t pos = w.revoked_off;
        const uint32_t end = w.revoked_off + w.revoked_len;
        bool bad = false;
        while (pos < end && found.size() < bound && !bad) {
            const uint32_t next = hop(f, pos, end);
            const Entry e = walk_entry(f, pos, end);
            g_runs++;
            if (next == 0 || !e.ok) {
                bad = true;
                CHECK(next != 0 || !e.ok);  // what the hop cannot read walk_entry refuses
                break;
            }
            CHECK(e.next == next && next > pos && next - pos >= ENTRY_MIN && serial_ok(f, e.serial_at, e.serial_len));
            found.push_back({load_serial(f, e.serial_at, e.serial_len), pos});
            pos = next;
        }
        if (bad || pos != end) {
            status = ST_ENTRY;
            found.clear();
        }
    }
    std::fprintf(out, "%d %u %u %u %u %u %u %u %u %u %u %u %u %zu", status, w.tbs_off, w.tbs_len, w.sig_off, w.issuer_off, w.issuer_len, w.this_off,
                 w.next_off, w.revoked_off, w.revoked_len, w.ext_off, w.ext_len, w.sig_set, found.size());
    for (const Found& e : found) {
        std::fprintf(out, " ");
        for (uint32_t j = 0; j < e.s.len; j++) std::fprintf(out, "%02x", (e.s.w[j / 4] >> (8 * (j % 4))) & 0xFF);
        std::fprintf(out, "@%u#%08x", e.at, hash_serial(index, e.s));
    }
    std::fprintf(out, "\n");
}

static void prefixes(const Bytes& der) {
    for (size_t len = 2; len < der.size(); len++) {
        const Block block(der.data(), len);
        CHECK(walk_crl(Heap{block.p}, (uint32_t)len).status == ST_DER);
        g_runs++;
    }
}

static void edges() {
    const auto ok = [](const Bytes& b) {
        const Block block(b.data(), b.size());
        return serial_ok(Heap{block.p}, 0, (uint32_t)b.size());
    };
    CHECK(!ok({}) && ok({0x00}) && ok({0x7F}) && ok({0x80}) && ok({0xFF}) && ok({0x00, 0x80}) && ok({0x00, 0xFF}) && ok({0xFF, 0x7F}) && ok({0xFF, 0x00}));
    CHECK(!ok({0x00, 0x00}) && !ok({0x00, 0x7F}) && !ok({0xFF, 0x80}) && !ok({0xFF, 0xFF}) && ok({0x01, 0x00}) && ok({0x81, 0xFF}));
    CHECK(ok(Bytes(20, 0x55)) && !ok(Bytes(21, 0x55)));
    // the serial's words: the bytes as they stand, zero-padded, little endian
    const Bytes s = {0x00, 0x81, 0x02, 0x03, 0x04};
    const Block sb(s.data(), s.size());
    const Serial ser = load_serial(Heap{sb.p}, 0, 5);
    CHECK(ser.len == 5 && ser.w[0] == 0x03028100u && ser.w[1] == 0x04u && ser.w[2] == 0 && ser.w[3] == 0 && ser.w[4] == 0);
    Serial other = ser;
    other.len = 6;  // 00 81 02 03 04 and 00 81 02 03 04 00 differ in length alone
    CHECK(hash_serial(3, ser) != hash_serial(3, other) && hash_serial(3, ser) != hash_serial(4, ser) && hash_serial(3, ser) == hash_serial(3, ser));
    // the table and the placement
    CHECK(table_slots(0) == 64 && table_slots(32) == 64 && table_slots(33) == 128 && table_slots(65) == 256 && table_slots(1u << 30) == (1ull << 31));
    CHECK(table_slots((1ull << 30) + 1) == 0 && entries_bound(0) == 0 && entries_bound(19) == 0 && entries_bound(20) == 1 && entries_bound(41) == 2);
    CHECK(scratch_bytes(0) == 0 && scratch_bytes(1) == 256 && scratch_bytes(256 * 32) == 256 && scratch_bytes(256 * 32 + 1) == 512);
    CHECK(scratch_bytes(MAX_CRLS + 1) == 0 && n_blocks(257) == 2);
    CHECK(place_status(0, 0, 0) == ST_OK && place_status(0, 1, 0) == ST_SPACE && place_status(5, 5, 10) == ST_OK && place_status(5, 6, 10) == ST_SPACE);
    CHECK(place_status(11, 0, 10) == ST_SPACE);
    // the window: every loaded chunk lies inside the CRL, the loaded part is what the chunks cover, and the position asked for is in
    // it unless the CRL's own ends are in the way
    for (uint32_t mis = 0; mis < 16; mis++)
        for (uint32_t len : {2u, 15u, 16u, 17u, 31u, 32u, 33u, 1000u, 1024u, 1040u, 5000u})
            for (uint32_t pos = 0; pos < len; pos += (len > 64 ? 7 : 1)) {
                const Window w = window_at(mis, len, pos);
                CHECK(w.ws % 16 == 0 && w.ws <= (uint64_t)mis + pos && (uint64_t)mis + pos < w.ws + 16);
                uint64_t lo = ~0ull, hi = 0;
                for (uint32_t k = 0; k < WINDOW / 16; k++)
                    if (window_chunk(w, k)) {
                        const uint64_t a = w.ws + 16 * k;
                        CHECK(a >= mis && a + 16 <= (uint64_t)mis + len);
                        lo = a < lo ? a : lo;
                        hi = a + 16 > hi ? a + 16 : hi;
                    }
                if (hi != 0) CHECK(lo == w.lo && hi == w.hi);
                else CHECK(w.lo >= w.hi);
                for (uint64_t q = mis; q < (uint64_t)mis + len; q += 5)
                    if (window_holds(w, q)) CHECK(q >= lo && q < hi && q - w.ws < WINDOW);
                const uint64_t q0 = (uint64_t)mis + pos;
                if (q0 >= ((mis + 15u) & ~15u) && (q0 | 15) < (uint64_t)mis + len) CHECK(window_holds(w, q0));
            }
    // the certificate's serial
    const auto cs = [](const Bytes& b) {
        const Block block(b.data(), b.size());
        return cert_serial(Heap{block.p}, (uint32_t)b.size());
    };
    CHECK(cs({0x30, 0x03, 0x02, 0x01, 0x05}).len == 1 && cs({0x30, 0x03, 0x02, 0x01, 0x05}).w[0] == 5);
    CHECK(cs({0x30, 0x08, 0xA0, 0x03, 0x02, 0x01, 0x02, 0x02, 0x01, 0x85}).w[0] == 0x85 && cs({0x30, 0x04, 0x02, 0x02, 0x00, 0x05}).len == 0);
    CHECK(cs({0x30, 0x02, 0x02, 0x00}).len == 0 && cs({0x31, 0x03, 0x02, 0x01, 0x05}).len == 0 && cs({0x30, 0x03, 0x04, 0x01, 0x05}).len == 0);
    CHECK(cs({0x30, 0x03, 0x02, 0x02, 0x05}).len == 0 && cs({0x30}).len == 0 && cs({0x30, 0x05, 0xA0, 0x03, 0x02, 0x01, 0x02}).len == 0);
    // the link rule and the answers
    const uint64_t n = 10;
    CHECK(link_status(ST_DER, 0, 3, n, ST_OK, 44) == ST_DER && link_status(ST_ENTRY, 44, 3, n, ST_OK, 44) == ST_ENTRY);
    CHECK(link_status(ST_SPACE, 44, 30, n, 0, 0) == ST_SPACE && link_status(ST_OK, 44, 10, n, 0, 0) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 0xFFFFFFFFu, n, 0, 0) == ST_ISSUER && link_status(ST_OK, 44, 3, n, ST_RANGE, 44) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 3, n, ST_DER, 44) == ST_ISSUER && link_status(ST_OK, 44, 3, n, ST_OK, 0) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 3, n, ST_OK, 65) == ST_ISSUER && link_status(ST_OK, 44, 3, n, ST_ALG, 44) == ST_OK);
    CHECK(link_status(ST_OK, 87, 9, n, 7, 87) == ST_OK && link_status(ST_OK, 44, 0, 0, 0, 0) == ST_ISSUER);
    // a CRL always names an issuer: 0xFFFFFFFF, the certificate's "no issuer", is out of range under every cap and never "parse only"
    static_assert(MAX_CERTS == (size_t)1 << 30 && mldsa_x509::NO_ISSUER == 0xFFFFFFFFu && mldsa_x509::ST_PARSE_ONLY == 7, "the caps and the sentinel");
    CHECK(link_status(ST_OK, 44, 0xFFFFFFFFu, (uint64_t)1 << 30, 0, 0) == ST_ISSUER && link_status(ST_OK, 44, 0xFFFFFFFFu, MAX_CERTS, ST_OK, 44) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, (1u << 30) - 1, MAX_CERTS, ST_OK, 44) == ST_OK && link_status(ST_OK, 44, 1u << 30, MAX_CERTS, ST_OK, 44) == ST_ISSUER);
    // same_alg, which walk_crl takes from the certificate's plan: a heap block of exactly the two contents, each byte in turn
    {
        uint8_t* block = static_cast<uint8_t*>(std::malloc(2 * OID_LEN));
        const uint8_t oid[OID_LEN] = {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x03, 0x12};
        std::memcpy(block, oid, OID_LEN);
        std::memcpy(block + OID_LEN, oid, OID_LEN);
        CHECK(same_alg(Heap{block}, 0, OID_LEN));
        for (uint32_t j = 0; j < OID_LEN; j++) {
            block[j] ^= 0x40;
            CHECK(!same_alg(Heap{block}, 0, OID_LEN) && !same_alg(Heap{block}, OID_LEN, 0));
            block[j] ^= 0x40;
        }
        std::free(block);
    }
    CHECK(answer(false, false, false, false, false, true) == REV_NO_CRL && answer(true, false, true, true, true, true) == REV_CRL_INDEX);
    CHECK(answer(true, true, false, false, false, true) == REV_CRL_REFUSED && answer(true, true, true, false, false, true) == REV_CERT);
    CHECK(answer(true, true, true, true, false, true) == REV_SCOPE && answer(true, true, true, true, true, true) == REV_REVOKED);
    CHECK(answer(true, true, true, true, true, false) == REV_GOOD);
}

int main() {
    const char* cases = std::getenv("CRL_CASES");
    const char* rows = std::getenv("CRL_ROWS");
    if (!cases || !rows) {
        std::fprintf(stderr, "CRL_CASES and CRL_ROWS expected\n");
        return 2;
    }
    std::ifstream in(cases);
    std::FILE* out = std::fopen(rows, "w");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open the case or the row file\n");
        return 2;
    }
    std::string line;
    uint32_t index = 0;
    while (std::getline(in, line)) {
        const Bytes der = from_hex(line);
        if (index == 0) prefixes(der);
        run_case(index++, der, out);
    }
    std::fclose(out);
    CHECK(index > 0);
    edges();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("crl_plan OK (%u cases, %ld walks)\n", index, g_runs);
    return 0;
}
