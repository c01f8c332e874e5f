// The identifier walk, the key comparison, the hash and the table's size of libmldsa_find.so (fips204_amd/find/find_plan.h) on their own:
// pure host code, compiled with -fsanitize=address,undefined and run as a child process by tests/test_find_cpu.py.  The test writes its
// cases as lines into the file FIND_CASES names ("-" stands for no bytes):
//   I <hex>                                   the content of one Extensions SEQUENCE: walk_ids on a heap block of EXACTLY these bytes, so
//                                             that the sanitizer sees any byte read outside the range
//   K <kind> <set> <name> <id> <kind> <set> <name> <id>
//                                             two keys, each on heap blocks of exactly its bytes: keys_equal, whether the 64-bit hashes
//                                             are equal, and whether every hash_bits 1 ... 64 gives the 64-bit hash's low bits
//   S <n>                                     table_slots and scratch_bytes
// For every case one row goes to the file FIND_ROWS names, which the test compares with the Python restatement of tests/find_cases.py.
// A proper prefix of the first I case is accepted only where it ends with one of its extensions.  Then the edges that need no case.  Exit status 0 and "find_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../fips204_amd/find/find_plan.h"

using namespace mldsa_find;
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
    if (s == "-") return Bytes();
    Bytes out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

static Ids run_ids(const Bytes& b, size_t len) {
    const Block block(b.data(), len);
    g_runs++;
    return walk_ids(Heap{block.p}, 0, (uint32_t)len);
}

// Both keys in one address space, as the blob is for the kernels: the functor maps a position to one of four exact heap blocks.
struct FourBlocks {
    const uint8_t* p[4];
    uint64_t len[4];
    uint32_t operator()(uint64_t pos) const {
        const uint64_t which = pos >> 32, at = pos & 0xFFFFFFFFu;
        if (which >= 4 || at >= len[which]) std::abort();  // a byte outside a key's own ranges
        return p[which][at];
    }
};

static const uint64_t S0 = 0x0123456789ABCDEFull, S1 = 0xFEDCBA9876543210ull;

static void edges() {
    static_assert(table_slots(0) == 64 && table_slots(16) == 64 && table_slots(17) == 128 && table_slots(MAX_CERTS) == 4 * MAX_CERTS &&
                      table_slots(MAX_CERTS + 1) == 0 && scratch_bytes(MAX_CERTS + 1) == 0,
                  "the plan is constexpr");
    static_assert(inside(10, 5, 10, 5) && !inside(9, 5, 10, 5) && !inside(10, 6, 10, 5) && inside(15, 0, 10, 5) && !inside(16, 0, 10, 5) &&
                      !inside(~0ull, 2, 10, 5) && !inside(12, ~0ull, 10, 5),
                  "a range is followed only inside its certificate");
    static_assert(candidate_row(ST_OK, 44, ST_OK) && candidate_row(ST_ALG, 65, ST_OK) && candidate_row(ST_SIG, 87, ST_OK) &&
                      !candidate_row(ST_RANGE, 44, ST_OK) && !candidate_row(ST_DER, 44, ST_OK) && !candidate_row(ST_OK, 0, ST_OK) &&
                      !candidate_row(ST_OK, 44, ST_EXT) && seeker_row(ST_OK, 44, ST_OK) && !seeker_row(ST_ALG, 44, ST_OK) &&
                      !seeker_row(ST_OK, 0, ST_OK) && !seeker_row(ST_OK, 44, ST_DER),
                  "who takes part");
    // the join of two lookups and the answer's status
    Match a, b;
    CHECK(result_status(false, a) == R_CERT && result_status(true, a) == R_NONE);
    a.lowest = 7, a.count = 2, b.lowest = 3, b.count = 1;
    Match m = join(a, b);
    CHECK(m.lowest == 3 && m.count == 3 && !m.space && result_status(true, m) == R_FOUND);
    m = join(a, Match());
    CHECK(m.lowest == 7 && m.count == 2);
    b.space = true;
    m = join(a, b);
    CHECK(m.space && m.count == 0 && m.lowest == NO_ISSUER && result_status(true, m) == R_SPACE);
    // no hash is the empty tag, at any width; the seed matters
    Key k;
    k.kind = KIND_ANY, k.set = 44;
    const uint8_t none = 0;
    const Heap f{&none};
    for (int bits = 1; bits <= 64; bits++) {
        const uint64_t h = key_hash(f, k, S0, S1, bits);
        CHECK(h != EMPTY_TAG && (bits == 64 || h >> bits == 0));
    }
    CHECK(finish_hash(0, k, 0, 64) != EMPTY_TAG);
    CHECK(key_hash(f, k, S0, S1, 64) != key_hash(f, k, S0 + 1, S1, 64) || k.name_len == 0);
    CHECK(key_hash(f, k, S0, S1, 64) != key_hash(f, k, S0, S1 + 1, 64));
    // the layout's parts lie behind one another, 256-byte aligned, and the whole is the header's formula
    for (size_t n : {(size_t)0, (size_t)1, (size_t)16, (size_t)17, (size_t)1000, (size_t)65536}) {
        const Layout L = layout(n);
        const size_t s = table_slots(n);
        CHECK(L.tags == 0 && L.owners >= 8 * s && L.counts >= L.owners + 4 * s && L.slot_of >= L.counts + 4 * s && L.keys >= L.slot_of + 8 * n && L.overflow >= L.keys + 64 * n &&
              L.ca_crl >= L.overflow + 4 * OVERFLOW_MAX && L.total >= L.ca_crl + 4 * n);
        CHECK(L.owners % 256 == 0 && L.counts % 256 == 0 && L.slot_of % 256 == 0 && L.keys % 256 == 0 && L.overflow % 256 == 0 && L.ca_crl % 256 == 0 && L.total % 256 == 0);
    }
}

int main() {
    const char* cases = std::getenv("FIND_CASES");
    const char* rows = std::getenv("FIND_ROWS");
    if (!cases || !rows) {
        std::fprintf(stderr, "FIND_CASES and FIND_ROWS must name files\n");
        return 2;
    }
    std::ifstream in(cases);
    std::ofstream out(rows);
    std::string line;
    bool first = true;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        ls >> kind;
        if (kind == "I") {
            std::string hex;
            ls >> hex;
            const Bytes b = unhex(hex);
            const Ids w = run_ids(b, b.size());
            out << w.status << " " << w.ski_off << " " << w.ski_len << " " << w.aki_off << " " << w.aki_len << "\n";
            if (first) {  // a valid case: a proper prefix of it is valid only where it ends with one of its extensions
                CHECK(w.status == ST_OK);
                std::vector<bool> boundary(b.size() + 1, false);
                for (uint32_t q = 0; q < b.size();) {
                    const Tlv x = read_tlv(Heap{b.data()}, q, (uint32_t)b.size());
                    CHECK(x.ok);
                    if (!x.ok) break;
                    q = x.at + x.len;
                    boundary[q] = true;
                }
                for (size_t len = 1; len < b.size(); len++) CHECK((run_ids(b, len).status == ST_OK) == boundary[len]);
                first = false;
            }
        } else if (kind == "K") {
            Key key[2];
            Bytes bytes[4];
            for (int i = 0; i < 2; i++) {
                std::string name, id;
                ls >> key[i].kind >> key[i].set >> name >> id;
                bytes[2 * i] = unhex(name);
                bytes[2 * i + 1] = unhex(id);
                key[i].name_off = (uint64_t)(2 * i) << 32;
                key[i].id_off = (uint64_t)(2 * i + 1) << 32;
                key[i].name_len = (uint32_t)bytes[2 * i].size();
                key[i].id_len = (uint32_t)bytes[2 * i + 1].size();
            }
            const Block b0(bytes[0].data(), bytes[0].size()), b1(bytes[1].data(), bytes[1].size()), b2(bytes[2].data(), bytes[2].size()),
                b3(bytes[3].data(), bytes[3].size());
            const FourBlocks f{{b0.p, b1.p, b2.p, b3.p}, {bytes[0].size(), bytes[1].size(), bytes[2].size(), bytes[3].size()}};
            g_runs++;
            const bool equal = keys_equal(f, key[0], key[1]);
            CHECK(equal == keys_equal(f, key[1], key[0]) && keys_equal(f, key[0], key[0]));
            const uint64_t h0 = key_hash(f, key[0], S0, S1, 64), h1 = key_hash(f, key[1], S0, S1, 64);
            bool low_bits = true;
            for (int bits = 1; bits < 64; bits++)
                low_bits = low_bits && key_hash(f, key[0], S0, S1, bits) == (h0 & (((uint64_t)1 << bits) - 1));
            out << (equal ? 1 : 0) << " " << (h0 == h1 ? 1 : 0) << " " << (low_bits ? 1 : 0) << "\n";
        } else if (kind == "S") {
            unsigned long long n = 0;
            ls >> n;
            out << table_slots((size_t)n) << " " << scratch_bytes((size_t)n) << "\n";
        } else if (!kind.empty()) {
            std::fprintf(stderr, "unknown case kind %s\n", kind.c_str());
            return 2;
        }
    }
    edges();
    out.close();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("find_plan OK (%ld runs)\n", g_runs);
    return 0;
}
