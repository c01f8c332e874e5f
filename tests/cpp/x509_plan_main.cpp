// The DER walk and the link rule of libmldsa_x509.so (fips204_amd/x509/x509_plan.h) on their own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_x509_cpu.py.  A valid certificate per parameter set is built
// here; every run of the walk reads a heap block of EXACTLY the declared length, so that the sanitizer sees any byte read outside
// [off, off + len).  The walk runs on every prefix 0 ... len of the certificate and on every single-byte change -- to 00, 7F, 80, 81, 84,
// 85 and FF -- of its first 130 bytes and of the 20 bytes around the outer algorithm's and the signature's headers.  Each run must end,
// and its status must be the one a second, plainly written reading of the header's rules (spec_status below, on a bounds-checked vector)
// gives: in particular 0 only where the changed bytes still satisfy the rules.  Then read_tlv's own edges, the link rule and the Name
// comparison.  Exit status 0 and "x509_plan OK".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../fips204_amd/x509/x509_plan.h"

using namespace mldsa_x509;
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

// ---- a certificate of the builder's shape -----------------------------------------------------------------------------------------------
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes out;
    for (const Bytes& p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}
static Bytes tlv(uint8_t tag, const Bytes& content) {
    Bytes out = {tag};
    const size_t n = content.size();
    if (n < 128) out.push_back((uint8_t)n);
    else if (n < 256) out.insert(out.end(), {0x81, (uint8_t)n});
    else out.insert(out.end(), {0x82, (uint8_t)(n >> 8), (uint8_t)n});
    out.insert(out.end(), content.begin(), content.end());
    return out;
}
static Bytes alg_id(int set) {
    return tlv(0x30, {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x03, (uint8_t)(set == 44 ? 0x11 : set == 65 ? 0x12 : 0x13)});
}
static Bytes name(const char* cn) {
    const Bytes s(cn, cn + std::strlen(cn));
    return tlv(0x30, tlv(0x31, tlv(0x30, cat({{0x06, 0x03, 0x55, 0x04, 0x03}, tlv(0x0C, s)}))));
}
static Bytes filled(size_t n, uint8_t seed) {
    Bytes b(n);
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(i * 37 + seed);
    return b;
}
static Bytes bits(const Bytes& content) { return tlv(0x03, cat({{0x00}, content})); }
static Bytes certificate(int set) {
    const int c = class_of_set(set);
    const Bytes date = tlv(0x17, Bytes(13, '1'));
    const Bytes tbs = tlv(0x30, cat({tlv(0xA0, {0x02, 0x01, 0x02}), {0x02, 0x02, 0x12, 0x34}, alg_id(set), name("root"), tlv(0x30, cat({date, date})),
                                     name("leaf"), tlv(0x30, cat({alg_id(set), bits(filled(pk_len(c), 3))}))}));
    return tlv(0x30, cat({tbs, alg_id(set), bits(filled(sig_len(c), 9))}));
}

// ---- the rules read a second time, on a bounds-checked vector ----------------------------------------------------------------------------
struct Bad {};
struct Item {
    uint8_t tag;
    size_t at, end;
};
static Item item(const Bytes& b, size_t pos, size_t end) {
    if (pos + 2 > end) throw Bad();
    Item it = {b.at(pos), 0, 0};
    if ((it.tag & 0x1F) == 0x1F) throw Bad();
    const uint8_t l = b.at(pos + 1);
    size_t n = l, h = 2;
    if (l & 0x80) {
        const size_t k = l & 0x7F;
        if (k < 1 || k > 4 || pos + 2 + k > end) throw Bad();
        n = 0;
        for (size_t j = 0; j < k; j++) n = n * 256 + b.at(pos + 2 + j);
        if (b.at(pos + 2) == 0 || n < 128) throw Bad();
        h += k;
    }
    if (pos + h + n > end) throw Bad();
    it.at = pos + h;
    it.end = pos + h + n;
    return it;
}
static Item tagged(const Bytes& b, size_t pos, size_t end, uint8_t tag) {
    const Item it = item(b, pos, end);
    if (it.tag != tag) throw Bad();
    return it;
}
static int oid_of(const Bytes& b, const Item& it) {
    static const uint8_t head[10] = {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x03};
    if (it.end - it.at != 11 || std::memcmp(&b.at(it.at), head, 10) != 0) return 0;
    const uint8_t x = b.at(it.at + 10);
    return x == 0x11 ? 44 : x == 0x12 ? 65 : x == 0x13 ? 87 : 0;
}
struct Spec {
    int status = ST_DER;
    uint32_t key_set = 0, sig_set = 0;
    size_t tbs = 0, tbs_len = 0, key = 0, sig = 0, issuer = 0, issuer_len = 0, subject = 0, subject_len = 0;
};
static Spec spec_status(const Bytes& b) {
    Spec s;
    try {
        const size_t n = b.size();
        const Item cert = tagged(b, 0, n, 0x30);
        if (cert.end != n) throw Bad();
        const Item tbs = tagged(b, cert.at, n, 0x30), alg = tagged(b, tbs.end, n, 0x30), sig = tagged(b, alg.end, n, 0x03);
        if (sig.end != n) throw Bad();
        size_t pos = tbs.at;
        if (item(b, pos, tbs.end).tag == 0xA0) pos = item(b, pos, tbs.end).end;
        pos = tagged(b, pos, tbs.end, 0x02).end;
        const size_t inner_pos = pos;
        const Item inner = tagged(b, pos, tbs.end, 0x30), issuer = tagged(b, inner.end, tbs.end, 0x30);
        const Item validity = tagged(b, issuer.end, tbs.end, 0x30), subject = tagged(b, validity.end, tbs.end, 0x30);
        const Item spki = tagged(b, subject.end, tbs.end, 0x30), kalg = tagged(b, spki.at, spki.end, 0x30);
        const Item key = tagged(b, kalg.end, spki.end, 0x03);
        if (key.end != spki.end) throw Bad();
        s.tbs = cert.at, s.tbs_len = tbs.end - cert.at, s.issuer = inner.end, s.issuer_len = issuer.end - inner.end;
        s.subject = validity.end, s.subject_len = subject.end - validity.end;
        const int ks = oid_of(b, kalg);
        if (ks && key.end - key.at == 1 + pk_len(class_of_set(ks)) && b.at(key.at) == 0) s.key_set = ks, s.key = key.at + 1;
        s.status = ST_ALG;
        const int ss = oid_of(b, alg);
        if (!ss || inner.end - inner_pos != alg.end - tbs.end || std::memcmp(&b.at(inner_pos), &b.at(tbs.end), alg.end - tbs.end) != 0) return s;
        s.status = ST_SIG;
        if (sig.end - sig.at != 1 + sig_len(class_of_set(ss)) || b.at(sig.at) != 0) return s;
        s.status = ST_OK, s.sig_set = ss, s.sig = sig.at + 1;
    } catch (const Bad&) {
        s = Spec();
    } catch (const std::out_of_range&) {
        std::fprintf(stderr, "spec_status read outside the certificate\n");
        g_fail++;
        s = Spec();
    }
    return s;
}

// ---- the walk on a heap block of exactly len bytes ---------------------------------------------------------------------------------------
struct Heap {
    const uint8_t* p;
    uint32_t operator()(uint64_t pos) const { return p[pos]; }
};
static Walk run_walk(const Bytes& b, size_t len) {
    uint8_t* block = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(block, b.data(), len);
    const Walk w = walk(Heap{block}, (uint32_t)len);
    std::free(block);
    g_runs++;
    return w;
}
static void compare(const Bytes& b) {
    const Walk w = run_walk(b, b.size());
    const Spec s = spec_status(b);
    CHECK(w.status == s.status);
    CHECK(w.key_set == s.key_set && w.sig_set == s.sig_set && w.key_off == s.key && w.sig_off == s.sig);
    CHECK(w.tbs_off == s.tbs && w.tbs_len == s.tbs_len && w.issuer_off == s.issuer && w.issuer_len == s.issuer_len);
    CHECK(w.subject_off == s.subject && w.subject_len == s.subject_len);
    if (w.status == ST_DER) CHECK(w.tbs_off == 0 && w.tbs_len == 0 && w.issuer_len == 0 && w.subject_len == 0 && w.key_set == 0 && w.sig_set == 0);
}

static void one_set(int set) {
    const Bytes good = certificate(set);
    const int c = class_of_set(set);
    const Walk w = run_walk(good, good.size());
    CHECK(w.status == ST_OK && w.sig_set == (uint32_t)set && w.key_set == (uint32_t)set);
    CHECK(w.tbs_off == 4 && w.key_off == 118 && w.sig_off == 118 + pk_len(c) + 13 + 5 && w.sig_off + sig_len(c) == good.size());
    CHECK(w.issuer_off == 30 && w.issuer_len == 17 && w.subject_off == 79 && w.subject_len == 17);
    compare(good);
    // every proper prefix of at least 2 bytes is malformed (shorter ones the range rule refuses before the walk)
    for (size_t len = 2; len < good.size(); len++) CHECK(run_walk(good, len).status == ST_DER);
    // single-byte changes: the head, and the bytes around the outer algorithm's and the signature's headers
    std::vector<size_t> at;
    for (size_t p = 0; p < 130; p++) at.push_back(p);
    const size_t outer = w.tbs_off + w.tbs_len;  // the outer AlgorithmIdentifier begins here; the BIT STRING 13 bytes on
    for (size_t p = outer - 3; p < outer + 17; p++) at.push_back(p);
    const uint8_t values[7] = {0x00, 0x7F, 0x80, 0x81, 0x84, 0x85, 0xFF};
    long accepted = 0;
    for (size_t p : at)
        for (uint8_t v : values) {
            Bytes b = good;
            b[p] = v;
            compare(b);
            accepted += run_walk(b, b.size()).status == ST_OK;
        }
    // what is still accepted: changes of content the walk does not look into (the version, the serial, the dates, the inside of the Names,
    // the key).  Never a change of the Certificate's or the TBS's header (8 bytes) or of the inner or outer algorithm TLV (13 bytes each).
    CHECK(accepted > 0 && accepted <= ((long)at.size() - 34) * 7);
}

static void tlv_edges() {
    const auto rd = [](const Bytes& b, uint32_t pos, uint32_t end) { return read_tlv(Heap{b.data()}, pos, end); };
    CHECK(!rd({0x30}, 0, 1).ok && !rd({0x30, 0x00}, 1, 2).ok && !rd({0x30, 0x00}, 2, 2).ok && !rd({0x30, 0x00}, 3, 2).ok);
    CHECK(rd({0x30, 0x00}, 0, 2).ok && rd({0x30, 0x00}, 0, 2).len == 0 && rd({0x30, 0x00}, 0, 2).at == 2);
    CHECK(!rd({0x1F, 0x00}, 0, 2).ok && !rd({0xFF, 0x00}, 0, 2).ok && !rd({0x30, 0x80}, 0, 2).ok && !rd({0x30, 0x01}, 0, 2).ok);
    CHECK(!rd({0x30, 0x81}, 0, 2).ok && !rd({0x30, 0x81, 0x7F}, 0, 3).ok && !rd({0x30, 0x82, 0x00, 0xFF}, 0, 4).ok);
    CHECK(!rd({0x30, 0x85, 1, 0, 0, 0, 0}, 0, 7).ok && !rd({0x30, 0xFF, 1, 0, 0, 0, 0}, 0, 7).ok);
    CHECK(!rd({0x30, 0x84, 0xFF, 0xFF, 0xFF, 0xFF}, 0, 6).ok && !rd({0x30, 0x84, 0x01, 0x00, 0x00, 0x00}, 0, 6).ok);  // nothing wraps
    CHECK(!rd({0x30, 0x84, 0x00, 0x01, 0x00, 0x00}, 0, 6).ok && !rd({0x30, 0x83, 0x01, 0x00}, 0, 4).ok);
    Bytes b = {0x04, 0x81, 0x80};
    b.resize(3 + 128, 7);
    CHECK(rd(b, 0, (uint32_t)b.size()).ok && rd(b, 0, (uint32_t)b.size()).len == 128 && !rd(b, 0, (uint32_t)b.size() - 1).ok);
}

// same_alg on a heap block of exactly the two contents: equal, and unequal in each of the OID_LEN bytes in turn, first and last included
static void same_alg_edges() {
    for (int c = 0; c < 3; c++) {
        uint8_t* block = static_cast<uint8_t*>(std::malloc(2 * OID_LEN));
        const uint8_t oid[OID_LEN] = {0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x03, (uint8_t)(0x11 + c)};
        std::memcpy(block, oid, OID_LEN);
        std::memcpy(block + OID_LEN, oid, OID_LEN);
        const Heap f{block};
        CHECK(same_alg(f, 0, OID_LEN) && same_alg(f, OID_LEN, 0) && same_alg(f, 0, 0) && same_alg(f, OID_LEN, OID_LEN));
        for (uint32_t j = 0; j < OID_LEN; j++)
            for (uint8_t flip : {0x01, 0x80, 0xFF}) {
                block[OID_LEN + j] ^= flip;
                CHECK(!same_alg(f, 0, OID_LEN) && !same_alg(f, OID_LEN, 0) && same_alg(f, OID_LEN, OID_LEN));
                block[OID_LEN + j] ^= flip;
            }
        CHECK(same_alg(f, 0, OID_LEN));
        std::free(block);
    }
}

static void link_and_names() {
    const uint64_t n = 10;
    // the rules a CRL shares: the certificate's without its "no issuer" case, at the caps' edge too
    CHECK(signer_status(ST_OK, 44, NO_ISSUER, n, 0, 0) == ST_ISSUER && signer_status(ST_OK, 44, NO_ISSUER, (uint64_t)1 << 30, 0, 0) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, NO_ISSUER, (uint64_t)1 << 30, 0, 0) == ST_PARSE_ONLY && signer_status(ST_SIG, 0, NO_ISSUER, n, 0, 0) == ST_SIG);
    for (uint32_t issuer : {0u, 3u, 9u, 10u, 0xFFFFFFFEu})
        for (int ist : {ST_OK, ST_RANGE, ST_DER, ST_ALG, ST_PARSE_ONLY})
            for (uint32_t ks : {0u, 44u, 65u})
                for (int own : {ST_OK, ST_DER, ST_SIG}) CHECK(signer_status(own, 44, issuer, n, ist, ks) == link_status(own, 44, issuer, n, ist, ks));
    CHECK(link_status(ST_DER, 0, 3, n, ST_OK, 44) == ST_DER && link_status(ST_SIG, 0, NO_ISSUER, n, 0, 0) == ST_SIG);
    CHECK(link_status(ST_OK, 44, NO_ISSUER, n, 0, 0) == ST_PARSE_ONLY && link_status(ST_OK, 44, 10, n, 0, 0) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 0xFFFFFFFEu, n, 0, 0) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 3, n, ST_RANGE, 44) == ST_ISSUER && link_status(ST_OK, 44, 3, n, ST_DER, 44) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 3, n, ST_OK, 0) == ST_ISSUER && link_status(ST_OK, 44, 3, n, ST_OK, 65) == ST_ISSUER);
    CHECK(link_status(ST_OK, 44, 3, n, ST_ALG, 44) == ST_OK && link_status(ST_OK, 87, 3, n, ST_SIG, 87) == ST_OK);
    CHECK(link_status(ST_OK, 65, 9, n, ST_OK, 65) == ST_OK);
    // the Names: a heap block of exactly the bytes, compared at its very ends
    for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 300u}) {
        uint8_t* block = static_cast<uint8_t*>(std::malloc(2 * len + 1));
        for (uint32_t i = 0; i < len; i++) block[i] = block[len + 1 + i] = (uint8_t)(i * 5 + 1);
        block[len] = 0xEE;
        const Heap f{block};
        CHECK(!names_differ(f, 0, len, len + 1, len));
        CHECK(names_differ(f, 0, len, len + 1, len + 1));
        if (len) {
            block[2 * len] ^= 1;  // the last byte
            CHECK(names_differ(f, 0, len, len + 1, len));
            uint32_t lanes = 0;
            for (uint32_t idx = 0; idx < (len + 63) / 64 * 64; idx++) lanes |= name_byte_diff(f, 0, len + 1, len, idx);  // as the wave steps
            CHECK(lanes == 1);
        }
        std::free(block);
    }
}

int main() {
    for (int set : {44, 65, 87}) one_set(set);
    tlv_edges();
    same_alg_edges();
    link_and_names();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("x509_plan OK (%ld walks)\n", g_runs);
    return 0;
}
