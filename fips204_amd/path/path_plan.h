// The pure arithmetic of libmldsa_path.so (include/mldsa_path.h): the Time reader, the walk behind the subjectPublicKeyInfo of one X.509
// Certificate, the rules of a node, the climb to a trust anchor, the freshness rule of a CRL and the row layouts.  No HIP here: every
// function is constexpr and takes bytes through a fetch functor f(pos) -> byte pos of the certificate (or of a Time's surroundings),
// so the kernels of path.hip call these very functions on the blob and tests/cpp/path_plan_main.cpp compiles the file alone, under
// the sanitizers, on a heap block of exactly len bytes.  The DER reader and the range check are those of ../x509/x509_plan.h and
// ../rec/rec_plan.h, included and not copied.
//
// Positions are relative to the functor's first byte and 32 bits wide.  No function fetches a position at or behind the `end` it was
// given.  walk_policy is a fixed sequence of read_tlv steps and one loop bounded by MAX_EXTS; climb is one loop bounded by MAX_DEPTH.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../x509/x509_plan.h"

namespace mldsa_path {

using mldsa_rec::in_range;
using mldsa_x509::NO_ISSUER;
using mldsa_x509::read_tlv;
using mldsa_x509::Tlv;

// the codes, flags and caps of include/mldsa_path.h (path.hip asserts the equality)
constexpr int ST_OK = 0, ST_RANGE = 1, ST_DER = 2, ST_VERSION = 22, ST_TIME = 23, ST_EXT = 24, ST_CRITICAL = 25;
constexpr uint32_t FLAG_ALLOW_UNKNOWN_CRITICAL = 1, FLAG_REQUIRE_NEXT_UPDATE = 2, FLAG_ALLOW_NO_CRL = 4;
constexpr uint32_t F_V3 = 1, F_HAS_BC = 2, F_IS_CA = 4, F_HAS_KU = 8;
constexpr uint32_t MAX_EXTS = 32, MAX_DEPTH = 16, NO_PATH_LEN = 0xFFFFFFFFu;
constexpr uint64_t MAX_CERTS = 1u << 30;
constexpr int V_TRUSTED = 0, V_CERT = 1, V_SIG = 2, V_POLICY = 3, V_NOT_YET = 4, V_EXPIRED = 5, V_REVOKED = 6, V_REVOCATION = 7, V_NOT_CA = 8,
              V_KEY_USAGE = 9, V_PATH_LEN = 10, V_NO_ANCHOR = 11, V_DEPTH = 12;
constexpr int CRL_FRESH = 0, CRL_REFUSED = 1, CRL_TIME = 2, CRL_NOT_YET = 3, CRL_STALE = 4;
constexpr int REV_GOOD = 0, REV_REVOKED = 1, REV_NO_CRL = 2;  // the answers of include/mldsa_crl.h that the node rule names
constexpr uint32_t KU_KEY_CERT_SIGN = 1u << 5;
constexpr uint32_t TIME_TLV_MAX = 17;  // 18 0F and 15 bytes: no Time is longer, so a reader bounded by this many bytes misses nothing

// the row layouts (path.hip asserts them against the structs of the header)
constexpr size_t FIELDS_BYTES = 48, FIELDS_NOT_AFTER = 8, FIELDS_EXT_OFF = 16, FIELDS_CRIT_OFF = 24, FIELDS_EXT_LEN = 32, FIELDS_PATH_LEN = 36,
                 FIELDS_KEY_USAGE = 40, FIELDS_FLAGS = 42, FIELDS_N_EXT = 43, FIELDS_STATUS = 44;
constexpr size_t RESULT_BYTES = 8, RESULT_VERDICT = 4, RESULT_DEPTH = 5, NODE_BYTES = 8;
static_assert(FIELDS_STATUS + 1 + 3 == FIELDS_BYTES && RESULT_DEPTH + 1 + 2 == RESULT_BYTES, "the rows end with their reserved bytes");

constexpr size_t scratch_bytes(size_t n) { return n > MAX_CERTS ? 0 : (NODE_BYTES * n + 255) / 256 * 256; }

// ---- one Time ---------------------------------------------------------------------------------------------------------------------------
struct Time {
    bool ok = false;
    int64_t seconds = 0;
    uint32_t next = 0;  // the position behind the TLV
};

// days from 1970-01-01 to y-m-d of the proleptic Gregorian calendar, 1 <= m <= 12: the years are counted from 1 March, so that the
// leap day is a year's last, in eras of 400 years
constexpr int64_t days_from_civil(int64_t y, uint32_t m, uint32_t d) {
    y -= m <= 2 ? 1 : 0;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const uint32_t yoe = (uint32_t)(y - era * 400);
    const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
    const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + (int64_t)doe - 719468;
}

constexpr bool leap_year(uint32_t y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }

// 31 for January, March, May, July, August, October and December: the parity flips behind July
constexpr uint32_t days_in_month(uint32_t y, uint32_t m) { return m == 2 ? (leap_year(y) ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u); }

// the two decimal digits at pos; bad is set where either is none
template <class Fetch>
constexpr uint32_t two_digits(const Fetch& f, uint32_t pos, bool& bad) {
    const uint32_t a = f(pos) - 0x30u, b = f(pos + 1) - 0x30u;
    if (a > 9 || b > 9) bad = true;
    return a * 10 + b;
}

// The Time TLV at pos inside [pos, end): the rules of the header.
template <class Fetch>
constexpr Time parse_time(const Fetch& f, uint32_t pos, uint32_t end) {
    Time out;
    const Tlv t = read_tlv(f, pos, end);
    if (!t.ok) return out;
    const bool utc = t.tag == 0x17 && t.len == 13, generalized = t.tag == 0x18 && t.len == 15;
    if (!utc && !generalized) return out;
    bool bad = false;
    uint32_t p = t.at, year = 0;
    if (generalized) {
        year = 100 * two_digits(f, p, bad);
        p += 2;
    }
    const uint32_t yy = two_digits(f, p, bad);
    year = generalized ? year + yy : (yy < 50 ? 2000 + yy : 1900 + yy);
    const uint32_t month = two_digits(f, p + 2, bad), day = two_digits(f, p + 4, bad), hour = two_digits(f, p + 6, bad);
    const uint32_t minute = two_digits(f, p + 8, bad), second = two_digits(f, p + 10, bad);
    if (bad || f(p + 12) != 0x5A) return out;
    if (year < 1 || month < 1 || month > 12 || day < 1 || day > days_in_month(year, month) || hour > 23 || minute > 59 || second > 59) return out;
    out.ok = true;
    out.seconds = days_from_civil(year, month, day) * 86400 + (int64_t)(hour * 3600 + minute * 60 + second);
    out.next = t.at + t.len;
    return out;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------
// What the walk finds, relative to the certificate.  A status of ST_DER leaves everything else 0.
struct Policy {
    int64_t not_before = 0, not_after = 0;
    uint32_t ext_off = 0, ext_len = 0, crit_off = 0, path_len = 0, key_usage = 0, flags = 0, n_ext = 0, n_crit = 0;
    int status = ST_DER;
};

// the content of a basicConstraints extnValue, [pos, end)
struct Basic {
    bool ok = false, ca = false;
    uint32_t path_len = NO_PATH_LEN;
};

template <class Fetch>
constexpr Basic basic_constraints(const Fetch& f, uint32_t pos, uint32_t end) {
    Basic out;
    const Tlv seq = read_tlv(f, pos, end);
    if (!seq.ok || seq.tag != 0x30 || seq.at + seq.len != end) return out;
    uint32_t p = seq.at;
    bool ca = false;
    uint32_t path_len = NO_PATH_LEN;
    if (p < end) {
        Tlv t = read_tlv(f, p, end);
        if (!t.ok) return out;
        if (t.tag == 0x01) {
            if (t.len != 1 || f(t.at) != 0xFF) return out;
            ca = true;
            p = t.at + t.len;
            if (p < end) {
                t = read_tlv(f, p, end);
                if (!t.ok) return out;
            }
        }
        if (p < end) {
            if (t.tag != 0x02 || t.len < 1 || t.len > 4 || !ca) return out;
            const uint32_t first = f(t.at);
            if (first >= 0x80) return out;                             // negative
            if (t.len > 1 && first == 0 && f(t.at + 1) < 0x80) return out;  // a leading 00 the value does not need
            path_len = 0;
            for (uint32_t j = 0; j < 4; ++j)
                if (j < t.len) path_len = (path_len << 8) | f(t.at + j);
            p = t.at + t.len;
        }
    }
    if (p != end) return out;
    out.ok = true;
    out.ca = ca;
    out.path_len = path_len;
    return out;
}

// the eight bits of a byte in the opposite order: KeyUsage bit 0 is the first byte's highest
constexpr uint32_t reversed8(uint32_t b) {
    b = ((b & 0xF0) >> 4) | ((b & 0x0F) << 4);
    b = ((b & 0xCC) >> 2) | ((b & 0x33) << 2);
    return ((b & 0xAA) >> 1) | ((b & 0x55) << 1);
}

// the content of a keyUsage extnValue, [pos, end): bits = 0 where it is refused (an accepted one has a bit set)
template <class Fetch>
constexpr uint32_t key_usage_bits(const Fetch& f, uint32_t pos, uint32_t end) {
    const Tlv bs = read_tlv(f, pos, end);
    if (!bs.ok || bs.tag != 0x03 || bs.at + bs.len != end || bs.len < 2 || bs.len > 3) return 0;
    const uint32_t unused = f(bs.at), b0 = f(bs.at + 1), b1 = bs.len == 3 ? f(bs.at + 2) : 0;
    if (unused > 7) return 0;
    const uint32_t last = bs.len == 3 ? b1 : b0;
    if ((last & ((1u << unused) - 1)) != 0 || ((last >> unused) & 1) == 0) return 0;
    return reversed8(b0) | reversed8(b1) << 8;
}

// The certificate's len bytes (2 <= len: the caller's range check); flags: FLAG_ALLOW_UNKNOWN_CRITICAL.  The whole path is walked for
// its structure; then the first class broken of VERSION, TIME, EXT, CRITICAL is the status.
template <class Fetch>
constexpr Policy walk_policy(const Fetch& f, uint32_t len, uint32_t flags) {
    const Policy der;  // what every structural refusal returns
    // 1. ... 3. of mldsa_x509::walk, the [0] looked into on the way
    const Tlv cert = read_tlv(f, 0, len);
    if (!cert.ok || cert.tag != 0x30 || cert.at + cert.len != len) return der;
    const Tlv tbs = read_tlv(f, cert.at, len);
    if (!tbs.ok || tbs.tag != 0x30) return der;
    const Tlv alg = read_tlv(f, tbs.at + tbs.len, len);
    if (!alg.ok || alg.tag != 0x30) return der;
    const Tlv sig = read_tlv(f, alg.at + alg.len, len);
    if (!sig.ok || sig.tag != 0x03 || sig.at + sig.len != len) return der;
    const uint32_t tend = tbs.at + tbs.len;
    bool bad_version = false, bad_ext = false;
    uint32_t version = 1;
    Tlv t = read_tlv(f, tbs.at, tend);
    if (t.ok && t.tag == 0xA0) {
        if (t.len == 3 && f(t.at) == 0x02 && f(t.at + 1) == 0x01 && (f(t.at + 2) == 1 || f(t.at + 2) == 2)) version = f(t.at + 2) + 1;
        else bad_version = true;
        t = read_tlv(f, t.at + t.len, tend);
    }
    if (!t.ok || t.tag != 0x02) return der;
    const Tlv inner = read_tlv(f, t.at + t.len, tend);
    if (!inner.ok || inner.tag != 0x30) return der;
    const Tlv issuer = read_tlv(f, inner.at + inner.len, tend);
    if (!issuer.ok || issuer.tag != 0x30) return der;
    const Tlv validity = read_tlv(f, issuer.at + issuer.len, tend);
    if (!validity.ok || validity.tag != 0x30) return der;
    const Tlv subject = read_tlv(f, validity.at + validity.len, tend);
    if (!subject.ok || subject.tag != 0x30) return der;
    const Tlv spki = read_tlv(f, subject.at + subject.len, tend);
    if (!spki.ok || spki.tag != 0x30) return der;
    const uint32_t send = spki.at + spki.len;
    const Tlv kalg = read_tlv(f, spki.at, send);
    if (!kalg.ok || kalg.tag != 0x30) return der;
    const Tlv key = read_tlv(f, kalg.at + kalg.len, send);
    if (!key.ok || key.tag != 0x03 || key.at + key.len != send) return der;

    Policy p;
    p.path_len = NO_PATH_LEN;
    // 4. behind the SPKI: unique IDs, extensions, the TBS's end
    uint32_t pos = send;
    bool more = pos < tend, has_uid = false, has_ext = false;
    Tlv exts;  // the Extensions SEQUENCE
    if (more) {
        t = read_tlv(f, pos, tend);
        if (!t.ok) return der;
    }
    for (uint32_t tag = 0x81; tag <= 0x82; ++tag)
        if (more && t.tag == tag) {
            has_uid = true;
            pos = t.at + t.len;
            more = pos < tend;
            if (more) {
                t = read_tlv(f, pos, tend);
                if (!t.ok) return der;
            }
        }
    if (more) {
        if (t.tag != 0xA3) return der;
        exts = read_tlv(f, t.at, t.at + t.len);
        if (!exts.ok || exts.tag != 0x30 || exts.at + exts.len != t.at + t.len) return der;
        has_ext = true;
        pos = t.at + t.len;
    }
    if (pos != tend) return der;
    if ((has_uid && version < 2) || (has_ext && version < 3)) bad_version = true;
    // 5. ... 7. the extensions: the frames in the loop, the two values this library reads behind it, once each
    uint32_t bc_at = 0, bc_end = 0, ku_at = 0, ku_end = 0;
    bool bad_der = false;
    if (has_ext) {
        const uint32_t eend = exts.at + exts.len;
        uint32_t q = exts.at;
        p.ext_off = exts.at;
        p.ext_len = exts.len;
        if (q == eend) bad_ext = true;
        for (uint32_t k = 0; k < MAX_EXTS && q < eend && !bad_der; ++k) {  // MAX_EXTS rounds at most, whatever the data says
            const Tlv x = read_tlv(f, q, eend);
            const uint32_t xend = x.at + x.len;
            const Tlv oid = read_tlv(f, x.at, xend);
            Tlv v = read_tlv(f, oid.at + oid.len, xend);
            bool framed = x.ok && x.tag == 0x30 && oid.ok && oid.tag == 0x06 && v.ok;
            bool critical = false;
            if (framed && v.tag == 0x01) {
                if (v.len == 1 && f(v.at) == 0xFF) critical = true;
                else bad_ext = true;
                v = read_tlv(f, v.at + v.len, xend);
            }
            framed = framed && v.ok && v.tag == 0x04 && v.at + v.len == xend;
            if (!framed) {
                bad_der = true;
            } else {
                const bool id_ce = oid.len == 3 && f(oid.at) == 0x55 && f(oid.at + 1) == 0x1D;
                const uint32_t arc = id_ce ? f(oid.at + 2) : 0;
                if (arc == 0x13) {
                    if (bc_end != 0) bad_ext = true;  // twice
                    else bc_at = v.at, bc_end = xend;
                } else if (arc == 0x0F) {
                    if (ku_end != 0) bad_ext = true;
                    else ku_at = v.at, ku_end = xend;
                } else if (critical) {
                    if (p.n_crit == 0) p.crit_off = q;
                    ++p.n_crit;
                }
                ++p.n_ext;
                q = xend;
            }
        }
        if (bad_der) return der;
        if (q != eend) bad_ext = true;  // more than MAX_EXTS extensions
    }
    if (bc_end != 0) {
        const Basic b = basic_constraints(f, bc_at, bc_end);
        if (!b.ok) {
            bad_ext = true;
        } else {
            p.flags |= F_HAS_BC | (b.ca ? F_IS_CA : 0);
            p.path_len = b.path_len;
        }
    }
    if (ku_end != 0) {
        const uint32_t bits = key_usage_bits(f, ku_at, ku_end);
        if (bits == 0) {
            bad_ext = true;
        } else {
            p.flags |= F_HAS_KU;
            p.key_usage = bits;
        }
    }
    // 3. the validity
    const uint32_t vend = validity.at + validity.len;
    const Time nb = parse_time(f, validity.at, vend);
    Time na;
    if (nb.ok) na = parse_time(f, nb.next, vend);
    const bool bad_time = !(nb.ok && na.ok && na.next == vend);
    if (!bad_time) {
        p.not_before = nb.seconds;
        p.not_after = na.seconds;
    }
    if (!bad_version && version == 3) p.flags |= F_V3;
    p.status = bad_version ? ST_VERSION
               : bad_time  ? ST_TIME
               : bad_ext   ? ST_EXT
               : (p.n_crit != 0 && (flags & FLAG_ALLOW_UNKNOWN_CRITICAL) == 0) ? ST_CRITICAL
                                                                              : ST_OK;
    return p;
}

// ---- the node and the climb -------------------------------------------------------------------------------------------------------------
// the first rule a certificate breaks for itself, or 0
constexpr int own_rule(int cert_status, bool cert_ok, int policy_status, int64_t not_before, int64_t not_after, bool has_revocation, int revocation,
                       int64_t now, uint32_t flags) {
    if (cert_status != 0) return V_CERT;
    if (!cert_ok) return V_SIG;
    if (policy_status != ST_OK) return V_POLICY;
    if (now < not_before) return V_NOT_YET;
    if (now > not_after) return V_EXPIRED;
    if (!has_revocation) return 0;
    if (revocation == REV_REVOKED) return V_REVOKED;
    if (revocation == REV_GOOD || (revocation == REV_NO_CRL && (flags & FLAG_ALLOW_NO_CRL) != 0)) return 0;
    return V_REVOCATION;
}

// the first rule it breaks as somebody's issuer, or 0
constexpr int issuer_rule(uint32_t policy_flags, uint32_t key_usage) {
    const uint32_t ca = F_V3 | F_HAS_BC | F_IS_CA;
    if ((policy_flags & ca) != ca) return V_NOT_CA;
    if ((policy_flags & F_HAS_KU) != 0 && (key_usage & KU_KEY_CERT_SIGN) == 0) return V_KEY_USAGE;
    return 0;
}

struct Node {
    uint32_t issuer = 0, own = 0, as_issuer = 0, path_len = 255, anchor = 0;
};

constexpr Node node_of(uint32_t issuer, int own, int as_issuer, uint32_t path_len, bool anchor) {
    Node nd;
    nd.issuer = issuer;
    nd.own = (uint32_t)own;
    nd.as_issuer = (uint32_t)as_issuer;
    nd.path_len = path_len == NO_PATH_LEN ? 255u : path_len > 254 ? 254u : path_len;
    nd.anchor = anchor ? 1 : 0;
    return nd;
}

// the node as its 8 bytes, little-endian: {uint32 issuer; uint8 own; uint8 as_issuer; uint8 path_len; uint8 anchor}
constexpr uint64_t pack_node(const Node& nd) {
    return nd.issuer | (uint64_t)nd.own << 32 | (uint64_t)nd.as_issuer << 40 | (uint64_t)nd.path_len << 48 | (uint64_t)nd.anchor << 56;
}

constexpr Node unpack_node(uint64_t w) {
    Node nd;
    nd.issuer = (uint32_t)w;
    nd.own = (uint32_t)(w >> 32) & 0xFF;
    nd.as_issuer = (uint32_t)(w >> 40) & 0xFF;
    nd.path_len = (uint32_t)(w >> 48) & 0xFF;
    nd.anchor = (uint32_t)(w >> 56) & 0xFF;
    return nd;
}

struct Result {
    int verdict = V_DEPTH;
    uint32_t where = 0, depth = 0;
};

// The climb from certificate i < n; g(a) is the packed node of certificate a < n.  MAX_DEPTH + 1 rounds at most.
template <class Nodes>
constexpr Result climb(const Nodes& g, uint32_t i, uint32_t n) {
    Result r;
    uint32_t a = i;
    for (uint32_t k = 0; k <= MAX_DEPTH; ++k) {
        const Node nd = unpack_node(g(a));
        r.where = a;
        r.depth = k;
        if (nd.anchor != 0) {
            r.verdict = V_TRUSTED;
            return r;
        }
        const int broken = nd.own != 0 ? (int)nd.own
                           : k >= 1 && nd.as_issuer != 0 ? (int)nd.as_issuer
                           : k >= 1 && nd.path_len != 255 && k - 1 > nd.path_len ? V_PATH_LEN
                                                                                  : 0;
        if (broken != 0) {
            r.verdict = broken;
            return r;
        }
        if (nd.issuer == NO_ISSUER || nd.issuer >= n || nd.issuer == a) {
            r.verdict = V_NO_ANCHOR;
            return r;
        }
        if (k + 1 > MAX_DEPTH) break;
        a = nd.issuer;
    }
    r.verdict = V_DEPTH;
    return r;
}

// ---- the freshness of a CRL -------------------------------------------------------------------------------------------------------------
// accepted: the CRL's status and its row's are OK; times_ok: thisUpdate was read, and nextUpdate too where there is one
constexpr int crl_time_status(bool accepted, bool times_ok, int64_t this_s, bool has_next, int64_t next_s, int64_t now, uint32_t flags) {
    if (!accepted) return CRL_REFUSED;
    if (!times_ok) return CRL_TIME;
    if (now < this_s) return CRL_NOT_YET;
    if (has_next ? now > next_s : (flags & FLAG_REQUIRE_NEXT_UPDATE) != 0) return CRL_STALE;
    return CRL_FRESH;
}

}  // namespace mldsa_path
