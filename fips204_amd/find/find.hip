// libmldsa_find.so (include/mldsa_find.h): the issuer of every certificate and of every CRL, and the CRL of every certificate, found
// among an unordered bag of certificates -- the front of X.509 path validation.  This library links and calls none of the other
// layers; it reads the rows that libmldsa_x509.so, libmldsa_crl.so and libmldsa_path.so wrote.
//
// Seven kernels; those of one call are ordered by the kernel boundary alone: no wave waits for another.
//   k_find_ids          one certificate per lane: walk_ids of find_plan.h over the extensions range of its policy row.
//   k_find_claim        one certificate per wave: the hashes of its two keys, 64 bytes per step, and a slot for each by atomicCAS.
//   k_find_confirm      one certificate per wave: each entry against its slot's owner, into the group or onto the overflow list.
//   k_find_issuers      one certificate per wave: one or two lookups, every answer confirmed byte for byte.
//   k_find_crl_issuers  one CRL per wave: the same lookups from the CRL's row and the authorityKeyIdentifier of its extensions.
//   k_find_ca_min       one CRL per lane: an atomicMin on its CA's word.
//   k_find_cert_crl     one certificate per lane: its CA's word.
// Every lane of a wave reads the same rows and derives the same key, so control flow is uniform in the wave; the Names are read one
// byte per lane at any alignment of the blob, as k_x509_link reads them.  What bounds them: the dependent loads of the walks, and
// in the claim the atomics on the table; the batch counters are summed per workgroup in LDS first.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/mldsa_find.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"
#include "../x509/x509_dev.h"
#include "find_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_find;
using mldsa_x509::BlobBytes;

static_assert(sizeof(mldsa_find_id) == ID_BYTES && offsetof(mldsa_find_id, aki_off) == ID_AKI_OFF && offsetof(mldsa_find_id, ski_len) == ID_SKI_LEN &&
                  offsetof(mldsa_find_id, aki_len) == ID_AKI_LEN && offsetof(mldsa_find_id, status) == ID_STATUS &&
                  sizeof(mldsa_find_result) == RESULT_BYTES && offsetof(mldsa_find_result, candidates) == RESULT_CANDIDATES &&
                  offsetof(mldsa_find_result, status) == RESULT_STATUS && sizeof(mldsa_find_totals) == TOTALS_BYTES &&
                  sizeof(mldsa_x509_cert) == 16 && sizeof(mldsa_crl_item) == 16 && sizeof(mldsa_x509_fields) == 56 && sizeof(mldsa_crl_fields) == 88 &&
                  sizeof(mldsa_path_fields) == 48,
              "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_ALG == MLDSA_X509_ALG &&
                  ST_SIG == MLDSA_X509_SIG && ST_EXT == MLDSA_FIND_EXT && MLDSA_FIND_EXT > MLDSA_PATH_CRITICAL,
              "the status codes of include/mldsa_find.h and include/mldsa_x509.h");
static_assert(R_FOUND == MLDSA_FIND_FOUND && R_NONE == MLDSA_FIND_NONE && R_CERT == MLDSA_FIND_CERT && R_SPACE == MLDSA_FIND_SPACE,
              "the answers of include/mldsa_find.h");
static_assert(MAX_EXTS == MLDSA_PATH_MAX_EXTS && MAX_KEYID == MLDSA_FIND_MAX_KEYID && PROBE_MAX == MLDSA_FIND_PROBE_MAX &&
                  OVERFLOW_MAX == MLDSA_FIND_OVERFLOW_MAX && MAX_CERTS == MLDSA_FIND_MAX_CERTS && MAX_CERTS <= MLDSA_X509_MAX_CERTS &&
                  NO_ISSUER == MLDSA_X509_NO_ISSUER && CRL_NONE == MLDSA_CRL_NONE && MAX_KEYID <= 64 && 8 * MAX_CERTS <= 0x80000000ull,
              "the caps of include/mldsa_find.h; an identifier is one 64-byte step; slots and entries are 32 bits wide");

constexpr int IDS_BLOCK = 256;  // items per workgroup of the lane-per-item kernels
constexpr int WAVES = 4;        // items per workgroup of the wave-per-item kernels

// the rows of the certificates, as every kernel behind k_find_ids takes them
struct Certs {
    const mldsa_x509_cert* certs;
    const mldsa_x509_fields* fields;
    const mldsa_find_id* ids;
    uint32_t n;
    uint64_t blob_len;
};

// the table, in scratch
struct Table {
    const unsigned long long* tags;
    const uint32_t* owners;
    const uint32_t* counts;
    const uint32_t* overflow;
    const Key* keys;  // entry e's key as k_find_claim made it from the rows, every range checked: the rows are not read again
    uint32_t mask;
};

struct Seed {
    uint64_t s0, s1;
    int hash_bits;
};

// Key k (0: ANY; 1: SKI or NOSKI) of certificate j < n, where j is a candidate: every range checked before it is followed.
__device__ __forceinline__ bool candidate_key(const Certs& C, uint32_t j, uint32_t k, Key* out) {
    const mldsa_x509_cert c = C.certs[j];
    const mldsa_x509_fields& f = C.fields[j];
    const mldsa_find_id d = C.ids[j];
    if (!candidate_row(f.status, f.key_set, d.status) || !in_range(c.off, c.len, C.blob_len)) return false;
    if (!inside(f.subject_off, f.subject_len, c.off, c.len)) return false;
    if (d.ski_len != 0 && (d.ski_len > MAX_KEYID || !inside(d.ski_off, d.ski_len, c.off, c.len))) return false;
    const bool has_ski = k != 0 && d.ski_len != 0;
    out->name_off = f.subject_off;
    out->name_len = f.subject_len;
    out->set = f.key_set;
    out->kind = k == 0 ? KIND_ANY : has_ski ? KIND_SKI : KIND_NOSKI;
    out->id_off = has_ski ? d.ski_off : 0;
    out->id_len = has_ski ? d.ski_len : 0u;
    return true;
}

// key_hash of find_plan.h, the same value in every lane: lane l adds the bytes l, l + 64, ...
__device__ __forceinline__ uint64_t wave_hash(const uint8_t* __restrict__ blob, const Key& k, int lane, const Seed& sd) {
    const BlobBytes f{blob};
    uint64_t sum = 0;
    for (uint64_t idx = lane; idx < k.name_len; idx += 64) sum += byte_term(sd.s0, idx, f(k.name_off + idx));
    if ((uint32_t)lane < k.id_len) sum += byte_term(sd.s0, (uint64_t)k.name_len + lane, f(k.id_off + lane));
    return finish_hash(wave_sum(sum), k, sd.s1, sd.hash_bits);
}

// keys_equal of find_plan.h, the same value in every lane, 64 bytes per step
__device__ __forceinline__ bool wave_equal(const uint8_t* __restrict__ blob, const Key& a, const Key& b, int lane) {
    if (!same_shape(a, b)) return false;
    const BlobBytes f{blob};
    const uint64_t total = (uint64_t)a.name_len + a.id_len;
    uint32_t diff = 0;
    for (uint64_t base = 0; base < total; base += 64) diff |= key_byte_diff(f, a, b, base + lane);
    return wave_or(diff) == 0;
}

// One lookup: the rule of the header.  Every probe loop is bounded by PROBE_MAX, the scan by OVERFLOW_MAX.
__device__ __forceinline__ Match lookup(const uint8_t* __restrict__ blob, const Certs& C, const Table& T, uint32_t n_overflow, const Key& key,
                                        int lane, const Seed& sd) {
    Match m;
    const uint64_t h = wave_hash(blob, key, lane, sd);
    uint32_t slot = NO_SLOT;
    for (uint32_t p = 0; p < PROBE_MAX; ++p) {
        const uint32_t s = (uint32_t)(h + p) & T.mask;
        const uint64_t t = T.tags[s];
        if (t == h) slot = s;
        if (t == h || t == EMPTY_TAG) break;
    }
    if (slot != NO_SLOT) {
        const uint32_t e = T.owners[slot];
        if (e < 2 * C.n && wave_equal(blob, key, T.keys[e], lane)) {
            m.lowest = e >> 1;
            m.count = T.counts[slot];
            return m;
        }
    }
    if (n_overflow == 0) return m;
    if (n_overflow > OVERFLOW_MAX) {
        m.space = true;
        return m;
    }
    for (uint32_t q = 0; q < n_overflow; ++q) {
        const uint32_t e = T.overflow[q];
        if (e < 2 * C.n && wave_equal(blob, key, T.keys[e], lane)) {
            ++m.count;
            m.lowest = (e >> 1) < m.lowest ? (e >> 1) : m.lowest;
        }
    }
    return m;
}

// the answer of a seeker with set, Name and keyIdentifier (id_len = 0: none)
__device__ __forceinline__ Match seek(const uint8_t* __restrict__ blob, const Certs& C, const Table& T, uint32_t n_overflow, uint32_t set,
                                      uint64_t name_off, uint32_t name_len, uint64_t id_off, uint32_t id_len, int lane, const Seed& sd) {
    Key key;
    key.set = set;
    key.name_off = name_off;
    key.name_len = name_len;
    if (id_len == 0) {
        key.kind = KIND_ANY;
        return lookup(blob, C, T, n_overflow, key, lane, sd);
    }
    key.kind = KIND_NOSKI;
    const Match without = lookup(blob, C, T, n_overflow, key, lane, sd);
    key.kind = KIND_SKI;
    key.id_off = id_off;
    key.id_len = id_len;
    return join(lookup(blob, C, T, n_overflow, key, lane, sd), without);
}

__device__ __forceinline__ void write_result(mldsa_find_result* __restrict__ r, bool seeker, const Match& m) {
    const int st = result_status(seeker, m);
    mldsa_find_result out = {};
    out.issuer = st == R_FOUND ? m.lowest : NO_ISSUER;
    out.candidates = st == R_FOUND ? m.count : 0;
    out.status = (uint8_t)st;
    *r = out;
}

__global__ __launch_bounds__(IDS_BLOCK) void k_find_ids(const uint8_t* __restrict__ blob, uint64_t blob_len, const mldsa_x509_cert* __restrict__ certs,
                                                        const mldsa_path_fields* __restrict__ policy, uint32_t n, mldsa_find_id* __restrict__ ids) {
    const uint32_t i = blockIdx.x * IDS_BLOCK + threadIdx.x;
    if (i >= n) return;
    mldsa_find_id r = {};
    if (policy != nullptr) {
        const mldsa_x509_cert c = certs[i];
        const uint32_t pst = policy[i].status;
        const uint64_t ext_off = policy[i].ext_off;
        const uint32_t ext_len = policy[i].ext_len;
        if (pst != ST_RANGE && pst != ST_DER && ext_len != 0) {
            r.status = ST_RANGE;
            if (in_range(c.off, c.len, blob_len) && inside(ext_off, ext_len, c.off, c.len)) {
                const uint32_t rel = (uint32_t)(ext_off - c.off);
                const Ids w = walk_ids(BlobBytes{blob + c.off}, rel, rel + ext_len);
                r.status = (uint8_t)w.status;
                if (w.status == ST_OK) {
                    if (w.ski_len != 0) r.ski_off = c.off + w.ski_off;
                    if (w.aki_len != 0) r.aki_off = c.off + w.aki_off;
                    r.ski_len = (uint8_t)w.ski_len;
                    r.aki_len = (uint8_t)w.aki_len;
                }
            }
        }
    }
    ids[i] = r;
}

__global__ __launch_bounds__(64 * WAVES) void k_find_claim(const uint8_t* __restrict__ blob, Certs C, Seed sd, unsigned long long* __restrict__ tags,
                                                           uint32_t* __restrict__ owners, uint32_t mask, uint32_t* __restrict__ slot_of,
                                                           Key* __restrict__ keys, mldsa_find_totals* __restrict__ totals) {
    __shared__ uint32_t counted[2];  // candidates, slots claimed
    if (threadIdx.x < 2) counted[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i < C.n) {  // (the whole wave: one certificate per wave)
        for (uint32_t k = 0; k < 2; ++k) {
            const uint32_t e = 2 * i + k;
            Key key;
            uint32_t slot = NO_ENTRY;
            if (candidate_key(C, i, k, &key)) {
                const uint64_t h = wave_hash(blob, key, lane, sd);
                slot = NO_SLOT;
                if (lane == 0) {
                    keys[e] = key;
                    if (k == 0) atomicAdd(&counted[0], 1u);
                    for (uint32_t p = 0; p < PROBE_MAX && slot == NO_SLOT; ++p) {
                        const uint32_t s = (uint32_t)(h + p) & mask;
                        // a look first: a tag that is there already needs no atomic
                        uint64_t t = __hip_atomic_load(&tags[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (t == EMPTY_TAG) {
                            t = atomicCAS(&tags[s], (unsigned long long)EMPTY_TAG, (unsigned long long)h);
                            if (t == EMPTY_TAG) {
                                atomicAdd(&counted[1], 1u);
                                t = h;
                            }
                        }
                        if (t == h) slot = s;
                    }
                    if (slot != NO_SLOT) atomicMin(&owners[slot], e);
                }
            }
            if (lane == 0) slot_of[e] = slot;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (counted[0] != 0) {
            atomicAdd(&totals->candidates, counted[0]);
            atomicAdd(&totals->keys, 2 * counted[0]);
        }
        if (counted[1] != 0) atomicAdd(&totals->slots, counted[1]);
    }
}

__global__ __launch_bounds__(64 * WAVES) void k_find_confirm(const uint8_t* __restrict__ blob, Certs C, const uint32_t* __restrict__ owners,
                                                             uint32_t* __restrict__ counts, const uint32_t* __restrict__ slot_of,
                                                             const Key* __restrict__ keys, uint32_t* __restrict__ overflow,
                                                             mldsa_find_totals* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= C.n) return;  // (the whole wave)
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t e = 2 * i + k;
        const uint32_t slot = slot_of[e];
        if (slot == NO_ENTRY) continue;
        bool in_group = false;
        if (slot != NO_SLOT) {
            const uint32_t o = owners[slot];
            in_group = o == e || (o < 2 * C.n && wave_equal(blob, keys[e], keys[o], lane));
        }
        if (lane == 0) {
            if (in_group) {
                atomicAdd(&counts[slot], 1u);
            } else {
                const uint32_t at = atomicAdd(&totals->overflow, 1u);
                if (at < OVERFLOW_MAX) overflow[at] = e;
            }
        }
    }
}

// certs_out may be C.certs: a wave writes its own row's issuer alone, which no wave reads
__global__ __launch_bounds__(64 * WAVES) void k_find_issuers(const uint8_t* __restrict__ blob, Certs C, Seed sd, Table T,
                                                             const mldsa_find_totals* __restrict__ totals, mldsa_x509_cert* certs_out,
                                                             mldsa_find_result* __restrict__ results) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= C.n) return;  // (the whole wave)
    const mldsa_x509_cert c = C.certs[i];
    const mldsa_x509_fields& f = C.fields[i];
    const mldsa_find_id d = C.ids[i];
    const bool seeker = seeker_row(f.status, f.sig_set, d.status) && in_range(c.off, c.len, C.blob_len) &&
                        inside(f.issuer_off, f.issuer_len, c.off, c.len) &&
                        (d.aki_len == 0 || (d.aki_len <= MAX_KEYID && inside(d.aki_off, d.aki_len, c.off, c.len)));
    Match m;
    if (seeker) m = seek(blob, C, T, totals->overflow, f.sig_set, f.issuer_off, f.issuer_len, d.aki_off, d.aki_len, lane, sd);
    if (lane == 0) {
        write_result(&results[i], seeker, m);
        mldsa_x509_cert out;
        out.off = c.off;
        out.len = c.len;
        out.issuer = seeker && !m.space && m.count != 0 ? m.lowest : NO_ISSUER;
        certs_out[i] = out;
    }
}

// crls_out may be crls
__global__ __launch_bounds__(64 * WAVES) void k_find_crl_issuers(const uint8_t* __restrict__ blob, const mldsa_crl_item* crls,
                                                                 const mldsa_crl_fields* __restrict__ crl_fields, uint32_t n_crls, Certs C, Seed sd,
                                                                 Table T, const mldsa_find_totals* __restrict__ totals, mldsa_crl_item* crls_out,
                                                                 mldsa_find_result* __restrict__ results) {
    const int lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (c >= n_crls) return;  // (the whole wave)
    const mldsa_crl_item item = crls[c];
    const mldsa_crl_fields& f = crl_fields[c];
    bool seeker = f.status == ST_OK && f.sig_set != 0 && in_range(item.off, item.len, C.blob_len) &&
                  inside(f.issuer_off, f.issuer_len, item.off, item.len);
    uint64_t aki_off = 0;
    uint32_t aki_len = 0;
    if (seeker && f.ext_len != 0) {
        seeker = inside(f.ext_off, f.ext_len, item.off, item.len);
        if (seeker) {
            const uint32_t rel = (uint32_t)(f.ext_off - item.off);
            const Ids w = walk_ids(BlobBytes{blob + item.off}, rel, rel + f.ext_len);
            seeker = w.status == ST_OK;
            if (seeker && w.aki_len != 0) {
                aki_off = item.off + w.aki_off;
                aki_len = w.aki_len;
            }
        }
    }
    Match m;
    if (seeker) m = seek(blob, C, T, totals->overflow, f.sig_set, f.issuer_off, f.issuer_len, aki_off, aki_len, lane, sd);
    if (lane == 0) {
        write_result(&results[c], seeker, m);
        mldsa_crl_item out;
        out.off = item.off;
        out.len = item.len;
        out.issuer = seeker && !m.space && m.count != 0 ? m.lowest : NO_ISSUER;
        crls_out[c] = out;
    }
}

__global__ __launch_bounds__(IDS_BLOCK) void k_find_ca_min(const mldsa_crl_item* __restrict__ crls, uint32_t n_crls, uint32_t n,
                                                           uint32_t* __restrict__ ca_crl) {
    const uint32_t c = blockIdx.x * IDS_BLOCK + threadIdx.x;
    if (c >= n_crls) return;
    const uint32_t ca = crls[c].issuer;
    if (ca < n) atomicMin(&ca_crl[ca], c);
}

__global__ __launch_bounds__(IDS_BLOCK) void k_find_cert_crl(const mldsa_x509_cert* __restrict__ certs, uint32_t n, const uint32_t* __restrict__ ca_crl,
                                                             uint32_t* __restrict__ cert_crl) {
    const uint32_t i = blockIdx.x * IDS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t ca = certs[i].issuer;
    cert_crl[i] = ca < n ? ca_crl[ca] : CRL_NONE;
}

// ------------------------------------------------------------------------------------------------------------ host side
unsigned lane_grid(size_t n) { return (unsigned)((n + IDS_BLOCK - 1) / IDS_BLOCK); }
unsigned wave_grid(size_t n) { return (unsigned)((n + WAVES - 1) / WAVES); }

int check_batch(const char* fn, const mldsa_ctx* ctx, size_t n, const char* what) {
    if (n > MLDSA_FIND_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_FIND_MAX_CERTS " + what);
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    return MLDSA_OK;
}

int check_scratch(const char* fn, const void* scratch, size_t bytes, size_t n) {
    if (!scratch || !aligned(scratch, 256) || bytes < scratch_bytes(n))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_find_scratch_bytes");
    return MLDSA_OK;
}

// the checks of the calls that use the table
int check_table(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs,
                const mldsa_x509_fields* fields, const mldsa_find_id* ids, size_t n, const uint8_t* seed, int hash_bits,
                const mldsa_find_totals* totals, const void* scratch, size_t bytes) {
    const int rc = check_batch(fn, ctx, n, "certificates");
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !certs || !fields || !ids || !seed || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(fields, 8) || !aligned(ids, 8) || !aligned(totals, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs, fields and ids must be 8-byte aligned, totals 4-byte aligned");
    if (hash_bits < 1 || hash_bits > 64) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": hash_bits outside 1 ... 64");
    return check_scratch(fn, scratch, bytes, n);
}

Seed seed_of(const uint8_t* seed, int hash_bits) {
    Seed sd;
    memcpy(&sd.s0, seed, 8);
    memcpy(&sd.s1, seed + 8, 8);
    sd.hash_bits = hash_bits;
    return sd;
}

Table table_of(const void* scratch, size_t n) {
    const Layout L = layout(n);
    const uint8_t* base = static_cast<const uint8_t*>(scratch);
    Table T;
    T.tags = reinterpret_cast<const unsigned long long*>(base + L.tags);
    T.owners = reinterpret_cast<const uint32_t*>(base + L.owners);
    T.counts = reinterpret_cast<const uint32_t*>(base + L.counts);
    T.overflow = reinterpret_cast<const uint32_t*>(base + L.overflow);
    T.keys = reinterpret_cast<const Key*>(base + L.keys);
    T.mask = (uint32_t)(table_slots(n) - 1);
    return T;
}

// every check is the caller's
int launch_ids(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_path_fields* policy, size_t n,
               mldsa_find_id* ids, hipStream_t s) {
    hipLaunchKernelGGL(k_find_ids, dim3(lane_grid(n)), dim3(IDS_BLOCK), 0, s, blob, blob_len, certs, policy, (uint32_t)n, ids);
    LAYER_LAUNCHED("k_find_ids launch");
    return MLDSA_OK;
}

int launch_table(const char* fn, const uint8_t* blob, const Certs& C, const Seed& sd, mldsa_find_totals* totals, void* scratch, hipStream_t s) {
    const Layout L = layout(C.n);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    const size_t slots = table_slots(C.n);
    hipError_t e = hipMemsetAsync(base + L.tags, 0xFF, L.counts - L.tags, s);  // tags and owners
    if (e == hipSuccess) e = hipMemsetAsync(base + L.counts, 0, 4 * slots, s);
    if (e == hipSuccess) e = hipMemsetAsync(totals, 0, sizeof(*totals), s);
    if (e != hipSuccess) return hip_failed(fn, "clearing the table", e);
    unsigned long long* tags = reinterpret_cast<unsigned long long*>(base + L.tags);
    uint32_t* owners = reinterpret_cast<uint32_t*>(base + L.owners);
    uint32_t* counts = reinterpret_cast<uint32_t*>(base + L.counts);
    uint32_t* slot_of = reinterpret_cast<uint32_t*>(base + L.slot_of);
    uint32_t* overflow = reinterpret_cast<uint32_t*>(base + L.overflow);
    Key* keys = reinterpret_cast<Key*>(base + L.keys);
    hipLaunchKernelGGL(k_find_claim, dim3(wave_grid(C.n)), dim3(64 * WAVES), 0, s, blob, C, sd, tags, owners, (uint32_t)(slots - 1), slot_of, keys, totals);
    LAYER_LAUNCHED("k_find_claim launch");
    hipLaunchKernelGGL(k_find_confirm, dim3(wave_grid(C.n)), dim3(64 * WAVES), 0, s, blob, C, owners, counts, slot_of, keys, overflow, totals);
    LAYER_LAUNCHED("k_find_confirm launch");
    return MLDSA_OK;
}

int launch_issuers(const char* fn, const uint8_t* blob, const Certs& C, const Seed& sd, const mldsa_find_totals* totals, const void* scratch,
                   mldsa_x509_cert* certs_out, mldsa_find_result* results, hipStream_t s) {
    hipLaunchKernelGGL(k_find_issuers, dim3(wave_grid(C.n)), dim3(64 * WAVES), 0, s, blob, C, sd, table_of(scratch, C.n), totals, certs_out, results);
    LAYER_LAUNCHED("k_find_issuers launch");
    return MLDSA_OK;
}

}  // namespace

extern "C" {

int mldsa_find_abi_version(void) { return MLDSA_FIND_ABI_VERSION; }

const char* mldsa_find_last_error(void) { return g_err.c_str(); }

size_t mldsa_find_table_slots(size_t n) { return table_slots(n); }

size_t mldsa_find_scratch_bytes(size_t n) { return scratch_bytes(n); }

int mldsa_find_ids(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_path_fields* policy, size_t n,
                   mldsa_find_id* ids, void* stream) {
    const char* fn = "mldsa_find_ids";
    if (n == 0) return MLDSA_OK;
    const int rc = check_batch(fn, ctx, n, "certificates");
    if (rc != MLDSA_OK) return rc;
    if ((!blob && blob_len != 0) || !certs || !ids) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(policy, 8) || !aligned(ids, 8))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs, policy and ids must be 8-byte aligned");
    LAYER_ON_DEVICE(ctx);
    return launch_ids(fn, blob, blob_len, certs, policy, n, ids, (hipStream_t)stream);
}

int mldsa_find_table(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields,
                     const mldsa_find_id* ids, size_t n, const uint8_t seed[16], int hash_bits, mldsa_find_totals* totals, void* scratch,
                     size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_find_table";
    if (n == 0) return MLDSA_OK;
    const int rc = check_table(fn, ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_table(fn, blob, Certs{certs, fields, ids, (uint32_t)n, blob_len}, seed_of(seed, hash_bits), totals, scratch, (hipStream_t)stream);
}

int mldsa_find_issuers(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields,
                       const mldsa_find_id* ids, size_t n, const uint8_t seed[16], int hash_bits, const mldsa_find_totals* totals, const void* scratch,
                       size_t scratch_bytes, mldsa_x509_cert* certs_out, mldsa_find_result* results, void* stream) {
    const char* fn = "mldsa_find_issuers";
    if (n == 0) return MLDSA_OK;
    const int rc = check_table(fn, ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes);
    if (rc != MLDSA_OK) return rc;
    if (!certs_out || !results) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs_out, 8) || !aligned(results, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs_out must be 8-byte aligned, results 4-byte aligned");
    LAYER_ON_DEVICE(ctx);
    return launch_issuers(fn, blob, Certs{certs, fields, ids, (uint32_t)n, blob_len}, seed_of(seed, hash_bits), totals, scratch, certs_out, results,
                          (hipStream_t)stream);
}

int mldsa_find_build(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields,
                     const mldsa_path_fields* policy, size_t n, const uint8_t seed[16], int hash_bits, mldsa_find_id* ids, mldsa_find_totals* totals,
                     mldsa_x509_cert* certs_out, mldsa_find_result* results, void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_find_build";
    if (n == 0) return MLDSA_OK;
    int rc = check_table(fn, ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes);
    if (rc != MLDSA_OK) return rc;
    if (!certs_out || !results) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(policy, 8) || !aligned(certs_out, 8) || !aligned(results, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": policy and certs_out must be 8-byte aligned, results 4-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    const Certs C{certs, fields, ids, (uint32_t)n, blob_len};
    const Seed sd = seed_of(seed, hash_bits);
    rc = launch_ids(fn, blob, blob_len, certs, policy, n, ids, s);
    if (rc == MLDSA_OK) rc = launch_table(fn, blob, C, sd, totals, scratch, s);
    if (rc == MLDSA_OK) rc = launch_issuers(fn, blob, C, sd, totals, scratch, certs_out, results, s);
    return rc;
}

int mldsa_find_crl_issuers(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_item* crls, const mldsa_crl_fields* crl_fields,
                           size_t n_crls, const mldsa_x509_cert* certs, const mldsa_x509_fields* fields, const mldsa_find_id* ids, size_t n,
                           const uint8_t seed[16], int hash_bits, const mldsa_find_totals* totals, const void* scratch, size_t scratch_bytes,
                           mldsa_crl_item* crls_out, mldsa_find_result* crl_results, void* stream) {
    const char* fn = "mldsa_find_crl_issuers";
    if (n_crls == 0) return MLDSA_OK;
    if (n_crls > MLDSA_FIND_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_FIND_MAX_CERTS CRLs");
    const int rc = check_table(fn, ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes);
    if (rc != MLDSA_OK) return rc;
    if (!crls || !crl_fields || !crls_out || !crl_results) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(crls, 8) || !aligned(crl_fields, 8) || !aligned(crls_out, 8) || !aligned(crl_results, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": crls, crl_fields and crls_out must be 8-byte aligned, crl_results 4-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_find_crl_issuers, dim3(wave_grid(n_crls)), dim3(64 * WAVES), 0, (hipStream_t)stream, blob, crls, crl_fields, (uint32_t)n_crls,
                       Certs{certs, fields, ids, (uint32_t)n, blob_len}, seed_of(seed, hash_bits), table_of(scratch, n), totals, crls_out, crl_results);
    LAYER_LAUNCHED("k_find_crl_issuers launch");
    return MLDSA_OK;
}

int mldsa_find_cert_crls(mldsa_ctx* ctx, const mldsa_x509_cert* certs, size_t n, const mldsa_crl_item* crls, size_t n_crls, uint32_t* cert_crl,
                         void* scratch, size_t scratch_bytes, void* stream) {
    const char* fn = "mldsa_find_cert_crls";
    if (n == 0) return MLDSA_OK;
    if (n_crls > MLDSA_FIND_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_FIND_MAX_CERTS CRLs");
    int rc = check_batch(fn, ctx, n, "certificates");
    if (rc != MLDSA_OK) return rc;
    if (!certs || !cert_crl || (!crls && n_crls != 0)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8) || !aligned(crls, 8) || !aligned(cert_crl, 4))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs and crls must be 8-byte aligned, cert_crl 4-byte aligned");
    rc = check_scratch(fn, scratch, scratch_bytes, n);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* ca_crl = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(scratch) + layout(n).ca_crl);
    const hipError_t e = hipMemsetAsync(ca_crl, 0xFF, 4 * n, s);
    if (e != hipSuccess) return hip_failed(fn, "clearing the CA array", e);
    if (n_crls != 0) {
        hipLaunchKernelGGL(k_find_ca_min, dim3(lane_grid(n_crls)), dim3(IDS_BLOCK), 0, s, crls, (uint32_t)n_crls, (uint32_t)n, ca_crl);
        LAYER_LAUNCHED("k_find_ca_min launch");
    }
    hipLaunchKernelGGL(k_find_cert_crl, dim3(lane_grid(n)), dim3(IDS_BLOCK), 0, s, certs, (uint32_t)n, ca_crl, cert_crl);
    LAYER_LAUNCHED("k_find_cert_crl launch");
    return MLDSA_OK;
}

}  // extern "C"
