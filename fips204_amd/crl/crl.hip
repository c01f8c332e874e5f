// libmldsa_crl.so (include/mldsa_crl.h): certificate revocation lists in a blob to mldsa_rec_op descriptors (the CRL's own signature, in
// front of mldsa_rec_verify), to a table of the revoked serials, to one answer per certificate.  This library links and calls none of
// the other layers.
//
// Eight kernels, ordered by the kernel boundaries alone: no wave waits for another.
//   k_crl_parse          one CRL per lane, SCAN_BLOCK lanes per workgroup, as k_x509_parse: the range check and walk_crl of crl_plan.h on
//                        the blob; one mldsa_crl_fields row per CRL.
//   k_crl_place_sums     one CRL per lane: bound_i = revoked_len / 20 of the CRLs whose walk was accepted, summed per workgroup.
//   k_crl_place_offsets  one wave: the workgroups' sums to exclusive prefixes, in place.
//   k_crl_place          the same quantity scanned inside the workgroup (wave_inclusive of ../rec/rec_wave.h, the waves' totals through
//                        LDS): first_i, the SPACE rule, the slots reserved.  The first two are the placement scan of ../rec/rec_place.h at
//                        one quantity; this one keeps its scan written out (rec_place.h says why).
//   k_crl_entries        one CRL per wave, ENTRY_WAVES per workgroup: a WINDOW of the revoked list in LDS, staged by aligned 16-byte
//                        loads, one per lane; lane 0 hops from entry header to entry header inside it, the lanes walk one entry each
//                        and write its row.  The fetch functor reads LDS inside the window and the blob outside it.
//   k_crl_link           one CRL per wave: the link rule by lane 0, the two Names 64 bytes per step, ops[i], status[i], the totals; the
//                        slots of a CRL that is refused after all are emptied again.  The comparison and the op's write are those of
//                        ../x509/x509_dev.h, which k_x509_link shares.
//   k_crl_insert         one entry slot per lane, grid-stride: the open-addressing table over the entry rows, claimed by atomicCAS.
//   k_crl_check          one certificate per lane: its serial from its TBS, the probe, one answer byte.
// What bounds them: latency of the walk's dependent loads in k_crl_parse; in k_crl_entries lane 0's hop, a chain of dependent LDS byte
// reads per entry, while the list itself is read once through the window; k_crl_insert and k_crl_check are one random 4-byte and one
// random 32-byte access per probe.  Measured (profiles/crl_bench.jsonl): 4 096 CRLs of 64 entries take mldsa_crl_ops 0.18 ms, 1.4 G
// entries/s; one CRL of 262 144 entries is one wave's chain and takes 126 ms, about 480 ns per entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mldsa_crl.h"
#include "../layer/layer_dev.h"
#include "../layer/layer_host.h"
#include "../rec/rec_place.h"
#include "../x509/x509_dev.h"
#include "crl_plan.h"

namespace {

using namespace mldsa_layer;
using namespace mldsa_crl;
using mldsa_rec::wave_inclusive;
using mldsa_x509::BlobBytes;
using mldsa_x509::wave_names_differ;
using mldsa_x509::write_link_op;

static_assert(sizeof(mldsa_crl_item) == 16 && sizeof(mldsa_crl_fields) == 88 && sizeof(mldsa_crl_entry) == 32 && sizeof(mldsa_crl_totals) == 40 &&
                  sizeof(mldsa_rec_op) == 40 && sizeof(mldsa_x509_fields) == 56 && sizeof(mldsa_x509_cert) == 16,
              "the layouts of the headers");
static_assert(ST_OK == MLDSA_X509_OK && ST_RANGE == MLDSA_X509_RANGE && ST_DER == MLDSA_X509_DER && ST_ALG == MLDSA_X509_ALG &&
                  ST_SIG == MLDSA_X509_SIG && ST_ISSUER == MLDSA_X509_ISSUER && ST_NAME == MLDSA_X509_NAME && ST_VERSION == MLDSA_CRL_VERSION &&
                  ST_ENTRY == MLDSA_CRL_ENTRY && ST_SPACE == MLDSA_CRL_SPACE,
              "the status codes of include/mldsa_crl.h and include/mldsa_x509.h");
static_assert(REV_GOOD == MLDSA_CRL_GOOD && REV_REVOKED == MLDSA_CRL_REVOKED && REV_NO_CRL == MLDSA_CRL_NO_CRL &&
                  REV_CRL_INDEX == MLDSA_CRL_CRL_INDEX && REV_CRL_REFUSED == MLDSA_CRL_CRL_REFUSED && REV_CERT == MLDSA_CRL_CERT &&
                  REV_SCOPE == MLDSA_CRL_SCOPE && CRL_NONE == MLDSA_CRL_NONE,
              "the answers of include/mldsa_crl.h");
static_assert(FLAG_CHECK_NAMES == MLDSA_CRL_CHECK_NAMES && SERIAL_MAX == MLDSA_CRL_SERIAL_MAX && SCAN_BLOCK == MLDSA_CRL_SCAN_BLOCK &&
                  SCAN_BLOCK % 64 == 0 && MAX_CRLS == MLDSA_CRL_MAX_CRLS && MAX_ENTRIES == MLDSA_CRL_MAX_ENTRIES &&
                  MAX_CERTS == MLDSA_CRL_MAX_CERTS && WINDOW == 64 * 16,
              "the flag and the caps of include/mldsa_crl.h; one 16-byte chunk of the window per lane");

constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int ENTRY_WAVES = 4;    // CRLs per workgroup of k_crl_entries
constexpr int LINK_WAVES = 4;     // CRLs per workgroup of k_crl_link
constexpr int TABLE_BLOCK = 256;  // lanes per workgroup of k_crl_insert and k_crl_check
constexpr uint32_t HEADER_MAX = 6;  // bytes of the longest TLV header read_tlv accepts

// byte pos of a CRL of which the part `w` lies in LDS: the window where it holds the position, the blob elsewhere
struct WindowBytes {
    const uint8_t* crl;
    const uint8_t* lds;
    uint32_t mis;
    Window w;
    __device__ __forceinline__ uint32_t operator()(uint32_t pos) const {
        const uint64_t q = (uint64_t)mis + pos;
        return window_holds(w, q) ? lds[q - w.ws] : crl[pos];
    }
};

// what one lane wrote to the wave's LDS is read by another lane of the same wave behind this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t bound_of(const mldsa_crl_fields& r) { return r.status == ST_OK ? entries_bound(r.revoked_len) : 0; }

__global__ __launch_bounds__(SCAN_BLOCK) void k_crl_parse(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                          const mldsa_crl_item* __restrict__ crls, uint32_t n,
                                                          mldsa_crl_fields* __restrict__ fields) {
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const mldsa_crl_item c = crls[i];
    mldsa_crl_fields r = {};
    r.status = ST_RANGE;
    if (in_range(c.off, c.len, blob_len) && c.len >= 2) {
        const CrlWalk w = walk_crl(BlobBytes{blob + c.off}, c.len);
        r.status = (uint8_t)w.status;
        if (w.status != ST_DER) {
            r.tbs_off = c.off + w.tbs_off;
            r.tbs_len = w.tbs_len;
            r.issuer_off = c.off + w.issuer_off;
            r.issuer_len = w.issuer_len;
            r.this_off = c.off + w.this_off;
            if (w.next_off != 0) r.next_off = c.off + w.next_off;
            if (w.has_revoked) {
                r.revoked_off = c.off + w.revoked_off;
                r.revoked_len = w.revoked_len;
            }
            if (w.has_ext) {
                r.ext_off = c.off + w.ext_off;
                r.ext_len = w.ext_len;
            }
            r.sig_set = (uint8_t)w.sig_set;
            if (w.sig_set != 0) r.sig_off = c.off + w.sig_off;
        }
    }
    fields[i] = r;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_crl_place_sums(const mldsa_crl_fields* __restrict__ fields, uint32_t n,
                                                               uint64_t* __restrict__ sums) {
    __shared__ uint64_t part[SCAN_WAVES][1];
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    uint64_t bound[1] = {i < n ? bound_of(fields[i]) : 0};
    mldsa_rec::place_block_sums(bound, part, sums);
}

// one wave: sums[b] -> the sum over the blocks before b (in place)
__global__ __launch_bounds__(64) void k_crl_place_offsets(uint64_t* __restrict__ sums, uint32_t n_blocks) {
    uint64_t total[1];  // (the sum of all bounds: nobody asks for it)
    mldsa_rec::place_block_offsets(sums, n_blocks, total);
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_crl_place(mldsa_crl_fields* __restrict__ fields, uint32_t n, const uint64_t* __restrict__ sums,
                                                          uint64_t max_entries, mldsa_crl_totals* __restrict__ totals) {
    __shared__ uint64_t part[SCAN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    int st = ST_RANGE;
    uint64_t bound = 0;
    if (i < n) {
        st = fields[i].status;
        bound = bound_of(fields[i]);
    }
    const uint64_t inc = wave_inclusive(bound, lane);
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    // what the blocks before, the waves before and the lanes before add up to
    uint64_t first = sums[blockIdx.x] + inc - bound;
    for (int w = 0; w < SCAN_WAVES; ++w) {
        if (w >= wave) break;
        first += part[w];
    }
    uint64_t got = 0;  // the slots this CRL gets
    if (i < n && st == ST_OK) {
        if (place_status(first, bound, max_entries) == ST_OK) {
            fields[i].first = (uint32_t)first;
            got = bound;
        } else {
            fields[i].status = ST_SPACE;
        }
    }
    got = wave_sum(got);
    if (lane == 0 && got != 0) atomicAdd((unsigned long long*)&totals->slots, (unsigned long long)got);
}

__global__ __launch_bounds__(64 * ENTRY_WAVES) void k_crl_entries(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                                  const mldsa_crl_item* __restrict__ crls, uint32_t n,
                                                                  mldsa_crl_fields* __restrict__ fields, mldsa_crl_entry* __restrict__ entries,
                                                                  uint64_t max_entries) {
    __shared__ uint4 win[ENTRY_WAVES][WINDOW / 16];
    __shared__ uint32_t starts[ENTRY_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * ENTRY_WAVES + wave;
    if (i >= n) return;  // (the whole wave: one CRL per wave)
    const mldsa_crl_fields r = fields[i];
    if (r.status != ST_OK || r.revoked_len == 0) return;  // (no list: nothing to walk, count stays 0)
    const mldsa_crl_item c = crls[i];
    const uint64_t bound = entries_bound(r.revoked_len);
    // The row is checked again: only then is an offset followed or a slot written.
    if (!in_range(c.off, c.len, blob_len) || r.revoked_off < c.off || !in_range(r.revoked_off - c.off, r.revoked_len, c.len) ||
        !in_range(r.first, bound, max_entries)) {
        if (lane == 0) fields[i].status = ST_ENTRY;
        return;
    }
    const uint8_t* crl = blob + c.off;
    const uint32_t mis = (uint32_t)((uintptr_t)crl & 15);
    const uint8_t* frame = crl - mis;  // 16-byte aligned; nothing below crl is read through it
    uint32_t pos = (uint32_t)(r.revoked_off - c.off);
    const uint32_t end = pos + r.revoked_len;
    uint64_t total = 0;  // entries found so far
    bool bad = false;
    // Every round takes at least one entry of the at most `bound` that are taken in all: the loop ends whatever the data says.
    while (pos < end && total < bound && !bad) {
        const Window w = window_at(mis, c.len, pos);
        wave_sync();  // the round before is done with the window
        if (window_chunk(w, (uint32_t)lane)) win[wave][lane] = *reinterpret_cast<const uint4*>(frame + w.ws + 16 * (uint64_t)lane);
        wave_sync();
        const WindowBytes f{crl, reinterpret_cast<const uint8_t*>(win[wave]), mis, w};
        uint32_t found = 0, p = pos, fail = 0;
        if (lane == 0) {
            while (found < 64 && total + found < bound && p < end) {
                // the round's first header is read wherever it lies; a later one only where the window holds all of it
                const uint32_t header_end = end - p < HEADER_MAX ? end : p + HEADER_MAX;
                if (found != 0 && !(window_holds(w, (uint64_t)mis + p) && (uint64_t)mis + header_end <= w.hi)) break;
                const uint32_t next = hop(f, p, end);
                if (next == 0) {
                    fail = 1;
                    break;
                }
                starts[wave][found++] = p;
                p = next;
            }
        }
        wave_sync();
        found = (uint32_t)__shfl((int)found, 0, 64);
        p = (uint32_t)__shfl((int)p, 0, 64);
        fail = (uint32_t)__shfl((int)fail, 0, 64);
        if ((uint32_t)lane < found) {
            const uint32_t at = starts[wave][lane];
            const Entry e = walk_entry(f, at, end);
            if (!e.ok) {
                fail = 1;
            } else {
                const Serial s = load_serial(f, e.serial_at, e.serial_len);
                uint64_t* row = reinterpret_cast<uint64_t*>(&entries[r.first + total + lane]);
                row[0] = s.w[0] | (uint64_t)s.w[1] << 32;
                row[1] = s.w[2] | (uint64_t)s.w[3] << 32;
                row[2] = s.w[4] | (uint64_t)s.len << 32;
                row[3] = i | (uint64_t)at << 32;
            }
        }
        bad = wave_or(fail) != 0;
        total += found;
        pos = p;
    }
    if (pos != end) bad = true;  // more entries than slots, or bytes that are no entry
    if (lane == 0) {
        fields[i].count = bad ? 0 : (uint32_t)total;
        if (bad) fields[i].status = ST_ENTRY;
    }
}

__global__ __launch_bounds__(64 * LINK_WAVES) void k_crl_link(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                              const mldsa_crl_item* __restrict__ crls, uint32_t n,
                                                              const mldsa_x509_fields* __restrict__ cert_fields, uint32_t n_certs, uint32_t flags,
                                                              mldsa_crl_fields* __restrict__ fields, mldsa_crl_entry* __restrict__ entries,
                                                              uint64_t max_entries, mldsa_rec_op* __restrict__ ops, uint8_t* __restrict__ status,
                                                              mldsa_crl_totals* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * LINK_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;  // (the whole wave: one CRL per wave)
    int st = ST_OK;
    uint64_t mine = 0, theirs = 0;  // the two Names, where they are to be compared
    uint32_t name_len = 0;
    uint64_t pk_off = 0, sig_off = 0, tbs_off = 0;  // the op of an accepted CRL
    uint32_t tbs_len = 0, set = 0, count = 0;
    uint64_t slot = 0, slots = 0;  // the CRL's slots, where it has any
    if (lane == 0) {
        const mldsa_crl_fields& own = fields[i];
        const uint32_t issuer = crls[i].issuer;
        const bool known = issuer < n_certs;  // the issuer's row, never its DER; read only where issuer < n_certs
        const int iss_status = known ? cert_fields[issuer].status : 0;
        const uint32_t iss_key_set = known ? cert_fields[issuer].key_set : 0;
        set = own.sig_set;
        st = link_status(own.status, set, issuer, n_certs, iss_status, iss_key_set);
        if (own.status == ST_OK || own.status == ST_ENTRY) {  // (an empty list, the walk's ENTRY, has no slots: revoked_len is 0)
            const uint64_t bound = entries_bound(own.revoked_len);
            if (in_range(own.first, bound, max_entries)) {
                slot = own.first;
                slots = bound;
            }
        }
        if (st == ST_OK) {
            const mldsa_x509_fields& iss = cert_fields[issuer];
            pk_off = iss.key_off;
            sig_off = own.sig_off;
            tbs_off = own.tbs_off;
            tbs_len = own.tbs_len;
            count = own.count;
            if ((flags & FLAG_CHECK_NAMES) != 0) {
                const uint64_t a = own.issuer_off, b = iss.subject_off;
                const uint32_t a_len = own.issuer_len, b_len = iss.subject_len;
                // a row that points outside the blob is not followed: it counts as a mismatch, like Names of different lengths
                if (a_len != b_len || !in_range(a, a_len, blob_len) || !in_range(b, b_len, blob_len)) {
                    st = ST_NAME;
                } else {
                    mine = a;
                    theirs = b;
                    name_len = a_len;
                }
            }
        }
    }
    st = __shfl(st, 0, 64);
    mine = __shfl((unsigned long long)mine, 0, 64);
    theirs = __shfl((unsigned long long)theirs, 0, 64);
    name_len = (uint32_t)__shfl((int)name_len, 0, 64);
    slot = __shfl((unsigned long long)slot, 0, 64);
    slots = __shfl((unsigned long long)slots, 0, 64);
    if (wave_names_differ(blob, mine, theirs, name_len, lane)) st = ST_NAME;
    const bool acc = st == ST_OK;
    if (!acc) {  // a refused CRL lists nobody: its slots are emptied again
        uint64_t* rows = reinterpret_cast<uint64_t*>(entries + slot);
        for (uint64_t k = lane; k < 4 * slots; k += 64) rows[k] = 0;
    }
    if (lane == 0) {
        write_link_op(ops[i], acc, pk_off, sig_off, tbs_off, tbs_len, set);  // every other CRL's op is all zero
        status[i] = (uint8_t)st;
        if (!acc) fields[i].count = 0;
        atomicAdd((unsigned long long*)(acc ? &totals->accepted : &totals->refused), 1ull);
        if (acc && count != 0) atomicAdd((unsigned long long*)&totals->entries, (unsigned long long)count);
    }
}

// what the table needs of an entry row: the serial and the CRL
struct Row {
    Serial s;
    uint32_t crl;
};

__device__ __forceinline__ Row load_row(const mldsa_crl_entry* __restrict__ entries, uint64_t idx) {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(entries + idx);
    const uint64_t a = p[0], b = p[1], c = p[2];
    Row r;
    r.s.w[0] = (uint32_t)a;
    r.s.w[1] = (uint32_t)(a >> 32);
    r.s.w[2] = (uint32_t)b;
    r.s.w[3] = (uint32_t)(b >> 32);
    r.s.w[4] = (uint32_t)c;
    r.s.len = (uint32_t)(c >> 32) & 0xFF;
    r.crl = (uint32_t)p[3];
    return r;
}

__device__ __forceinline__ bool same_serial(const Serial& a, const Serial& b) {
    return a.len == b.len && a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3] && a.w[4] == b.w[4];
}

__global__ __launch_bounds__(TABLE_BLOCK) void k_crl_insert(const mldsa_crl_entry* __restrict__ entries, uint64_t max_entries,
                                                            uint32_t* __restrict__ table, uint32_t table_slots,
                                                            mldsa_crl_totals* __restrict__ totals) {
    const uint32_t mask = table_slots - 1;
    for (uint64_t e = (uint64_t)blockIdx.x * TABLE_BLOCK + threadIdx.x; e < max_entries; e += (uint64_t)gridDim.x * TABLE_BLOCK) {
        const Row r = load_row(entries, e);
        if (r.s.len == 0 || r.s.len > SERIAL_MAX) continue;  // an empty slot (or no serial at all)
        uint32_t h = hash_serial(r.crl, r.s) & mask;
        bool placed = false;
        for (uint32_t probe = 0; probe < table_slots; ++probe) {  // at most table_slots steps: the loop cannot spin
            if (atomicCAS(&table[h], 0u, (uint32_t)e + 1) == 0u) {
                placed = true;
                break;
            }
            h = (h + 1) & mask;
        }
        if (!placed) atomicOr(&totals->overflow, 1u);
    }
}

__global__ __launch_bounds__(TABLE_BLOCK) void k_crl_check(const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                           const mldsa_x509_cert* __restrict__ certs,
                                                           const mldsa_x509_fields* __restrict__ cert_fields,
                                                           const uint32_t* __restrict__ cert_crl, uint32_t n_certs,
                                                           const mldsa_crl_item* __restrict__ crls, const mldsa_crl_fields* __restrict__ crl_fields,
                                                           const uint8_t* __restrict__ crl_status, const uint8_t* __restrict__ crl_ok,
                                                           uint32_t n_crls, const mldsa_crl_entry* __restrict__ entries, uint64_t max_entries,
                                                           const uint32_t* __restrict__ table, uint32_t table_slots,
                                                           uint8_t* __restrict__ revocation) {
    const uint32_t i = blockIdx.x * TABLE_BLOCK + threadIdx.x;
    if (i >= n_certs) return;
    const uint32_t c = cert_crl[i];
    const bool has_crl = c != CRL_NONE, crl_in_range = c < n_crls;
    bool crl_accepted = false, cert_ok = false, same_issuer = false, listed = false;
    if (has_crl && crl_in_range) crl_accepted = crl_status[c] == ST_OK && crl_fields[c].status == ST_OK && (crl_ok == nullptr || crl_ok[c] != 0);
    if (crl_accepted) {
        const mldsa_x509_fields& r = cert_fields[i];
        Serial s;
        if (r.status != ST_RANGE && r.status != ST_DER && in_range(r.tbs_off, r.tbs_len, blob_len))
            s = cert_serial(BlobBytes{blob + r.tbs_off}, r.tbs_len);
        cert_ok = s.len != 0;
        same_issuer = certs[i].issuer == crls[c].issuer;
        if (cert_ok && same_issuer) {
            const uint32_t mask = table_slots - 1;
            uint32_t h = hash_serial(c, s) & mask;
            for (uint32_t probe = 0; probe < table_slots; ++probe) {  // at most table_slots steps
                const uint32_t v = table[h];
                if (v == 0) break;  // the chain ends: not listed
                if (v - 1 < max_entries) {  // (the table is untrusted like everything else: an index outside the rows matches nothing)
                    const Row row = load_row(entries, v - 1);
                    if (row.crl == c && same_serial(row.s, s)) {
                        listed = true;
                        break;
                    }
                }
                h = (h + 1) & mask;
            }
        }
    }
    revocation[i] = (uint8_t)answer(has_crl, crl_in_range, crl_accepted, cert_ok, same_issuer, listed);
}

// ------------------------------------------------------------------------------------------------------------ host side
// the checks the entry points share; the message names what failed
int check_crls(const char* fn, const mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_item* crls, size_t n_crls,
               const mldsa_crl_fields* crl_fields) {
    if (n_crls > MLDSA_CRL_MAX_CRLS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_CRL_MAX_CRLS CRLs");
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    if ((!blob && blob_len != 0) || ((!crls || !crl_fields) && n_crls != 0)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(crls, 8) || !aligned(crl_fields, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": crls and crl_fields must be 8-byte aligned");
    return MLDSA_OK;
}

int check_entries(const char* fn, const mldsa_crl_entry* entries, size_t max_entries) {
    if (max_entries > MLDSA_CRL_MAX_ENTRIES) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_CRL_MAX_ENTRIES entries");
    if (!entries && max_entries != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(entries, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": entries must be 8-byte aligned");
    return MLDSA_OK;
}

int check_table(const char* fn, const uint32_t* table, size_t slots, size_t max_entries) {
    if (!table) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(table, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": table must be 4-byte aligned");
    if (slots == 0 || (slots & (slots - 1)) != 0 || slots < table_slots(max_entries) || slots > ((size_t)1 << 31))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": table_slots must be a power of two, at least mldsa_crl_table_slots and at most 2^31");
    return MLDSA_OK;
}

int check_certs(const char* fn, const mldsa_x509_fields* cert_fields, size_t n_certs) {
    if (n_certs > MLDSA_CRL_MAX_CERTS) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": more than MLDSA_CRL_MAX_CERTS certificates");
    if (!cert_fields && n_certs != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(cert_fields, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": cert_fields must be 8-byte aligned");
    return MLDSA_OK;
}

// every check is the caller's: 1 <= n <= MLDSA_CRL_MAX_CRLS, the current device is the context's
int launch_parse(const char* fn, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_item* crls, size_t n, mldsa_crl_fields* fields,
                 hipStream_t s) {
    hipLaunchKernelGGL(k_crl_parse, dim3((unsigned)n_blocks(n)), dim3(SCAN_BLOCK), 0, s, blob, blob_len, crls, (uint32_t)n, fields);
    LAYER_LAUNCHED("k_crl_parse launch");
    return MLDSA_OK;
}

unsigned table_grid(size_t n) {
    const size_t blocks = (n + TABLE_BLOCK - 1) / TABLE_BLOCK;
    return (unsigned)(blocks < 4096 ? blocks : 4096);  // k_crl_insert strides over the rest
}

}  // namespace

extern "C" {

int mldsa_crl_abi_version(void) { return MLDSA_CRL_ABI_VERSION; }

const char* mldsa_crl_last_error(void) { return g_err.c_str(); }

size_t mldsa_crl_entries_bound(size_t bytes) { return (size_t)entries_bound(bytes); }

size_t mldsa_crl_table_slots(size_t max_entries) { return (size_t)table_slots(max_entries); }

size_t mldsa_crl_scratch_bytes(size_t n_crls) { return scratch_bytes(n_crls); }

int mldsa_crl_parse(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_item* crls, size_t n_crls,
                    mldsa_crl_fields* crl_fields, void* stream) {
    const char* fn = "mldsa_crl_parse";
    if (n_crls == 0) return MLDSA_OK;
    const int rc = check_crls(fn, ctx, blob, blob_len, crls, n_crls, crl_fields);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    return launch_parse(fn, blob, blob_len, crls, n_crls, crl_fields, (hipStream_t)stream);
}

int mldsa_crl_ops(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_crl_item* crls, size_t n_crls,
                  const mldsa_x509_fields* cert_fields, size_t n_certs, unsigned flags, mldsa_crl_fields* crl_fields, mldsa_crl_entry* entries,
                  size_t max_entries, mldsa_rec_op* ops, uint8_t* status, mldsa_crl_totals* totals, void* scratch, size_t scratch_bytes,
                  void* stream) {
    const char* fn = "mldsa_crl_ops";
    if (n_crls == 0) return MLDSA_OK;
    int rc = check_crls(fn, ctx, blob, blob_len, crls, n_crls, crl_fields);
    if (rc == MLDSA_OK) rc = check_certs(fn, cert_fields, n_certs);
    if (rc == MLDSA_OK) rc = check_entries(fn, entries, max_entries);
    if (rc != MLDSA_OK) return rc;
    if (!ops || !status || !totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(ops, 8) || !aligned(totals, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": ops and totals must be 8-byte aligned");
    if ((flags & ~MLDSA_CRL_CHECK_NAMES) != 0) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": unknown flag");
    if (!scratch || !aligned(scratch, 256) || scratch_bytes < mldsa_crl::scratch_bytes(n_crls))
        return fail(MLDSA_ERR_PARAM, std::string(fn) + ": scratch is NULL, not 256-byte aligned or smaller than mldsa_crl_scratch_bytes");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(totals, 0, sizeof(mldsa_crl_totals), s);
    if (e == hipSuccess && max_entries != 0) e = hipMemsetAsync(entries, 0, max_entries * sizeof(mldsa_crl_entry), s);
    if (e != hipSuccess) return hip_failed(fn, "clearing entries and totals", e);
    rc = launch_parse(fn, blob, blob_len, crls, n_crls, crl_fields, s);
    if (rc != MLDSA_OK) return rc;
    const uint32_t n = (uint32_t)n_crls, nb = (uint32_t)n_blocks(n_crls);
    uint64_t* sums = static_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(k_crl_place_sums, dim3(nb), dim3(SCAN_BLOCK), 0, s, crl_fields, n, sums);
    hipLaunchKernelGGL(k_crl_place_offsets, dim3(1), dim3(64), 0, s, sums, nb);
    hipLaunchKernelGGL(k_crl_place, dim3(nb), dim3(SCAN_BLOCK), 0, s, crl_fields, n, sums, (uint64_t)max_entries, totals);
    LAYER_LAUNCHED("place launch");
    hipLaunchKernelGGL(k_crl_entries, dim3((n + ENTRY_WAVES - 1) / ENTRY_WAVES), dim3(64 * ENTRY_WAVES), 0, s, blob, blob_len, crls, n, crl_fields,
                       entries, (uint64_t)max_entries);
    LAYER_LAUNCHED("k_crl_entries launch");
    hipLaunchKernelGGL(k_crl_link, dim3((n + LINK_WAVES - 1) / LINK_WAVES), dim3(64 * LINK_WAVES), 0, s, blob, blob_len, crls, n, cert_fields,
                       (uint32_t)n_certs, (uint32_t)flags, crl_fields, entries, (uint64_t)max_entries, ops, status, totals);
    LAYER_LAUNCHED("k_crl_link launch");
    return MLDSA_OK;
}

int mldsa_crl_table(mldsa_ctx* ctx, const mldsa_crl_entry* entries, size_t max_entries, uint32_t* table, size_t table_slots,
                    mldsa_crl_totals* totals, void* stream) {
    const char* fn = "mldsa_crl_table";
    if (!ctx) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL context");
    int rc = check_entries(fn, entries, max_entries);
    if (rc == MLDSA_OK) rc = check_table(fn, table, table_slots, max_entries);
    if (rc != MLDSA_OK) return rc;
    if (!totals) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(totals, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": totals must be 8-byte aligned");
    LAYER_ON_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(table, 0, table_slots * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(&totals->overflow, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_failed(fn, "clearing the table", e);
    if (max_entries == 0) return MLDSA_OK;
    hipLaunchKernelGGL(k_crl_insert, dim3(table_grid(max_entries)), dim3(TABLE_BLOCK), 0, s, entries, (uint64_t)max_entries, table,
                       (uint32_t)table_slots, totals);
    LAYER_LAUNCHED("k_crl_insert launch");
    return MLDSA_OK;
}

int mldsa_crl_check(mldsa_ctx* ctx, const uint8_t* blob, uint64_t blob_len, const mldsa_x509_cert* certs, const mldsa_x509_fields* cert_fields,
                    const uint32_t* cert_crl, size_t n_certs, const mldsa_crl_item* crls, const mldsa_crl_fields* crl_fields,
                    const uint8_t* crl_status, const uint8_t* crl_ok, size_t n_crls, const mldsa_crl_entry* entries, size_t max_entries,
                    const uint32_t* table, size_t table_slots, uint8_t* revocation, void* stream) {
    const char* fn = "mldsa_crl_check";
    if (n_certs == 0) return MLDSA_OK;
    int rc = check_crls(fn, ctx, blob, blob_len, crls, n_crls, crl_fields);
    if (rc == MLDSA_OK) rc = check_certs(fn, cert_fields, n_certs);
    if (rc == MLDSA_OK) rc = check_entries(fn, entries, max_entries);
    if (rc != MLDSA_OK) return rc;
    if (!certs || !cert_crl || !revocation || (!crl_status && n_crls != 0)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": NULL pointer");
    if (!aligned(certs, 8)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": certs must be 8-byte aligned");
    if (!aligned(cert_crl, 4)) return fail(MLDSA_ERR_PARAM, std::string(fn) + ": cert_crl must be 4-byte aligned");
    rc = check_table(fn, table, table_slots, max_entries);
    if (rc != MLDSA_OK) return rc;
    LAYER_ON_DEVICE(ctx);
    hipLaunchKernelGGL(k_crl_check, dim3((unsigned)((n_certs + TABLE_BLOCK - 1) / TABLE_BLOCK)), dim3(TABLE_BLOCK), 0, (hipStream_t)stream, blob,
                       blob_len, certs, cert_fields, cert_crl, (uint32_t)n_certs, crls, crl_fields, crl_status, crl_ok, (uint32_t)n_crls, entries,
                       (uint64_t)max_entries, table, (uint32_t)table_slots, revocation);
    LAYER_LAUNCHED("k_crl_check launch");
    return MLDSA_OK;
}

}  // extern "C"
