// The device helpers the certificate layers' kernels share (libmldsa_x509.so, _x509sign, _csr, _crl, _path, _find): the fetch functor
// that reads the blob for the plan headers' walks, and of the tail of the link step that k_x509_link and k_crl_link have in common the
// wave's comparison of the two Names and the write of the mldsa_rec_op.  Helpers only: every kernel (__global__) stays in its library's
// .hip file.  What differs between the two link kernels stays in them: how the issuer's row is read, ST_PARSE_ONLY, the CRL's slots and
// the zeroing of a refused CRL's rows, the totals' atomics.
//
// Everything here has internal linkage (the unnamed namespace), for the reason ../rec/rec_scan.h and ../layer/layer_host.h give.
//
// The rule of ../layer/layer_dev.h holds: a piece is shared only if every kernel that uses it compiles to the same instructions as
// with the piece written out.  With the two helpers below both link kernels keep their instructions and registers but for two address
// registers that change places (DESIGN.md has the table).  Two pieces of the tail did not pass and stay in both kernels: lane 0's
// decision on the two Name ranges (as a helper of any shape, most of k_x509_link comes out with other registers) and the broadcast of
// lane 0's Names (inside the helper it costs k_crl_link a VGPR).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mldsa_rec.h"
#include "../layer/layer_dev.h"
#include "x509_plan.h"

namespace mldsa_x509 {
namespace {

// byte pos of the blob, or of a certificate, request, CRL or TBS that begins at `at`; the callers' range checks vouch for the position
struct BlobBytes {
    const uint8_t* at;
    __host__ __device__ __forceinline__ uint32_t operator()(uint64_t pos) const { return at[pos]; }
};

// The whole wave: the two Names (the same in every lane: lane 0's, broadcast; name_len = 0: nothing to compare) are compared 64 bytes
// per step, one byte of each per lane, OR-reduced.  The same answer in every lane.
__device__ __forceinline__ bool wave_names_differ(const uint8_t* __restrict__ blob, uint64_t mine, uint64_t theirs, uint32_t name_len, int lane) {
    uint32_t diff = 0;
    for (uint64_t base = 0; base < name_len; base += 64) diff |= name_byte_diff(BlobBytes{blob}, mine, theirs, name_len, base + lane);
    return mldsa_layer::wave_or(diff) != 0;
}

// the op of an accepted item -- the issuer's key over the item's TBS --, all zero for every other
__device__ __forceinline__ void write_link_op(mldsa_rec_op& op, bool acc, uint64_t pk_off, uint64_t sig_off, uint64_t tbs_off, uint32_t tbs_len,
                                              uint32_t set) {
    op.pk_off = acc ? pk_off : 0;
    op.sig_off = acc ? sig_off : 0;
    op.msg_off = acc ? tbs_off : 0;
    op.ctx_off = 0;
    op.msg_len = acc ? tbs_len : 0;
    op.ctx_len = 0;
    op.set = acc ? (uint8_t)set : 0;
    op.reserved = 0;
}

}  // namespace
}  // namespace mldsa_x509
