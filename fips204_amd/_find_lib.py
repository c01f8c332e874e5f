"""ctypes loader for the path-building library (include/mldsa_find.h, fips204_amd/find/libmldsa_find.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "find", "libmldsa_find.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_find.h")

ABI_VERSION = 1
MAX_CERTS = 1 << 28
MAX_KEYID = 64
PROBE_MAX = 256
OVERFLOW_MAX = 1024
# status of an identifier row (0 ... 2 are _x509_lib's)
OK, RANGE, DER = range(3)
EXT = 26
# mldsa_find_result.status
FOUND, NONE, CERT, SPACE = range(4)
NO_ISSUER = 0xFFFFFFFF
CRL_NONE = 0xFFFFFFFF

# mldsa_find_id as a numpy record: 24 bytes, 8-byte aligned
ID_DTYPE = np.dtype([("ski_off", "<u8"), ("aki_off", "<u8"), ("ski_len", "u1"), ("aki_len", "u1"), ("status", "u1"), ("reserved", "u1", (5,))])
# mldsa_find_result: 12 bytes
RESULT_DTYPE = np.dtype([("issuer", "<u4"), ("candidates", "<u4"), ("status", "u1"), ("reserved", "u1", (3,))])
# mldsa_find_totals: 16 bytes
TOTALS_DTYPE = np.dtype([("candidates", "<u4"), ("keys", "<u4"), ("slots", "<u4"), ("overflow", "<u4")])
assert ID_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 12 and TOTALS_DTYPE.itemsize == 16

_P, _SZ, _U64, _I = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_find_abi_version": [],
    "mldsa_find_last_error": [],
    "mldsa_find_table_slots": [_SZ],
    "mldsa_find_scratch_bytes": [_SZ],
    # ctx, blob, blob_len, certs, policy, n, ids, stream
    "mldsa_find_ids": [_P, _P, _U64, _P, _P, _SZ, _P, _P],
    # ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes, stream
    "mldsa_find_table": [_P, _P, _U64, _P, _P, _P, _SZ, _P, _I, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes, certs_out, results, stream
    "mldsa_find_issuers": [_P, _P, _U64, _P, _P, _P, _SZ, _P, _I, _P, _P, _SZ, _P, _P, _P],
    # ctx, blob, blob_len, certs, fields, policy, n, seed, hash_bits, ids, totals, certs_out, results, scratch, scratch_bytes, stream
    "mldsa_find_build": [_P, _P, _U64, _P, _P, _P, _SZ, _P, _I, _P, _P, _P, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, crls, crl_fields, n_crls, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes, crls_out,
    # crl_results, stream
    "mldsa_find_crl_issuers": [_P, _P, _U64, _P, _P, _SZ, _P, _P, _P, _SZ, _P, _I, _P, _P, _SZ, _P, _P, _P],
    # ctx, certs, n, crls, n_crls, cert_crl, scratch, scratch_bytes, stream
    "mldsa_find_cert_crls": [_P, _P, _SZ, _P, _SZ, _P, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_find_last_error": C.c_char_p, "mldsa_find_table_slots": _SZ, "mldsa_find_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "X.509 path building on the device")


def check(rc):
    _layer.check(rc, load().mldsa_find_last_error)
