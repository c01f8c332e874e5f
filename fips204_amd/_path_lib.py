"""ctypes loader for the path-validation library (include/mldsa_path.h, fips204_amd/path/libmldsa_path.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "path", "libmldsa_path.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_path.h")

ABI_VERSION = 1
MAX_CERTS = 1 << 30
MAX_EXTS = 32
MAX_DEPTH = 16
NO_PATH_LEN = 0xFFFFFFFF
# flags: mldsa_path_parse, mldsa_path_crl_times, mldsa_path_chain take one each
ALLOW_UNKNOWN_CRITICAL, REQUIRE_NEXT_UPDATE, ALLOW_NO_CRL = 1, 2, 4
# mldsa_path_fields.flags
V3, HAS_BC, IS_CA, HAS_KU = 1, 2, 4, 8
# status of the walk: the first class broken (0 ... 2 are _x509_lib's)
OK, RANGE, DER = range(3)
VERSION, TIME, EXT, CRITICAL = 22, 23, 24, 25
# mldsa_path_result.verdict
TRUSTED, CERT, SIG, POLICY, NOT_YET, EXPIRED, REVOKED, REVOCATION, NOT_CA, KEY_USAGE, PATH_LEN, NO_ANCHOR, DEPTH = range(13)
# time_status of mldsa_path_crl_times
CRL_FRESH, CRL_REFUSED, CRL_TIME, CRL_NOT_YET, CRL_STALE = range(5)

# mldsa_path_fields as a numpy record: 48 bytes, 8-byte aligned
FIELDS_DTYPE = np.dtype([("not_before", "<i8"), ("not_after", "<i8"), ("ext_off", "<u8"), ("crit_off", "<u8"), ("ext_len", "<u4"),
                         ("path_len", "<u4"), ("key_usage", "<u2"), ("flags", "u1"), ("n_ext", "u1"), ("status", "u1"), ("reserved", "u1", (3,))])
# mldsa_path_result: 8 bytes
RESULT_DTYPE = np.dtype([("where", "<u4"), ("verdict", "u1"), ("depth", "u1"), ("reserved", "u1", (2,))])
# a node of mldsa_path_chain's scratch: 8 bytes
NODE_DTYPE = np.dtype([("issuer", "<u4"), ("own", "u1"), ("as_issuer", "u1"), ("path_len", "u1"), ("anchor", "u1")])
assert FIELDS_DTYPE.itemsize == 48 and RESULT_DTYPE.itemsize == 8 and NODE_DTYPE.itemsize == 8

_P, _SZ, _U, _U64, _I64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_uint64, C.c_int64

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_path_abi_version": [],
    "mldsa_path_last_error": [],
    "mldsa_path_scratch_bytes": [_SZ],
    # ctx, blob, blob_len, offs, n, seconds, status, stream
    "mldsa_path_times": [_P, _P, _U64, _P, _SZ, _P, _P, _P],
    # ctx, blob, blob_len, certs, n, flags, fields, stream
    "mldsa_path_parse": [_P, _P, _U64, _P, _SZ, _U, _P, _P],
    # ctx, blob, blob_len, crl_fields, crl_status, crl_ok, n_crls, now, flags, this_s, next_s, time_status, fresh_ok, stream
    "mldsa_path_crl_times": [_P, _P, _U64, _P, _P, _P, _SZ, _I64, _U, _P, _P, _P, _P, _P],
    # ctx, certs, policy, cert_status, cert_ok, revocation, anchor, n, now, flags, results, scratch, scratch_bytes, stream
    "mldsa_path_chain": [_P, _P, _P, _P, _P, _P, _P, _SZ, _I64, _U, _P, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_path_last_error": C.c_char_p, "mldsa_path_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "X.509 path validation on the device")


def check(rc):
    _layer.check(rc, load().mldsa_path_last_error)
