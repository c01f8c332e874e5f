"""ctypes loader for the certificate-issuing library (include/mldsa_x509sign.h, fips204_amd/x509sign/libmldsa_x509sign.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "x509sign", "libmldsa_x509sign.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_x509sign.h")

ABI_VERSION = 1
MAX_CERTS = 1 << 30
SCAN_BLOCK = 256
FLAG_RND = 1
# status of a request: the first rule broken, in the order ENTRY, KEY, RANGE, LONG, DER, ALG, SPACE (1 ... 3 are _x509_lib's)
OK, RANGE, DER, ALG = 0, 1, 2, 3
ENTRY, KEY, LONG, SPACE = 8, 9, 10, 11

# mldsa_x509sign_req as a numpy record: 32 bytes, 8-byte aligned
REQ_DTYPE = np.dtype([("off", "<u8"), ("rnd_off", "<u8"), ("len", "<u4"), ("key", "<u4"), ("issuer", "<u4"), ("set", "u1"), ("flags", "u1"),
                      ("reserved", "<u2")])
# mldsa_x509sign_totals: 24 bytes, 8-byte aligned
TOTALS_DTYPE = np.dtype([("accepted", "<u8"), ("refused", "<u8"), ("out_bytes", "<u8")])
assert REQ_DTYPE.itemsize == 32 and TOTALS_DTYPE.itemsize == 24

_P, _SZ, _I, _U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
_NK = C.POINTER(C.c_size_t)  # n_keys: a host array of three

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_x509sign_abi_version": [],
    "mldsa_x509sign_last_error": [],
    "mldsa_x509sign_cert_len": [_I, _SZ],
    "mldsa_x509sign_out_bytes_max": [_SZ, _U64],
    "mldsa_x509sign_plan_bytes": [_SZ],
    # ctx, blob, blob_len, reqs, n, n_keys (host), out_len, out_certs, ops, status, totals, plan, plan_bytes, stream
    "mldsa_x509sign_plan": [_P, _P, _U64, _P, _SZ, _NK, _U64, _P, _P, _P, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, reqs, n, out, out_len, out_certs, status, stream
    "mldsa_x509sign_frame": [_P, _P, _U64, _P, _SZ, _P, _U64, _P, _P, _P],
    # ctx, blob, blob_len, reqs, n, n_keys (host), out, out_len, out_certs, ops, status, totals, plan, plan_bytes, stream
    "mldsa_x509sign_issue_ops": [_P, _P, _U64, _P, _SZ, _NK, _P, _U64, _P, _P, _P, _P, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_x509sign_last_error": C.c_char_p, "mldsa_x509sign_cert_len": _SZ, "mldsa_x509sign_out_bytes_max": _SZ,
             "mldsa_x509sign_plan_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "issuing certificates from TBSCertificates")


def check(rc):
    _layer.check(rc, load().mldsa_x509sign_last_error)
