"""ctypes loader for the certificate library (include/mldsa_x509.h, fips204_amd/x509/libmldsa_x509.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "x509", "libmldsa_x509.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_x509.h")

ABI_VERSION = 1
MAX_CERTS = 1 << 30
NO_ISSUER = 0xFFFFFFFF
# status of a certificate: the first rule broken, in this order
OK, RANGE, DER, ALG, SIG, ISSUER, NAME, PARSE_ONLY = range(8)
CHECK_NAMES = 1  # flag of mldsa_x509_link and mldsa_x509_ops

# mldsa_x509_cert as a numpy record: 16 bytes, 8-byte aligned
CERT_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("issuer", "<u4")])
# mldsa_x509_fields: 56 bytes, 8-byte aligned
FIELDS_DTYPE = np.dtype([("tbs_off", "<u8"), ("sig_off", "<u8"), ("key_off", "<u8"), ("issuer_off", "<u8"), ("subject_off", "<u8"),
                         ("tbs_len", "<u4"), ("issuer_len", "<u4"), ("subject_len", "<u4"), ("sig_set", "u1"), ("key_set", "u1"),
                         ("status", "u1"), ("reserved", "u1")])
assert CERT_DTYPE.itemsize == 16 and FIELDS_DTYPE.itemsize == 56

_P, _SZ, _U, _U64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_uint64

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_x509_abi_version": [],
    "mldsa_x509_last_error": [],
    # ctx, blob, blob_len, certs, n, fields, stream
    "mldsa_x509_parse": [_P, _P, _U64, _P, _SZ, _P, _P],
    # ctx, blob, blob_len, certs, fields, n, flags, ops, status, stream
    "mldsa_x509_link": [_P, _P, _U64, _P, _P, _SZ, _U, _P, _P, _P],
    # ctx, blob, blob_len, certs, n, flags, fields, ops, status, stream
    "mldsa_x509_ops": [_P, _P, _U64, _P, _SZ, _U, _P, _P, _P, _P],
}
_RESTYPES = {"mldsa_x509_last_error": C.c_char_p}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "certificate descriptors from DER")


def check(rc):
    _layer.check(rc, load().mldsa_x509_last_error)
