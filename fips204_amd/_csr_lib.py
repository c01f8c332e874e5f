"""ctypes loader for the certification-request library (include/mldsa_csr.h, fips204_amd/csr/libmldsa_csr.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csr", "libmldsa_csr.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_csr.h")

ABI_VERSION = 1
MAX_REQUESTS = 1 << 30
SCAN_BLOCK = 256
FLAG_RND = 1
SERIAL_MAX = 20
# status of a request: the first rule broken.  Stage 1: RANGE, DER, VERSION, ALG, KEY, SIG; stage 2: stage 1's, RANGE, POP, ENTRY,
# TEMPLATE, LONG, SPACE (0 ... 4 are _x509_lib's)
OK, RANGE, DER, ALG, SIG = 0, 1, 2, 3, 4
VERSION, KEY, POP, ENTRY, TEMPLATE, LONG, SPACE = 12, 13, 14, 15, 16, 17, 18

# mldsa_csr_item as a numpy record: 16 bytes, 8-byte aligned
ITEM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
# mldsa_csr_fields: 56 bytes, 8-byte aligned
FIELDS_DTYPE = np.dtype([("cri_off", "<u8"), ("sig_off", "<u8"), ("key_off", "<u8"), ("subject_off", "<u8"), ("spki_off", "<u8"),
                         ("cri_len", "<u4"), ("subject_len", "<u4"), ("spki_len", "<u4"), ("set", "u1"), ("status", "u1"),
                         ("reserved", "u1", (2,))])
# mldsa_csr_issue: 64 bytes, 8-byte aligned
ISSUE_DTYPE = np.dtype([("serial_off", "<u8"), ("issuer_off", "<u8"), ("validity_off", "<u8"), ("ext_off", "<u8"), ("rnd_off", "<u8"),
                        ("issuer_len", "<u4"), ("validity_len", "<u4"), ("ext_len", "<u4"), ("key", "<u4"), ("issuer", "<u4"),
                        ("serial_len", "u1"), ("set", "u1"), ("flags", "u1"), ("reserved", "u1")])
# mldsa_csr_totals: 24 bytes, 8-byte aligned
TOTALS_DTYPE = np.dtype([("accepted", "<u8"), ("refused", "<u8"), ("out_bytes", "<u8")])
assert ITEM_DTYPE.itemsize == 16 and FIELDS_DTYPE.itemsize == 56 and ISSUE_DTYPE.itemsize == 64 and TOTALS_DTYPE.itemsize == 24

_P, _SZ, _I, _U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_csr_abi_version": [],
    "mldsa_csr_last_error": [],
    # set, serial_len, issuer_len, validity_len, subject_len, spki_len, ext_len
    "mldsa_csr_tbs_len": [_I, _SZ, _SZ, _SZ, _SZ, _SZ, _SZ],
    "mldsa_csr_plan_bytes": [_SZ],
    # ctx, blob, blob_len, items, n, fields, ops, status, stream
    "mldsa_csr_parse": [_P, _P, _U64, _P, _SZ, _P, _P, _P, _P],
    # ctx, blob, blob_len, fields, entries, ok, n, out_len, reqs_out, status, totals, plan, plan_bytes, stream
    "mldsa_csr_tbs_plan": [_P, _P, _U64, _P, _P, _P, _SZ, _U64, _P, _P, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, fields, entries, n, out, out_len, reqs_out, status, stream
    "mldsa_csr_tbs_write": [_P, _P, _U64, _P, _P, _SZ, _P, _U64, _P, _P, _P],
    # ctx, blob, blob_len, fields, entries, ok, n, out, out_len, reqs_out, status, totals, plan, plan_bytes, stream
    "mldsa_csr_tbs": [_P, _P, _U64, _P, _P, _P, _SZ, _P, _U64, _P, _P, _P, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_csr_last_error": C.c_char_p, "mldsa_csr_tbs_len": _SZ, "mldsa_csr_plan_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "certification requests on the device")


def check(rc):
    _layer.check(rc, load().mldsa_csr_last_error)
