"""ctypes loader for the revocation-list library (include/mldsa_crl.h, fips204_amd/crl/libmldsa_crl.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "crl", "libmldsa_crl.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_crl.h")

ABI_VERSION = 1
MAX_CRLS = 1 << 30
MAX_ENTRIES = 1 << 30
MAX_CERTS = 1 << 30
SERIAL_MAX = 20
SCAN_BLOCK = 256
NONE = 0xFFFFFFFF  # cert_crl[i]: no CRL covers certificate i
CHECK_NAMES = 1    # flag of mldsa_crl_ops
# status of a CRL: the first rule broken (0 ... 6 are _x509_lib's)
OK, RANGE, DER, ALG, SIG, ISSUER, NAME = range(7)
VERSION, ENTRY, SPACE = 19, 20, 21
# revocation[i]
GOOD, REVOKED, NO_CRL, CRL_INDEX, CRL_REFUSED, CERT, SCOPE = range(7)

# mldsa_crl_item as a numpy record: 16 bytes, 8-byte aligned
ITEM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("issuer", "<u4")])
# mldsa_crl_fields: 88 bytes, 8-byte aligned
FIELDS_DTYPE = np.dtype([("tbs_off", "<u8"), ("sig_off", "<u8"), ("issuer_off", "<u8"), ("this_off", "<u8"), ("next_off", "<u8"),
                         ("revoked_off", "<u8"), ("ext_off", "<u8"), ("tbs_len", "<u4"), ("issuer_len", "<u4"), ("revoked_len", "<u4"),
                         ("ext_len", "<u4"), ("first", "<u4"), ("count", "<u4"), ("sig_set", "u1"), ("status", "u1"), ("reserved", "u1", (6,))])
# mldsa_crl_entry: 32 bytes, 8-byte aligned
ENTRY_DTYPE = np.dtype([("serial", "u1", (20,)), ("serial_len", "u1"), ("reserved", "u1", (3,)), ("crl", "<u4"), ("off", "<u4")])
# mldsa_crl_totals: 40 bytes, 8-byte aligned
TOTALS_DTYPE = np.dtype([("accepted", "<u8"), ("refused", "<u8"), ("entries", "<u8"), ("slots", "<u8"), ("overflow", "<u4"), ("reserved", "<u4")])
assert ITEM_DTYPE.itemsize == 16 and FIELDS_DTYPE.itemsize == 88 and ENTRY_DTYPE.itemsize == 32 and TOTALS_DTYPE.itemsize == 40

_P, _SZ, _U, _U64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_uint64

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_crl_abi_version": [],
    "mldsa_crl_last_error": [],
    "mldsa_crl_entries_bound": [_SZ],
    "mldsa_crl_table_slots": [_SZ],
    "mldsa_crl_scratch_bytes": [_SZ],
    # ctx, blob, blob_len, crls, n_crls, crl_fields, stream
    "mldsa_crl_parse": [_P, _P, _U64, _P, _SZ, _P, _P],
    # ctx, blob, blob_len, crls, n_crls, cert_fields, n_certs, flags, crl_fields, entries, max_entries, ops, status, totals, scratch,
    # scratch_bytes, stream
    "mldsa_crl_ops": [_P, _P, _U64, _P, _SZ, _P, _SZ, _U, _P, _P, _SZ, _P, _P, _P, _P, _SZ, _P],
    # ctx, entries, max_entries, table, table_slots, totals, stream
    "mldsa_crl_table": [_P, _P, _SZ, _P, _SZ, _P, _P],
    # ctx, blob, blob_len, certs, cert_fields, cert_crl, n_certs, crls, crl_fields, crl_status, crl_ok, n_crls, entries, max_entries, table,
    # table_slots, revocation, stream
    "mldsa_crl_check": [_P, _P, _U64, _P, _P, _P, _SZ, _P, _P, _P, _P, _SZ, _P, _SZ, _P, _SZ, _P, _P],
}
_RESTYPES = {"mldsa_crl_last_error": C.c_char_p, "mldsa_crl_entries_bound": _SZ, "mldsa_crl_table_slots": _SZ, "mldsa_crl_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "certificate revocation lists on the device")


def check(rc):
    _layer.check(rc, load().mldsa_crl_last_error)
