"""ctypes loader for the key-deduplication library (include/mldsa_keys.h, fips204_amd/keys/libmldsa_keys.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "keys", "libmldsa_keys.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_keys.h")

ABI_VERSION = 1
ROUTE_PLAIN, ROUTE_CACHED = 0, 1
MAX_KEYS, MAX_CACHED, PROBE_MAX = 1 << 30, 1 << 24, 256


class KeysInfo(C.Structure):
    """mldsa_keys_info"""
    _fields_ = [("n_rows", C.c_uint32), ("route", C.c_int)]


_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_keys_abi_version": [],
    "mldsa_keys_last_error": [],
    "mldsa_keys_dedup_scratch_bytes": [_I, _SZ],
    "mldsa_keys_verify_scratch_bytes": [_I, _SZ, _SZ],
    # ctx, set, pk, n_keys, seed (host), hash_bits, row_of, table, table_rows, n_rows, scratch, scratch_bytes, stream
    "mldsa_keys_dedup": [_P, _I, _P, _SZ, C.c_char_p, _I, _P, _P, _SZ, _P, _P, _SZ, _P],
    # ctx, set, mode, pk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, seed (host), hash_bits, max_cached_keys,
    # scratch, scratch_bytes, info (host), stream
    "mldsa_verify_pk_dedup": [_P, _I, _I, _P, _SZ] + [_P] * 7 + [_SZ, C.c_char_p, _I, _SZ, _P, _SZ, C.POINTER(KeysInfo), _P],
}
_RESTYPES = {"mldsa_keys_last_error": C.c_char_p, "mldsa_keys_dedup_scratch_bytes": _SZ, "mldsa_keys_verify_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "the device key deduplication")


def check(rc):
    _layer.check(rc, load().mldsa_keys_last_error)
