"""ctypes loader for the pre-hash library (include/mldsa_ph.h, fips204_amd/ph/libmldsa_ph.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the pre-hash library's
NEEDED libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of
mldsa_ctx).  There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "ph", "libmldsa_ph.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_ph.h")

ABI_VERSION = 1
PH_SHA256, PH_SHA512, PH_SHAKE128 = 0, 1, 2
# the other functions of the NIST hash OID arc: 16 + the last OID arc (include/mldsa_ph.h)
PH_SHA384, PH_SHA224, PH_SHA512_224, PH_SHA512_256 = 18, 20, 21, 22
PH_SHA3_224, PH_SHA3_256, PH_SHA3_384, PH_SHA3_512, PH_SHAKE256 = 23, 24, 25, 26, 28

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_ph_abi_version": [],
    "mldsa_ph_last_error": [],
    "mldsa_ph_row_len": [_I],
    "mldsa_ph_scratch_bytes": [_I, _SZ],
    # ctx, ph, msgs, msg_off, out, bad, n_ops, stream
    "mldsa_prehash": [_P, _I, _P, _P, _P, _P, _SZ, _P],
    # ctx, set, ph, rho, tr, t1, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, scratch, scratch_bytes, stream
    "mldsa_hash_verify": [_P, _I, _I, _P, _P, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P],
    # ctx, set, ph, pk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, scratch, scratch_bytes, stream
    "mldsa_hash_verify_pk": [_P, _I, _I, _P, _SZ, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _SZ, _P],
    # ctx, set, ph, rho, K, tr, s1, s2, t0, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, rnd, sigs, status, n_ops, scratch,
    # scratch_bytes, stream
    "mldsa_hash_sign": [_P, _I, _I] + [_P] * 6 + [_SZ] + [_P] * 8 + [_SZ, _P, _SZ, _P],
    # the incremental pre-hash
    "mldsa_ph_state_bytes": [_I, _SZ],
    # ctx, ph, state, state_bytes, n_ops, stream
    "mldsa_ph_init": [_P, _I, _P, _SZ, _SZ, _P],
    # ctx, ph, state, state_bytes, pieces, piece_off, n_ops, stream
    "mldsa_ph_update": [_P, _I, _P, _SZ, _P, _P, _SZ, _P],
    # ctx, ph, state, state_bytes, out, out_off, bad, n_ops, stream
    "mldsa_ph_final": [_P, _I, _P, _SZ, _P, _P, _P, _SZ, _P],
    # HashML-DSA from host memory: ctx, staging_bytes, out
    "mldsa_ph_host_create": [_P, _SZ, C.POINTER(_P)],
    "mldsa_ph_host_destroy": [_P],
    # h, set, ph, pk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops
    "mldsa_hash_verify_host": [_P, _I, _I, _P, _SZ] + [_P] * 7 + [_SZ],
    # h, set, ph, sk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, rnd, sigs, status, n_ops
    "mldsa_hash_sign_host": [_P, _I, _I, _P, _SZ] + [_P] * 8 + [_SZ],
}
_RESTYPES = {"mldsa_ph_last_error": C.c_char_p, "mldsa_ph_scratch_bytes": _SZ, "mldsa_ph_state_bytes": _SZ,
             "mldsa_ph_host_destroy": None}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "the device pre-hash")


def check(rc):
    _layer.check(rc, load().mldsa_ph_last_error)
