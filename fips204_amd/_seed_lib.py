"""ctypes loader for the seed-form key library (include/mldsa_seed.h, fips204_amd/seed/libmldsa_seed.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "seed", "libmldsa_seed.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_seed.h")

ABI_VERSION = 1
SEED_LEN = 32
MAX_KEYS = 1 << 24
MIN_PASS_KEYS = 64  # a scratch may be as small as one pass over min(n_keys, 64) keys

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_seed_abi_version": [],
    "mldsa_seed_last_error": [],
    "mldsa_seed_expand_scratch_bytes": [_I, _SZ],
    "mldsa_seed_check_scratch_bytes": [_I, _SZ],
    "mldsa_seed_sign_scratch_bytes": [_I, _SZ],
    # ctx, set, xi, rho, cap_k, tr, s1, s2, t0, pk, n_keys, scratch, scratch_bytes, stream
    "mldsa_seed_expand": [_P, _I] + [_P] * 8 + [_SZ, _P, _SZ, _P],
    # ctx, set, xi, sk, match, n_keys, scratch, scratch_bytes, stream
    "mldsa_seed_check": [_P, _I, _P, _P, _P, _SZ, _P, _SZ, _P],
    # ctx, set, mode, xi, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, rnd, sigs, status, n_ops, scratch, scratch_bytes, stream
    "mldsa_sign_seed": [_P, _I, _I, _P, _SZ] + [_P] * 8 + [_SZ, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_seed_last_error": C.c_char_p, "mldsa_seed_expand_scratch_bytes": _SZ, "mldsa_seed_check_scratch_bytes": _SZ,
             "mldsa_seed_sign_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "expanding or signing from seeds")


def check(rc):
    _layer.check(rc, load().mldsa_seed_last_error)
