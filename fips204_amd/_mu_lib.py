"""ctypes loader for the external-mu library (include/mldsa_mu.h, fips204_amd/mu/libmldsa_mu.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "mu", "libmldsa_mu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_mu.h")

ABI_VERSION = 1
MU_LEN = 64
MAX_OPS = 1 << 30
MIN_PASS_OPS = 64  # a scratch may be as small as one pass over min(n_ops, 64) operations

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_mu_abi_version": [],
    "mldsa_mu_last_error": [],
    "mldsa_mu_verify_scratch_bytes": [_I, _SZ],
    "mldsa_mu_sign_scratch_bytes": [_I, _SZ],
    # ctx, mode, tr, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, mu, mu_flag, n_ops, stream
    "mldsa_mu_compute": [_P, _I, _P, _SZ] + [_P] * 7 + [_SZ, _P],
    # ctx, set, rho, t1_d2_hat_mont, n_keys, key_idx, mu, mu_flag, sigs, ok, n_ops, scratch, scratch_bytes, stream
    "mldsa_verify_mu": [_P, _I, _P, _P, _SZ] + [_P] * 5 + [_SZ, _P, _SZ, _P],
    # ctx, set, rho, cap_k, s1, s2, t0, n_keys, key_idx, mu, mu_flag, rnd, sigs, status, n_ops, scratch, scratch_bytes, stream
    "mldsa_sign_mu": [_P, _I] + [_P] * 5 + [_SZ] + [_P] * 6 + [_SZ, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_mu_last_error": C.c_char_p, "mldsa_mu_verify_scratch_bytes": _SZ, "mldsa_mu_sign_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "signing or verifying from mu")


def check(rc):
    _layer.check(rc, load().mldsa_mu_last_error)
