"""ctypes loader for the mu-stream library (include/mldsa_mus.h, fips204_amd/mus/libmldsa_mus.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os
import re

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "mus", "libmldsa_mus.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_mus.h")

ABI_VERSION = 1
MU_LEN = 64
MAX_OPS = 1 << 30
STATE_BYTES_PER_OP = 208

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_mus_abi_version": [],
    "mldsa_mus_last_error": [],
    "mldsa_mus_state_bytes": [_SZ],
    # ctx, mode, tr, n_keys, key_idx, ctxs, ctx_off, state, state_bytes, n_ops, stream
    "mldsa_mus_init": [_P, _I, _P, _SZ, _P, _P, _P, _P, _SZ, _SZ, _P],
    # ctx, state, state_bytes, pieces, piece_off, n_ops, stream
    "mldsa_mus_update": [_P, _P, _SZ, _P, _P, _SZ, _P],
    # ctx, state, state_bytes, mu, mu_flag, n_ops, stream
    "mldsa_mus_final": [_P, _P, _SZ, _P, _P, _SZ, _P],
    # ctx, staging_bytes, out
    "mldsa_mus_host_create": [_P, _SZ, C.POINTER(C.c_void_p)],
    "mldsa_mus_host_destroy": [_P],
    # h, mode, tr, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, mu, mu_flag, n_ops
    "mldsa_mus_host_compute": [_P, _I, _P, _SZ] + [_P] * 7 + [_SZ],
}
_RESTYPES = {"mldsa_mus_last_error": C.c_char_p, "mldsa_mus_state_bytes": _SZ, "mldsa_mus_host_destroy": None}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "mu of messages in pieces or in host memory")


def check(rc):
    _layer.check(rc, load().mldsa_mus_last_error)


def wave_max_ops():
    """MLDSA_MUS_WAVE_MAX_OPS as the header states it: calls of at most this many ops run one op per wave"""
    return int(re.search(r"^#define MLDSA_MUS_WAVE_MAX_OPS (\d+)\s*$", open(HEADER_PATH).read(), flags=re.M).group(1))
