"""ctypes loader for the large-batch verify library (include/mldsa_vfy.h, fips204_amd/vfy/libmldsa_vfy.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os
import re

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "vfy", "libmldsa_vfy.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_vfy.h")

ABI_VERSION = 1
MAX_OPS = 1 << 22

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_vfy_abi_version": [],
    "mldsa_vfy_last_error": [],
    "mldsa_vfy_scratch_bytes": [_I, _SZ],
    # ctx, set, mode, rho, tr, t1, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops, scratch, scratch_bytes, stream
    "mldsa_vfy_verify": [_P, _I, _I, _P, _P, _P, _SZ] + [_P] * 7 + [_SZ, _P, _SZ, _P],
    # ctx, set, rho, a_hat, n_ops, stream
    "mldsa_vfy_expand_a": [_P, _I, _P, _P, _SZ, _P],
    "mldsa_vfy_set_part_ops": [_SZ],
    "mldsa_vfy_profile_enable": [_P, _I],
    "mldsa_vfy_profile_report": [_P, C.c_char_p, _SZ],
}
_RESTYPES = {"mldsa_vfy_last_error": C.c_char_p, "mldsa_vfy_scratch_bytes": _SZ, "mldsa_vfy_set_part_ops": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "the large-batch verify pass")


def check(rc):
    _layer.check(rc, load().mldsa_vfy_last_error)


def part_ops():
    """MLDSA_VFY_PART_OPS as the header states it: ops of one part of a call"""
    return int(re.search(r"^#define MLDSA_VFY_PART_OPS (\d+)\s*$", open(HEADER_PATH).read(), flags=re.M).group(1))
