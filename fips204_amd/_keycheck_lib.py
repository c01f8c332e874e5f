"""ctypes loader for the strict private-key import library (include/mldsa_keycheck.h, fips204_amd/keycheck/libmldsa_keycheck.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _layer, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "keycheck", "libmldsa_keycheck.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_keycheck.h")

ABI_VERSION = 1
MAX_KEYS = 1 << 24
MIN_PASS_KEYS = 64  # a scratch may be as small as one pass over min(n_keys, 64) keys

# verdict bits of one key (0 = good); a key with a range bit reports no consistency bit
KEY_S1_RANGE, KEY_S2_RANGE, KEY_T0, KEY_TR, KEY_PK = 1, 2, 4, 8, 16
KEY_BIT_NAMES = ((KEY_S1_RANGE, "S1_RANGE"), (KEY_S2_RANGE, "S2_RANGE"), (KEY_T0, "T0"), (KEY_TR, "TR"), (KEY_PK, "PK"))
# what mldsa_sk_import checks
LEVEL_RANGE, LEVEL_PAIR = 1, 2
LEVELS = {"range": LEVEL_RANGE, "pair": LEVEL_PAIR}

_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_keycheck_abi_version": [],
    "mldsa_keycheck_last_error": [],
    "mldsa_keycheck_scratch_bytes": [_I, _SZ],
    # ctx, set, sk, flag, n_keys, stream
    "mldsa_sk_range_check": [_P, _I, _P, _P, _SZ, _P],
    # ctx, set, sk, pk, flag, n_keys, scratch, scratch_bytes, stream
    "mldsa_keypair_check": [_P, _I, _P, _P, _P, _SZ, _P, _SZ, _P],
    # ctx, set, level, sk, pk, rho, cap_k, tr, s1, s2, t0, flag, n_keys, scratch, scratch_bytes, stream
    "mldsa_sk_import": [_P, _I, _I] + [_P] * 9 + [_SZ, _P, _SZ, _P],
}
_RESTYPES = {"mldsa_keycheck_last_error": C.c_char_p, "mldsa_keycheck_scratch_bytes": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "the pair check or the checked import")


def check(rc):
    _layer.check(rc, load().mldsa_keycheck_last_error)


def bit_names(flag):
    """'T0|TR' for 12, 'good' for 0"""
    return "|".join(nm for bit, nm in KEY_BIT_NAMES if flag & bit) or "good"
