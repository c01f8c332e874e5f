"""ctypes loader for the request-signing library (include/mldsa_recsign.h, fips204_amd/recsign/libmldsa_recsign.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "recsign", "libmldsa_recsign.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_recsign.h")

ABI_VERSION = 1
MAX_OPS = 1 << 30
SCAN_BLOCK = 256
FLAG_RND = 1
CLASS_44, CLASS_65, CLASS_87, CLASS_REFUSED = 0, 1, 2, 3
CLASS_SETS = (44, 65, 87)  # class -> parameter set

# mldsa_recsign_op as a numpy record: 48 bytes, 8-byte aligned
OP_DTYPE = np.dtype([("msg_off", "<u8"), ("ctx_off", "<u8"), ("rnd_off", "<u8"), ("sig_off", "<u8"), ("msg_len", "<u4"), ("key", "<u4"),
                     ("ctx_len", "<u2"), ("set", "u1"), ("flags", "u1"), ("reserved", "<u4")])
assert OP_DTYPE.itemsize == 48


class RecsignKeys(C.Structure):
    """mldsa_recsign_keys"""
    _fields_ = [("n_keys", C.c_size_t), ("rho", C.c_void_p), ("cap_k", C.c_void_p), ("tr", C.c_void_p), ("s_1_hat_mont", C.c_void_p),
                ("s_2_hat_mont", C.c_void_p), ("t_0_hat_mont", C.c_void_p)]


class RecsignTotals(C.Structure):
    """mldsa_recsign_totals"""
    _fields_ = [("n", C.c_uint64 * 4), ("msg_bytes", C.c_uint64 * 3), ("ctx_bytes", C.c_uint64 * 3)]


class RecsignClass(C.Structure):
    """mldsa_recsign_class"""
    _fields_ = [("n", C.c_size_t), ("key_idx", C.c_void_p), ("msgs", C.c_void_p), ("ctxs", C.c_void_p), ("rnd", C.c_void_p), ("sigs", C.c_void_p),
                ("msg_off", C.c_void_p), ("ctx_off", C.c_void_p), ("status", C.c_void_p)]


class RecsignPacked(C.Structure):
    """mldsa_recsign_packed"""
    _fields_ = [("c", RecsignClass * 3), ("rnd_region", C.c_void_p), ("rnd_region_bytes", C.c_size_t)]


class RecsignInfo(C.Structure):
    """mldsa_recsign_info"""
    _fields_ = [("n", C.c_uint64 * 4), ("msg_bytes", C.c_uint64), ("ctx_bytes", C.c_uint64), ("scratch_needed", C.c_uint64)]


_P, _SZ, _I, _U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
_NK = C.POINTER(C.c_size_t)  # n_keys: a host array of three

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_recsign_abi_version": [],
    "mldsa_recsign_last_error": [],
    "mldsa_recsign_plan_bytes": [_SZ],
    "mldsa_recsign_front_bytes": [_SZ],
    "mldsa_recsign_arena_bytes": [_SZ, _SZ, _SZ, _U64, _U64],
    "mldsa_recsign_arena_bytes_max": [_SZ, _U64, _U64],
    # ctx, blob_len, out_len, ops, n_ops, n_keys (host), class_slot, totals, plan, plan_bytes, stream
    "mldsa_recsign_plan": [_P, _U64, _U64, _P, _SZ, _NK, _P, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, out_len, ops, n_ops, n_keys (host), class_slot, plan, plan_bytes, totals (host), arena, arena_bytes, packed (host), stream
    "mldsa_recsign_pack": [_P, _P, _U64, _U64, _P, _SZ, _NK, _P, _P, _SZ, C.POINTER(RecsignTotals), _P, _SZ, C.POINTER(RecsignPacked), _P],
    # ctx, ops, n_ops, blob_len, out, out_len, n_keys (host), class_slot, packed (host), status, stream
    "mldsa_recsign_scatter": [_P, _P, _SZ, _U64, _P, _U64, _NK, _P, C.POINTER(RecsignPacked), _P, _P],
    # ctx, mode, keys (host [3]), blob, blob_len, ops, n_ops, out, out_len, status, scratch, scratch_bytes, info (host), stream
    "mldsa_recsign_sign": [_P, _I, C.POINTER(RecsignKeys), _P, _U64, _P, _SZ, _P, _U64, _P, _P, _SZ, C.POINTER(RecsignInfo), _P],
}
_RESTYPES = {"mldsa_recsign_last_error": C.c_char_p, "mldsa_recsign_plan_bytes": _SZ, "mldsa_recsign_front_bytes": _SZ,
             "mldsa_recsign_arena_bytes": _SZ, "mldsa_recsign_arena_bytes_max": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "signing of request records")


def check(rc):
    _layer.check(rc, load().mldsa_recsign_last_error)
