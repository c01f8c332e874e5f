"""ctypes loader for the wire-record library (include/mldsa_rec.h, fips204_amd/rec/libmldsa_rec.so).

The library is layered on the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED
libmldsa_hip.so resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).
There is no fallback: a missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

import numpy as np

from . import _layer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "rec", "libmldsa_rec.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mldsa_rec.h")

ABI_VERSION = 1
MAX_OPS = 1 << 30
SCAN_BLOCK = 256
CLASS_44, CLASS_65, CLASS_87, CLASS_REFUSED = 0, 1, 2, 3
CLASS_SETS = (44, 65, 87)  # class -> parameter set

# mldsa_rec_op as a numpy record: 40 bytes, 8-byte aligned
OP_DTYPE = np.dtype([("pk_off", "<u8"), ("sig_off", "<u8"), ("msg_off", "<u8"), ("ctx_off", "<u8"), ("msg_len", "<u4"), ("ctx_len", "<u2"),
                     ("set", "u1"), ("reserved", "u1")])
assert OP_DTYPE.itemsize == 40


class RecTotals(C.Structure):
    """mldsa_rec_totals"""
    _fields_ = [("n", C.c_uint64 * 4), ("msg_bytes", C.c_uint64 * 3), ("ctx_bytes", C.c_uint64 * 3)]


class RecClass(C.Structure):
    """mldsa_rec_class"""
    _fields_ = [("n", C.c_size_t), ("pk", C.c_void_p), ("sigs", C.c_void_p), ("msgs", C.c_void_p), ("ctxs", C.c_void_p), ("ok", C.c_void_p),
                ("msg_off", C.c_void_p), ("ctx_off", C.c_void_p)]


class RecPacked(C.Structure):
    """mldsa_rec_packed"""
    _fields_ = [("c", RecClass * 3)]


class RecInfo(C.Structure):
    """mldsa_rec_info"""
    _fields_ = [("n", C.c_uint64 * 4), ("msg_bytes", C.c_uint64), ("ctx_bytes", C.c_uint64), ("scratch_needed", C.c_uint64)]


_P, _SZ, _I, _U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64

# name -> argtypes (all return int unless listed in _RESTYPES)
_SIGNATURES = {
    "mldsa_rec_abi_version": [],
    "mldsa_rec_last_error": [],
    "mldsa_rec_plan_bytes": [_SZ],
    "mldsa_rec_front_bytes": [_SZ],
    "mldsa_rec_scratch_bytes": [_SZ, _SZ, _SZ, _U64, _U64],
    "mldsa_rec_scratch_bytes_max": [_SZ, _U64, _U64],
    # ctx, blob, blob_len, ops, n_ops, class_slot, totals, plan, plan_bytes, stream
    "mldsa_rec_plan": [_P, _P, _U64, _P, _SZ, _P, _P, _P, _SZ, _P],
    # ctx, blob, blob_len, ops, n_ops, class_slot, plan, plan_bytes, totals (host), arena, arena_bytes, out (host), stream
    "mldsa_rec_pack": [_P, _P, _U64, _P, _SZ, _P, _P, _SZ, C.POINTER(RecTotals), _P, _SZ, C.POINTER(RecPacked), _P],
    # ctx, mode, blob, blob_len, ops, n_ops, ok, scratch, scratch_bytes, info (host), stream
    "mldsa_rec_verify": [_P, _I, _P, _U64, _P, _SZ, _P, _P, _SZ, C.POINTER(RecInfo), _P],
}
_RESTYPES = {"mldsa_rec_last_error": C.c_char_p, "mldsa_rec_plan_bytes": _SZ, "mldsa_rec_front_bytes": _SZ, "mldsa_rec_scratch_bytes": _SZ,
             "mldsa_rec_scratch_bytes_max": _SZ}


def load():
    return _layer.load_layer(LIB_PATH, _SIGNATURES, _RESTYPES, "verification from wire records")


def check(rc):
    _layer.check(rc, load().mldsa_rec_last_error)
