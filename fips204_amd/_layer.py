"""What the ctypes loaders of the layered libraries share (_ph_lib, _keys_lib, _mu_lib, _seed_lib, _keycheck_lib).

A layered library links the core (include/mldsa_hip.h): the core is loaded first, so that the library's NEEDED libmldsa_hip.so
resolves to the copy already in the process (one HIP module registration, one kind of mldsa_ctx).  There is no fallback: a
missing library is an ImportError with a build hint.
"""
import ctypes as C
import os

from . import _lib

_loaded = {}


def load_layer(path, signatures, restypes, what):
    """The library at `path` (fips204_amd/<layer>/libmldsa_<layer>.so) with its prototypes set; loaded once per process.

    signatures: name -> argtypes; restypes: name -> restype for what does not return int; what: what the library is needed for,
    for the message of a missing one."""
    lib = _loaded.get(path)
    if lib is not None:
        return lib
    _lib.load()  # the core first: the library's NEEDED entry binds to it
    if not os.path.exists(path):
        layer = os.path.basename(os.path.dirname(path))
        raise ImportError(
            f"{path} is missing: build it with `python -m fips204_amd.build` "
            f"(make -C fips204_amd/{layer} after the core); there is no host fallback for {what}")
    lib = C.CDLL(path)
    for name, argtypes in signatures.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restypes.get(name, C.c_int)
    _loaded[path] = lib
    return lib


def check(rc, last_error):
    """Raises MldsaError with the library's message (last_error: its mldsa_*_last_error) unless rc is OK."""
    if rc != _lib.OK:
        raise _lib.MldsaError(rc, last_error().decode(errors="replace"))
