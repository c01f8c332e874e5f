"""The pre-hash library (include/mldsa_ph.h, fips204_amd/ph/libmldsa_ph.so) without a device: its C ABI, how it is linked
against the core, its host-only entry points and its kernels' resources and sources."""
import ctypes as C
import os
import re

import pytest

from fips204_amd import _lib, _ph_lib
from layer_checks import ROOT, built, header_and_exports, kernel_resources, layered_on_core, sources_clean

PH_DIR = os.path.join(ROOT, "fips204_amd", "ph")


@pytest.fixture(scope="module")
def ph():
    return built(_ph_lib, PH_DIR)


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(ph, tmp_path):
    header_and_exports(_ph_lib, ph, "int main(void) { return mldsa_ph_row_len(MLDSA_PH_SHA256) == 43 ? 0 : 1; }\n",
                       r"\b(mldsa_ph_[a-z0-9_]+|mldsa_prehash|mldsa_hash_[a-z0-9_]+)\s*\(", tmp_path)


def test_layered_on_the_one_core_library(ph):
    layered_on_core(_ph_lib.LIB_PATH)


def test_host_entry_points(ph):
    assert ph.mldsa_ph_abi_version() == _ph_lib.ABI_VERSION == 1
    assert [ph.mldsa_ph_row_len(p) for p in (0, 1, 2)] == [43, 75, 43]
    assert ph.mldsa_ph_row_len(3) < 0 and ph.mldsa_ph_row_len(-1) < 0
    for p in (0, 1, 2):
        rl = ph.mldsa_ph_row_len(p)
        prev = 0
        for n in (0, 1, 2, 63, 64, 65, 4096, 65536, 1 << 20):
            b = ph.mldsa_ph_scratch_bytes(p, n)
            assert b >= n * rl + 8 * (n + 1) and b >= prev, (p, n, b)
            prev = b
    assert ph.mldsa_ph_scratch_bytes(3, 10) == 0 and ph.mldsa_ph_scratch_bytes(-1, 10) == 0
    assert ph.mldsa_ph_scratch_bytes(0, 2 ** 63) == 0  # does not fit a size_t


def test_argument_errors_never_abort(ph):
    null = None
    # NULL context, NULL pointers, an unknown ph: an error code and a message, no launch, no abort
    rc = ph.mldsa_hash_verify(null, 44, 0, null, null, null, 1, null, null, null, null, null, null, null, 1, null, 0, null)
    assert rc == _lib.ERR_PARAM and ph.mldsa_ph_last_error()
    rc = ph.mldsa_hash_verify_pk(null, 44, 0, null, 1, null, null, null, null, null, null, null, 1, null, 0, null)
    assert rc == _lib.ERR_PARAM
    rc = ph.mldsa_hash_sign(null, 44, 0, *([null] * 6), 1, null, null, null, null, null, null, null, null, 1, null, 0, null)
    assert rc == _lib.ERR_PARAM
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = ph.mldsa_hash_verify(null, 44, 0, p, p, p, 1, null, p, p, null, null, p, p, 1, p, 64, null)
    assert rc == _lib.ERR_PARAM and b"context" in ph.mldsa_ph_last_error()
    rc = ph.mldsa_hash_verify(null, 44, 7, p, p, p, 1, null, p, p, null, null, p, p, 1, p, 64, null)
    assert rc == _lib.ERR_PARAM and b"unknown ph" in ph.mldsa_ph_last_error()
    assert ph.mldsa_prehash(null, 0, p, p, p, null, 1, null) == _lib.ERR_PARAM
    assert ph.mldsa_prehash(null, 5, p, p, p, null, 1, null) == _lib.ERR_PARAM
    # n_ops = 0 is a successful empty call
    assert ph.mldsa_prehash(null, 0, null, null, null, null, 0, null) == _lib.OK
    assert ph.mldsa_hash_verify(null, 44, 1, *([null] * 3), 0, *([null] * 7), 0, null, 0, null) == _lib.OK


def test_kernels_do_not_spill_and_sources_are_clean(ph):
    assert len(kernel_resources(PH_DIR)) >= 4  # k_prehash for three PH, k_ph_refuse
    # scalar-memory stores, scalar atomics, scalar-cache write-back / discard (spelled in pieces so that this file holds none of them)
    sp = "s" + "_"
    words = [sp + w for w in ("st" + "ore", "buffer_" + "st" + "ore", "scratch_" + "st" + "ore", "ato" + "mic", "buffer_" + "ato" + "mic",
                              "dca" + "che_wb", "dca" + "che_discard")]
    scalar_mem = re.compile("|".join(re.escape(w) for w in words), re.I)
    # sha2_dev.h pins its round constants to scalar registers with an empty asm statement: the one layer that is not plain C++ throughout
    for f, t in sources_clean(PH_DIR, ["../../include/mldsa_ph.h"], asm_free=False):
        assert not scalar_mem.search(t), f
