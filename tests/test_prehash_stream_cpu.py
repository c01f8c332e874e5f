"""The incremental pre-hash and the host-memory HashML-DSA entry points of libmldsa_ph.so without a device: their C ABI, the
argument errors that must come before any launch, the kernels' resource files, and the generator of the GPU test's inputs
against hashlib."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import ph_stream_cases as cases
from fips204_amd import _lib, _ph_lib
from layer_checks import ROOT, built, compiles_as_c99, declared, exported, kernel_resources

PH_DIR = os.path.join(ROOT, "fips204_amd", "ph")
NEW = ("mldsa_ph_state_bytes", "mldsa_ph_init", "mldsa_ph_update", "mldsa_ph_final", "mldsa_ph_host_create", "mldsa_ph_host_destroy",
       "mldsa_hash_verify_host", "mldsa_hash_sign_host")


@pytest.fixture(scope="module")
def ph():
    return built(_ph_lib, PH_DIR)


def test_new_names_are_exported_declared_and_listed(ph, tmp_path):
    in_library, in_header = exported(_ph_lib.LIB_PATH), declared(_ph_lib.HEADER_PATH, r"\b(mldsa_[a-z0-9_]+)\s*\(")
    for name in NEW:
        assert name in in_library, name
        assert name in in_header, name
        assert name in _ph_lib._SIGNATURES, name
    assert ph.mldsa_ph_abi_version() == 1  # additive: the version stays
    # strict C99, and the new declarations are usable from C
    compiles_as_c99('#include "mldsa_ph.h"\n'
                    "int main(void) { mldsa_ph_host *h = 0; mldsa_ph_host_destroy(h);\n"
                    "  return mldsa_ph_state_bytes(MLDSA_PH_SHA512, 1) > 0 && mldsa_ph_init(0, 0, 0, 0, 0, 0) == MLDSA_OK ? 0 : 1; }\n", tmp_path)


def test_state_bytes(ph):
    for p in (0, 1, 2):
        prev = 0
        for n in (1, 2, 63, 64, 65, 4096, 65536, 1 << 20, 1 << 32):
            b = ph.mldsa_ph_state_bytes(p, n)
            assert b > 0 and b >= prev, (p, n, b)
            prev = b
        # chaining value + byte count + a partial block (SHAKE128: the sponge alone) per op, at the least
        least = {0: 32 + 8 + 63, 1: 64 + 8 + 127, 2: 200 + 8}[p]
        assert ph.mldsa_ph_state_bytes(p, 1000) >= 1000 * least
        assert ph.mldsa_ph_state_bytes(p, 2 ** 63) == 0 and ph.mldsa_ph_state_bytes(p, 2 ** 64 - 1) == 0  # does not fit a size_t
    assert ph.mldsa_ph_state_bytes(3, 10) == 0 and ph.mldsa_ph_state_bytes(-1, 10) == 0


def test_argument_errors_come_before_any_launch(ph):
    null = None
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    fake_ctx = p  # never dereferenced: every call below fails on an earlier check or is an empty call
    calls = {
        "init": lambda ctx, code, st, nb, n: ph.mldsa_ph_init(ctx, code, st, nb, n, null),
        "update": lambda ctx, code, st, nb, n: ph.mldsa_ph_update(ctx, code, st, nb, p, p, n, null),
        "final": lambda ctx, code, st, nb, n: ph.mldsa_ph_final(ctx, code, st, nb, p, null, null, n, null),
    }
    for name, call in calls.items():
        assert call(null, 0, p, 4096, 1) == _lib.ERR_PARAM and b"context" in ph.mldsa_ph_last_error(), name
        assert call(fake_ctx, 3, p, 4096, 1) == _lib.ERR_PARAM and b"unknown ph" in ph.mldsa_ph_last_error(), name
        assert call(fake_ctx, -1, p, 4096, 1) == _lib.ERR_PARAM, name
        assert call(fake_ctx, 0, null, 4096, 1) == _lib.ERR_PARAM and b"state" in ph.mldsa_ph_last_error(), name
        for code in (0, 1, 2):
            need = ph.mldsa_ph_state_bytes(code, 4)
            assert call(fake_ctx, code, p, need - 1, 4) == _lib.ERR_PARAM and b"state" in ph.mldsa_ph_last_error(), (name, code)
        assert call(fake_ctx, 0, C.c_void_p(p.value + 2), 4000, 1) == _lib.ERR_PARAM, name  # misaligned
        assert call(fake_ctx, 0, p, 4096, 2 ** 63) == _lib.ERR_PARAM, name                   # a size that does not fit
        # n_ops = 0 is a successful empty call, whatever the pointers
        assert call(null, 0, null, 0, 0) == _lib.OK and call(null, 2, null, 0, 0) == _lib.OK, name
        assert call(null, 9, null, 0, 0) == _lib.ERR_PARAM, name


def test_host_object_and_host_calls_refuse_without_a_device(ph):
    out = C.c_void_p(0x1234)
    assert ph.mldsa_ph_host_create(None, 0, C.byref(out)) == _lib.ERR_PARAM and ph.mldsa_ph_last_error()
    assert not out.value  # no half-made object is handed out
    buf = (C.c_uint8 * 64)()
    assert ph.mldsa_ph_host_create(C.cast(buf, C.c_void_p), 0, None) == _lib.ERR_PARAM
    ph.mldsa_ph_host_destroy(None)  # no-op
    p = C.cast(buf, C.c_void_p)
    off = (C.c_uint64 * 2)(0, 8)
    po = C.cast(off, C.c_void_p)
    assert ph.mldsa_hash_verify_host(None, 44, 0, p, 1, None, p, po, None, None, p, p, 1) == _lib.ERR_PARAM
    assert ph.mldsa_hash_sign_host(None, 44, 0, p, 1, None, p, po, None, None, p, p, None, 1) == _lib.ERR_PARAM
    assert ph.mldsa_hash_verify_host(None, 44, 5, p, 1, None, p, po, None, None, p, p, 1) == _lib.ERR_PARAM
    assert b"unknown ph" in ph.mldsa_ph_last_error()
    assert ph.mldsa_hash_verify_host(None, 44, 0, *([None] * 1), 0, *([None] * 7), 0) == _lib.OK
    assert ph.mldsa_hash_sign_host(None, 44, 1, None, 0, *([None] * 8), 0) == _lib.OK


def test_res_files_name_the_new_kernels(ph):
    names = kernel_resources(PH_DIR)  # no kernel of the layer spills or uses scratch, the new ones among them
    for kernel in ("k_ph_init", "k_ph_update", "k_ph_final"):
        mine = [n for n in names if kernel in n]
        assert len(mine) == 3, (kernel, mine)  # one per PH


@pytest.mark.parametrize("ph_name", cases.PHS)
def test_generator_meets_its_coverage_conditions(ph_name):
    """the conditions test_gpu_prehash_stream.py asserts on its inputs, checked with hashlib alone: the schedules cut the messages
    without losing a byte, and they reach every head / tail case of the update kernel"""
    msgs = cases.seam_messages()
    sched = cases.schedules(msgs, ph_name)
    assert len(sched) == 1 + 9 + 1 + 3
    cov = cases.coverage(msgs, sched, ph_name)
    for key in ("tail_block_minus_1", "completes_exactly", "completes_then_2_blocks", "final_update_empty", "empty_piece", "one_byte"):
        assert cov[key] >= 1, (ph_name, key, cov)
    new = {"SHA256": hashlib.sha256, "SHA512": hashlib.sha512, "SHAKE128": hashlib.shake_128}[ph_name]
    whole = [new(m).digest(32) if ph_name == "SHAKE128" else new(m).digest() for m in msgs]
    for name, (ops, cuts) in sched.items():
        assert len({len(c) for c in cuts}) == 1, name  # every op of a schedule has the same number of pieces
        if name == "bytes":
            assert ops and all(len(msgs[i]) <= 300 for i in ops) and len(cuts[0]) == 301
        got = cases.hashlib_incremental(msgs, ops, cuts, ph_name)
        assert got == [whole[i] for i in ops], name


def test_vectorised_piece_gather():
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 50, 200)
    off = np.zeros(201, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    for U in (1, 3, 16):
        cuts = cases.random_cuts(lens, U, rng)
        assert cuts.shape == (200, U + 1) and (np.diff(cuts, axis=1) >= 0).all() and (cuts[:, -1] == lens).all()
        back = [b""] * 200
        for u in range(U):
            flat, poff = cases.gather_pieces(buf, off, cuts, u)
            for i in range(200):
                back[i] += flat[int(poff[i]):int(poff[i + 1])].tobytes()
        assert back == [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(200)]
