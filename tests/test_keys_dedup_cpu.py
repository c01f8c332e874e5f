"""The key-deduplication library (include/mldsa_keys.h, fips204_amd/keys/libmldsa_keys.so) without a device: its C ABI, how it is
linked against the core, its host-only entry points and its kernels' resources and sources."""
import ctypes as C
import os
import re

import pytest

from fips204_amd import _keys_lib, _lib
from layer_checks import (KL, PK_SK, ROOT, aligned_buffer, built, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, sources_clean)

KEYS_DIR = os.path.join(ROOT, "fips204_amd", "keys")


@pytest.fixture(scope="module")
def keys():
    return built(_keys_lib, KEYS_DIR)


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(keys, tmp_path):
    _, text = header_and_exports(
        _keys_lib, keys,
        "int main(void) { mldsa_keys_info i; i.n_rows = 0; i.route = MLDSA_KEYS_ROUTE_CACHED;\n"
        "  return mldsa_keys_abi_version() == MLDSA_KEYS_ABI_VERSION && i.route ? 0 : 1; }\n",
        r"\b(mldsa_keys_[a-z0-9_]+|mldsa_verify_pk_dedup)\s*\(", tmp_path)
    # the Python constants are the header's
    assert re.search(r"#define MLDSA_KEYS_PROBE_MAX (\d+)", text).group(1) == str(_keys_lib.PROBE_MAX)
    assert "#define MLDSA_KEYS_MAX_KEYS ((size_t)1 << 30)" in text and _keys_lib.MAX_KEYS == 1 << 30
    assert "#define MLDSA_KEYS_MAX_CACHED ((size_t)1 << 24)" in text and _keys_lib.MAX_CACHED == 1 << 24


def test_layered_on_the_one_core_library(keys):
    layered_on_core(_keys_lib.LIB_PATH, needs=("mldsa_verify_pk", "mldsa_verify_cached_a", "mldsa_pk_expand", "mldsa_expand_a", "mldsa_get_params",
                                               "mldsa_ctx_device", "mldsa_last_error"))
    links_the_core_and_never_builds_it(KEYS_DIR)


def _dedup_formula(n):
    cap = 64
    while cap < 2 * n:
        cap *= 2
    n_pad = (n + 1023) // 1024 * 1024
    return 12 * cap + 12 * n_pad + 16 * ((n_pad + 4095) // 4096)


def _r(x):
    return (x + 255) // 256 * 256


def _verify_formula(pset, n, m):
    pk_len, (k, l) = PK_SK[pset][0], KL[pset]
    return (_r(_dedup_formula(n)) + 2 * _r(4 * n) + 256 + _r(m * pk_len) + _r(32 * m) + _r(64 * m) + _r(1024 * k * m)
            + _r(1024 * k * l * m))


def test_scratch_sizes_follow_the_documented_formulas(keys):
    assert keys.mldsa_keys_abi_version() == _keys_lib.ABI_VERSION == 1
    for pset in KL:
        for n in (0, 1, 2, 31, 32, 33, 63, 64, 65, 1000, 1024, 1025, 4096, 65536, 65537, (1 << 20) + 1, 1 << 30):
            assert keys.mldsa_keys_dedup_scratch_bytes(pset, n) == _dedup_formula(n), (pset, n)
            for m in (0, 1, 7, 1024, 8192, min(n, 1 << 24)):
                assert keys.mldsa_keys_verify_scratch_bytes(pset, n, m) == _verify_formula(pset, n, m), (pset, n, m)
        # the slot table is a power of two of at least 2 n slots of 12 bytes
        assert keys.mldsa_keys_dedup_scratch_bytes(pset, 65536) >= 12 * 2 * 65536
        # too many keys / rows, or a size that does not fit: 0
        assert keys.mldsa_keys_dedup_scratch_bytes(pset, (1 << 30) + 1) == 0
        assert keys.mldsa_keys_dedup_scratch_bytes(pset, 2 ** 63) == 0
        assert keys.mldsa_keys_dedup_scratch_bytes(pset, 2 ** 64 - 1) == 0
        assert keys.mldsa_keys_verify_scratch_bytes(pset, (1 << 30) + 1, 1) == 0
        assert keys.mldsa_keys_verify_scratch_bytes(pset, 10, (1 << 24) + 1) == 0
        assert keys.mldsa_keys_verify_scratch_bytes(pset, 10, 2 ** 63) == 0
    for bad in (0, 43, 66, -1, 128):
        assert keys.mldsa_keys_dedup_scratch_bytes(bad, 10) == 0
        assert keys.mldsa_keys_verify_scratch_bytes(bad, 10, 10) == 0


def test_argument_errors_never_abort(keys):
    null = None
    seed = bytes(range(16))
    buf, p, odd = aligned_buffer()
    big = 1 << 40

    def dedup(ctx=null, pset=65, pk=p, n=4, sd=seed, bits=64, row_of=p, table=p, rows=4, n_rows=p, scratch=p, sb=big, stream=null):
        return keys.mldsa_keys_dedup(ctx, pset, pk, n, sd, bits, row_of, table, rows, n_rows, scratch, sb, stream)

    def verify(ctx=null, pset=65, mode=0, pk=p, n_keys=4, kidx=null, msgs=p, moff=p, ctxs=null, coff=null, sigs=p, ok=p, n_ops=4, sd=seed,
               bits=64, cached=4, scratch=p, sb=big, info=null, stream=null):
        return keys.mldsa_verify_pk_dedup(ctx, pset, mode, pk, n_keys, kidx, msgs, moff, ctxs, coff, sigs, ok, n_ops, sd, bits, cached, scratch,
                                          sb, info, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    assert dedup() == _lib.ERR_PARAM and b"context" in keys.mldsa_keys_last_error()
    assert verify() == _lib.ERR_PARAM and b"context" in keys.mldsa_keys_last_error()
    for pset in (0, 45, -65):
        assert dedup(pset=pset) == _lib.ERR_PARAM and b"parameter set" in keys.mldsa_keys_last_error()
        assert verify(pset=pset) == _lib.ERR_PARAM and b"parameter set" in keys.mldsa_keys_last_error()
    for bits in (0, -1, 65, 1 << 20):
        assert dedup(bits=bits) == _lib.ERR_PARAM and b"hash_bits" in keys.mldsa_keys_last_error()
        assert verify(bits=bits) == _lib.ERR_PARAM and b"hash_bits" in keys.mldsa_keys_last_error()
        assert verify(bits=bits, n_ops=0) == _lib.ERR_PARAM
    assert dedup(n=(1 << 30) + 1) == _lib.ERR_PARAM
    # a live context is needed to get further: a fake non-NULL one must still be refused before it is touched, because the checks on
    # pointers, alignment and scratch come before the first use of the context
    fake = p
    for kw in (dict(pk=null), dict(sd=null), dict(row_of=null), dict(n_rows=null), dict(table=null, rows=1)):
        assert dedup(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in keys.mldsa_keys_last_error(), kw
    for kw in (dict(pk=odd), dict(table=odd)):
        assert dedup(ctx=fake, **kw) == _lib.ERR_PARAM and b"aligned" in keys.mldsa_keys_last_error(), kw
    need = keys.mldsa_keys_dedup_scratch_bytes(65, 4)
    for kw in (dict(scratch=null), dict(scratch=odd), dict(sb=need - 1), dict(sb=0)):
        assert dedup(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch" in keys.mldsa_keys_last_error(), kw
    for kw in (dict(pk=null), dict(moff=null), dict(sigs=null), dict(ok=null), dict(sd=null)):
        assert verify(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in keys.mldsa_keys_last_error(), kw
    for mode in (-1, 3, 99):  # refused before anything is launched, as the core does
        assert verify(ctx=fake, mode=mode) == _lib.ERR_PARAM and b"mode" in keys.mldsa_keys_last_error(), mode
    assert verify(ctx=fake, n_keys=3) == _lib.ERR_PARAM and b"cover" in keys.mldsa_keys_last_error()
    assert verify(ctx=fake, n_keys=0, kidx=p) == _lib.ERR_PARAM and b"cover" in keys.mldsa_keys_last_error()
    assert verify(ctx=fake, pk=odd) == _lib.ERR_PARAM and b"aligned" in keys.mldsa_keys_last_error()
    assert verify(ctx=fake, cached=(1 << 24) + 1) == _lib.ERR_PARAM
    assert verify(ctx=fake, n_ops=(1 << 30) + 1, n_keys=(1 << 30) + 1) == _lib.ERR_PARAM
    need = keys.mldsa_keys_verify_scratch_bytes(65, 4, 4)
    assert need > 0
    for kw in (dict(scratch=null), dict(scratch=C.c_void_p(p.value + 16)), dict(sb=need - 1), dict(sb=0)):
        assert verify(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch" in keys.mldsa_keys_last_error(), kw
    # with key_idx the scratch covers max(n_keys, n_ops)
    assert verify(ctx=fake, kidx=p, n_keys=2, n_ops=5000, sb=keys.mldsa_keys_verify_scratch_bytes(65, 5000, 4) - 1) == _lib.ERR_PARAM
    # empty calls succeed without a context
    assert verify(n_ops=0, pk=null, moff=null, sigs=null, ok=null, scratch=null, sb=0) == _lib.OK
    assert dedup(n=0, pk=null, row_of=null, table=null, rows=0, n_rows=null, scratch=null, sb=0) == _lib.OK


def test_kernels_do_not_spill_and_sources_are_clean(keys):
    # registers and shuffles do everything here: no LDS either
    assert len(kernel_resources(KEYS_DIR, lds_zero=True)) >= 13  # claim, confirm, gather for three key lengths; count, offsets, rank; compose
    # scalar-memory stores, scalar atomics, scalar-cache write-back / discard (spelled in pieces so that this file holds none of them)
    sp = "s" + "_"
    words = [sp + w for w in ("st" + "ore", "buffer_" + "st" + "ore", "scratch_" + "st" + "ore", "ato" + "mic", "buffer_" + "ato" + "mic",
                              "dca" + "che_wb", "dca" + "che_discard")]
    scalar_mem = re.compile("|".join(re.escape(w) for w in words), re.I)
    for f, t in sources_clean(KEYS_DIR, ["../../include/mldsa_keys.h", "../_keys_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]):
        assert not scalar_mem.search(t), f
