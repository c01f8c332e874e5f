"""The seed-form key library (include/mldsa_seed.h, fips204_amd/seed/libmldsa_seed.so) without a device: that a clean build produces it
and leaves the core untouched, its C ABI, how it is linked against the core, its scratch formulas, its host-only argument checks, its
kernels' resources and sources, and the host helper private_key_forms."""
import os

import pytest

from fips204_amd import _lib, _seed_lib
from layer_checks import (KL, PK_SK, ROOT, aligned_buffer, built, clean_build, core_params, header_and_exports,
                          includes_the_core_device_headers, kernel_resources, layered_on_core, scratch_sweep, sources_clean)

SEED_DIR = os.path.join(ROOT, "fips204_amd", "seed")


@pytest.fixture(scope="module")
def seed():
    return built(_seed_lib, SEED_DIR)


def test_a_clean_build_of_the_layer_produces_the_library_and_leaves_the_core_alone(seed, tmp_path):
    from fips204_amd import build
    assert build.SEED_LIB == _seed_lib.LIB_PATH
    clean_build("seed", _seed_lib, ("Makefile", "seed.hip"), (build.LIB, build.PH_LIB, build.KEYS_LIB, build.MU_LIB, build.SEED_LIB), tmp_path)


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(seed, tmp_path):
    declared, text = header_and_exports(
        _seed_lib, seed,
        "int main(void) { unsigned char x[MLDSA_SEED_LEN]; x[0] = 0;\n"
        "  return mldsa_seed_abi_version() == MLDSA_SEED_ABI_VERSION && mldsa_seed_sign_scratch_bytes(MLDSA_65, 1) > x[0] ? 0 : 1; }\n",
        r"\b(mldsa_seed_[a-z0-9_]+|mldsa_sign_seed)\s*\(", tmp_path)
    assert {"mldsa_seed_expand", "mldsa_seed_check", "mldsa_sign_seed", "mldsa_seed_expand_scratch_bytes", "mldsa_seed_check_scratch_bytes",
            "mldsa_seed_sign_scratch_bytes", "mldsa_seed_abi_version", "mldsa_seed_last_error"} == declared
    assert "#define MLDSA_SEED_ABI_VERSION 1" in text and seed.mldsa_seed_abi_version() == _seed_lib.ABI_VERSION == 1
    assert "#define MLDSA_SEED_LEN 32" in text and _seed_lib.SEED_LEN == 32
    assert "#define MLDSA_SEED_MAX_KEYS ((size_t)1 << 24)" in text and _seed_lib.MAX_KEYS == 1 << 24
    # the reference crate signs from no seed: the entries cite FIPS 204; the range of the int32 outputs is stated
    assert text.count("FIPS 204") >= 3 and "Algorithm 6" in text and "lies in (-q, q)" in text


def test_layered_on_the_one_core_library(seed):
    layered_on_core(
        _seed_lib.LIB_PATH,
        # the sampling and the arithmetic are the core's seams, the check and the signer stand on its whole operations
        needs=("mldsa_expand_a", "mldsa_expand_s", "mldsa_ntt", "mldsa_mat_vec_mul", "mldsa_inv_ntt", "mldsa_to_mont", "mldsa_keygen",
               "mldsa_sign", "mldsa_memset", "mldsa_get_params", "mldsa_ctx_device", "mldsa_last_error"),
        # ... and the wire private key is never decoded or encoded here
        never=("mldsa_sk_expand", "mldsa_sk_into_bytes", "mldsa_bit_pack", "mldsa_bit_unpack"))


def _expand_formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (k * l + l + 2 * k) + 320 * k + 96)


def _check_formula(pset, n):
    return n * sum(PK_SK[pset])


def _sign_formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (l + 2 * k) + 128) + _expand_formula(pset, n)


def test_scratch_sizes_follow_the_documented_formulas(seed):
    for fn, formula in ((seed.mldsa_seed_expand_scratch_bytes, _expand_formula), (seed.mldsa_seed_check_scratch_bytes, _check_formula),
                        (seed.mldsa_seed_sign_scratch_bytes, _sign_formula)):
        scratch_sweep(fn, formula, 1 << 24)
    # the formulas are the header's
    text = open(_seed_lib.HEADER_PATH).read()
    assert "n_keys (1024 (K L + L + 2 K) + 320 K + 96)" in text
    assert "n_keys (PK_LEN + SK_LEN) = n_keys * 3872 / 5984 / 7488" in text
    assert "n_keys (1024 (L + 2 K) + 128) + expand(n_keys)" in text
    assert [sum(PK_SK[s]) for s in (44, 65, 87)] == [3872, 5984, 7488]
    core_params()


def test_argument_errors_never_abort(seed):
    null = None
    buf, p, odd = aligned_buffer()
    big = 1 << 50

    def expand(ctx=null, pset=65, xi=p, rho=p, cap_k=p, tr=p, s1=p, s2=p, t0=p, pk=null, n=4, scratch=p, sb=big, stream=null):
        return seed.mldsa_seed_expand(ctx, pset, xi, rho, cap_k, tr, s1, s2, t0, pk, n, scratch, sb, stream)

    def check(ctx=null, pset=65, xi=p, sk=p, match=p, n=4, scratch=p, sb=big, stream=null):
        return seed.mldsa_seed_check(ctx, pset, xi, sk, match, n, scratch, sb, stream)

    def sign(ctx=null, pset=65, mode=0, xi=p, n=4, kidx=null, msgs=p, moff=p, ctxs=null, coff=null, rnd=p, sigs=p, status=null, n_ops=4,
             scratch=p, sb=big, stream=null):
        return seed.mldsa_sign_seed(ctx, pset, mode, xi, n, kidx, msgs, moff, ctxs, coff, rnd, sigs, status, n_ops, scratch, sb, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call, name in ((expand, b"mldsa_seed_expand"), (check, b"mldsa_seed_check"), (sign, b"mldsa_sign_seed")):
        assert call() == _lib.ERR_PARAM
        assert b"context" in seed.mldsa_seed_last_error() and seed.mldsa_seed_last_error().startswith(name)
        assert call(n=0) == _lib.ERR_PARAM  # a NULL context is an argument error of an empty call too
    # a fake non-NULL context must still be refused before it is touched: the checks on sets, counts, pointers and scratch come first
    fake = p
    for pset in (0, 45, -65):
        for call in (expand, check, sign):
            assert call(ctx=fake, pset=pset) == _lib.ERR_PARAM and b"parameter set" in seed.mldsa_seed_last_error()
            assert call(ctx=fake, pset=pset, n=0) == _lib.ERR_PARAM
    for mode in (-1, 3, 99):
        assert sign(ctx=fake, mode=mode) == _lib.ERR_PARAM and b"mode" in seed.mldsa_seed_last_error()
    for kw in (dict(xi=null), dict(rho=null), dict(cap_k=null), dict(tr=null), dict(s1=null), dict(s2=null), dict(t0=null)):
        assert expand(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in seed.mldsa_seed_last_error(), kw
    for kw in (dict(s1=odd), dict(s2=odd), dict(t0=odd)):
        assert expand(ctx=fake, **kw) == _lib.ERR_PARAM and b"16-byte" in seed.mldsa_seed_last_error(), kw
    for kw in (dict(xi=null), dict(sk=null), dict(match=null)):
        assert check(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in seed.mldsa_seed_last_error(), kw
    for kw in (dict(xi=null), dict(moff=null), dict(rnd=null), dict(sigs=null)):
        assert sign(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in seed.mldsa_seed_last_error(), kw
    assert sign(ctx=fake, n=0) == _lib.ERR_PARAM and b"n_keys" in seed.mldsa_seed_last_error()       # no keys but ops
    assert sign(ctx=fake, n=3, n_ops=4) == _lib.ERR_PARAM and b"n_keys" in seed.mldsa_seed_last_error()  # key_idx NULL: a key per op
    for call in (expand, check, sign):
        assert call(ctx=fake, n=(1 << 24) + 1) == _lib.ERR_PARAM and b"MLDSA_SEED_MAX_KEYS" in seed.mldsa_seed_last_error()
        for kw in (dict(scratch=null), dict(scratch=odd)):
            assert call(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch" in seed.mldsa_seed_last_error(), kw
    # a scratch below the minimum -- one pass over min(n_keys, 64) keys, for the signer behind the whole table -- is MLDSA_ERR_NOMEM
    for pset in KL:
        k, l = KL[pset]
        for n in (1, 4, 64, 200):
            lo = min(n, 64)
            for sb in (0, 1, _expand_formula(pset, lo) - 1):
                assert expand(ctx=fake, pset=pset, n=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in seed.mldsa_seed_last_error()
            for sb in (0, 1, _check_formula(pset, lo) - 1):
                assert check(ctx=fake, pset=pset, n=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in seed.mldsa_seed_last_error()
            table = n * (1024 * (l + 2 * k) + 128)
            for sb in (0, table - 1, table, table + _expand_formula(pset, lo) - 1):
                assert sign(ctx=fake, pset=pset, n=n, n_ops=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in seed.mldsa_seed_last_error()
    # empty calls succeed on any context without touching it
    assert expand(ctx=fake, n=0, xi=null, rho=null, cap_k=null, tr=null, s1=null, s2=null, t0=null, scratch=null, sb=0) == _lib.OK
    assert check(ctx=fake, n=0, xi=null, sk=null, match=null, scratch=null, sb=0) == _lib.OK
    assert sign(ctx=fake, n_ops=0, n=0, xi=null, moff=null, rnd=null, sigs=null, scratch=null, sb=0) == _lib.OK
    assert sign(ctx=fake, n_ops=0, n=7, xi=null, moff=null, rnd=null, sigs=null, scratch=null, sb=0) == _lib.OK


def test_kernels_do_not_spill_and_sources_are_clean(seed):
    kernels = kernel_resources(SEED_DIR)
    for stem in ("k_seed_h", "k_seed_rows", "k_seed_t", "k_seed_tr", "k_seed_cmp"):
        assert any(stem in nm for nm in kernels), stem
    assert sum("k_seed_tr" in nm for nm in kernels) == 3  # one per parameter set
    sources_clean(SEED_DIR, ["../../include/mldsa_seed.h", "../_seed_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"])
    src = includes_the_core_device_headers(SEED_DIR, "seed.hip")
    # the comparison has one loop, whose bound is the key length, and leaves it by no other way
    cmp_src = src[src.index("void k_seed_cmp"):src.index("// ---", src.index("void k_seed_cmp"))]
    assert cmp_src.count("for (int c = lane; c < sk_vec; c += 64)") == 1 and "break" not in cmp_src and "__ballot" not in cmp_src
    assert cmp_src.count("return") == 1  # the wave-uniform bound check on the key's number


def test_private_key_forms_routes_the_three_encodings():
    from fips204_amd.ml_dsa import FORM_BOTH, FORM_EXPANDED, FORM_SEED, private_key_forms
    xi, sk = bytes(range(32)), bytes(4032)
    assert private_key_forms(seed=xi) == (FORM_SEED, "expand_seeds")
    assert private_key_forms(expanded=sk) == (FORM_EXPANDED, "sk_expand")
    assert private_key_forms(seed=xi, expanded=sk) == private_key_forms(xi, sk) == (FORM_BOTH, "check_then_expand")
    assert private_key_forms(bytearray(xi), memoryview(sk))[0] == FORM_BOTH
    assert {FORM_SEED, FORM_EXPANDED, FORM_BOTH} == {"seed", "expanded", "both"}
    with pytest.raises(ValueError):
        private_key_forms()
    for bad in (b"", xi[:31], xi + b"\0", bytes(64)):
        with pytest.raises(ValueError):
            private_key_forms(seed=bad)
        with pytest.raises(ValueError):
            private_key_forms(seed=bad, expanded=sk)
    with pytest.raises(ValueError):
        private_key_forms(expanded=b"")
    # a count is not a key: bytes(32) would be 32 zero bytes
    for bad in (32, [0] * 32, "0" * 32):
        with pytest.raises(TypeError):
            private_key_forms(seed=bad)
        with pytest.raises(TypeError):
            private_key_forms(seed=xi, expanded=bad)
    # the routes are methods of MlDsa
    from fips204_amd.ml_dsa import MlDsa
    for name in ("expand_seeds_device", "check_seeds_device", "sign_from_seeds_device", "try_sign_from_seeds", "private_keys_from_forms",
                 "private_keys_from_bytes", "seed_scratch"):
        assert callable(getattr(MlDsa, name)), name
