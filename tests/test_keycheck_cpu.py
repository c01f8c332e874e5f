"""The strict private-key import library (include/mldsa_keycheck.h, fips204_amd/keycheck/libmldsa_keycheck.so) without a device: that a
clean build produces it and leaves the core untouched, its C ABI, how it is linked against the core, its scratch formula, its host-only
argument checks, its kernels' resources and sources -- and the expected verdicts the device tests compare against: the restatement of
tests/keycheck_cases.py on the ACVP keyGen vectors and on every damage class, and the host helper private_key_faults against a second
decode."""
import os
import re

import numpy as np
import pytest

import keycheck_cases as kc
from fips204_amd import _keycheck_lib, _lib
from layer_checks import (KL, ROOT, aligned_buffer, built, clean_build, core_params, header_and_exports, includes_the_core_device_headers,
                          kernel_resources, layered_on_core, scratch_sweep, sources_clean)

KC_DIR = os.path.join(ROOT, "fips204_amd", "keycheck")
EXPORTS = {"mldsa_keycheck_abi_version", "mldsa_keycheck_last_error", "mldsa_keycheck_scratch_bytes", "mldsa_sk_range_check",
           "mldsa_keypair_check", "mldsa_sk_import"}


@pytest.fixture(scope="module")
def keycheck():
    return built(_keycheck_lib, KC_DIR)


def test_a_clean_build_of_the_layer_produces_the_library_and_leaves_the_core_alone(keycheck, tmp_path):
    from fips204_amd import build
    assert build.KEYCHECK_LIB == _keycheck_lib.LIB_PATH
    clean_build("keycheck", _keycheck_lib, ("Makefile", "keycheck.hip"),
                (build.LIB, build.PH_LIB, build.KEYS_LIB, build.MU_LIB, build.SEED_LIB, build.KEYCHECK_LIB), tmp_path)


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(keycheck, tmp_path):
    declared, text = header_and_exports(
        _keycheck_lib, keycheck,
        "int main(void) { unsigned char x[MLDSA_KEY_PK]; x[0] = MLDSA_KEY_S1_RANGE | MLDSA_KEY_S2_RANGE | MLDSA_KEY_T0 | MLDSA_KEY_TR;\n"
        "  return mldsa_keycheck_abi_version() == MLDSA_KEYCHECK_ABI_VERSION && MLDSA_KEYCHECK_RANGE != MLDSA_KEYCHECK_PAIR\n"
        "         && mldsa_keycheck_scratch_bytes(MLDSA_65, 1) > x[0] && MLDSA_KEYCHECK_MAX_KEYS > 1 ? 0 : 1; }\n",
        r"\b(mldsa_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == EXPORTS
    assert "#define MLDSA_KEYCHECK_ABI_VERSION 1" in text and keycheck.mldsa_keycheck_abi_version() == _keycheck_lib.ABI_VERSION == 1
    assert "#define MLDSA_KEYCHECK_MAX_KEYS ((size_t)1 << 24)" in text and _keycheck_lib.MAX_KEYS == 1 << 24
    for name, value in (("MLDSA_KEY_S1_RANGE", 1), ("MLDSA_KEY_S2_RANGE", 2), ("MLDSA_KEY_T0", 4), ("MLDSA_KEY_TR", 8), ("MLDSA_KEY_PK", 16),
                        ("MLDSA_KEYCHECK_RANGE", _keycheck_lib.LEVEL_RANGE), ("MLDSA_KEYCHECK_PAIR", _keycheck_lib.LEVEL_PAIR)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert (_keycheck_lib.KEY_S1_RANGE, _keycheck_lib.KEY_S2_RANGE, _keycheck_lib.KEY_T0, _keycheck_lib.KEY_TR, _keycheck_lib.KEY_PK) == \
        (kc.S1_RANGE, kc.S2_RANGE, kc.T0, kc.TR, kc.PK) == (1, 2, 4, 8, 16)
    # the reference has no such interface: the entries cite FIPS 204, never crate lines
    assert text.count("FIPS 204") >= 3 and "Algorithm 25" in text and "Algorithm 35" in text and not re.search(r"\bsrc/\w+\.rs", text)


def test_layered_on_the_one_core_library(keycheck):
    layered_on_core(
        _keycheck_lib.LIB_PATH,
        # the sampling, A s1 and the import itself are the core's; A s1 comes from the fused kernel, not from the three seams
        needs=("mldsa_expand_a", "mldsa_verify_arith", "mldsa_sk_expand", "mldsa_memset", "mldsa_get_params", "mldsa_ctx_device",
               "mldsa_last_error"),
        never=("mldsa_ntt", "mldsa_mat_vec_mul", "mldsa_inv_ntt", "mldsa_keygen", "mldsa_bit_unpack", "mldsa_get_public_key"))


def _formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (k * l + l + 2 * k + 1) + 320 * k + 48)


def test_scratch_size_follows_the_documented_formula(keycheck):
    scratch_sweep(keycheck.mldsa_keycheck_scratch_bytes, _formula, 1 << 24)
    # the formula is the header's
    text = open(_keycheck_lib.HEADER_PATH).read()
    assert "n_keys (1024 (K L + L + 2 K + 1) + 320 K + 48) = n_keys * 31024 / 51120 / 84528" in text
    assert [_formula(s, 1) for s in (44, 65, 87)] == [31024, 51120, 84528]
    for pset, p in core_params().items():
        y = kc.Layout(pset)
        assert (p.pk_len, p.sk_len, p.eta) == (y.pk_len, y.sk_len, y.eta)
        # what the layout and the 16-byte loads rely on: every section of a key and every part of the scratch starts on a multiple of 16
        assert _formula(pset, 1) % 16 == 0
        assert y.s1 % 16 == 0 and y.s2 % 16 == 0 and y.t0 % 16 == 0 and (32 * y.b) % 16 == 0


def test_argument_errors_never_abort(keycheck):
    null = None
    buf, p, odd = aligned_buffer()
    big = 1 << 50
    err = keycheck.mldsa_keycheck_last_error

    def rng(ctx=null, pset=65, sk=p, flag=p, n=4, stream=null):
        return keycheck.mldsa_sk_range_check(ctx, pset, sk, flag, n, stream)

    def pair(ctx=null, pset=65, sk=p, pk=null, flag=p, n=4, scratch=p, sb=big, stream=null):
        return keycheck.mldsa_keypair_check(ctx, pset, sk, pk, flag, n, scratch, sb, stream)

    def imp(ctx=null, pset=65, level=_keycheck_lib.LEVEL_PAIR, sk=p, pk=null, rho=p, cap_k=p, tr=p, s1=p, s2=p, t0=p, flag=p, n=4, scratch=p,
            sb=big, stream=null):
        return keycheck.mldsa_sk_import(ctx, pset, level, sk, pk, rho, cap_k, tr, s1, s2, t0, flag, n, scratch, sb, stream)

    calls = ((rng, b"mldsa_sk_range_check"), (pair, b"mldsa_keypair_check"), (imp, b"mldsa_sk_import"))
    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call, name in calls:
        assert call() == _lib.ERR_PARAM
        assert b"context" in err() and err().startswith(name)
        assert call(n=0) == _lib.ERR_PARAM  # a NULL context is an argument error of an empty call too
    # a fake non-NULL context must still be refused before it is touched: the checks on sets, counts, pointers and scratch come first
    fake = p
    for pset in (0, 45, -65):
        for call, _ in calls:
            assert call(ctx=fake, pset=pset) == _lib.ERR_PARAM and b"parameter set" in err()
            assert call(ctx=fake, pset=pset, n=0) == _lib.ERR_PARAM
    for level in (0, 3, -1, 99):
        assert imp(ctx=fake, level=level) == _lib.ERR_PARAM and b"level" in err()
        assert imp(ctx=fake, level=level, n=0) == _lib.ERR_PARAM
    for call, _ in calls:
        assert call(ctx=fake, n=(1 << 24) + 1) == _lib.ERR_PARAM and b"MLDSA_KEYCHECK_MAX_KEYS" in err()
        for kw in (dict(sk=null), dict(flag=null)):
            assert call(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in err(), kw
    for level in (_keycheck_lib.LEVEL_RANGE, _keycheck_lib.LEVEL_PAIR):
        for kw in (dict(rho=null), dict(cap_k=null), dict(tr=null), dict(s1=null), dict(s2=null), dict(t0=null)):
            assert imp(ctx=fake, level=level, **kw) == _lib.ERR_PARAM and b"NULL" in err(), kw
        for kw in (dict(s1=odd), dict(s2=odd), dict(t0=odd)):
            assert imp(ctx=fake, level=level, **kw) == _lib.ERR_PARAM and b"16-byte" in err(), kw
    for call in (pair, imp):
        for kw in (dict(scratch=null), dict(scratch=odd)):
            assert call(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch" in err(), kw
    # a scratch below the minimum -- one pass over min(n_keys, 64) keys -- is MLDSA_ERR_NOMEM
    for pset in KL:
        for n in (1, 4, 64, 65, 200):
            for sb in (0, 1, _formula(pset, min(n, 64)) - 1):
                for call in (pair, imp):
                    assert call(ctx=fake, pset=pset, n=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in err()
    # empty calls succeed on any context without touching it
    assert rng(ctx=fake, n=0, sk=null, flag=null) == _lib.OK
    assert pair(ctx=fake, n=0, sk=null, flag=null, scratch=null, sb=0) == _lib.OK
    for level in (_keycheck_lib.LEVEL_RANGE, _keycheck_lib.LEVEL_PAIR):
        assert imp(ctx=fake, level=level, n=0, sk=null, rho=null, cap_k=null, tr=null, s1=null, s2=null, t0=null, flag=null, scratch=null,
                   sb=0) == _lib.OK


def test_kernels_do_not_spill_and_sources_are_clean(keycheck):
    kernels = kernel_resources(KC_DIR)
    for stem in ("k_kc_range", "k_kc_s1", "k_kc_row", "k_kc_tr", "k_kc_merge", "k_kc_wipe"):
        assert any(stem in nm for nm in kernels), stem
    assert sum("k_kc_tr" in nm for nm in kernels) == 3     # one per parameter set (K = 4, 6, 8)
    assert sum("k_kc_range" in nm for nm in kernels) == 2  # 3-bit fields (ML-DSA-44 and 87) and 4-bit fields (ML-DSA-65)
    sources_clean(KC_DIR, ["../../include/mldsa_keycheck.h", "../_keycheck_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"])
    src = includes_the_core_device_headers(KC_DIR, "keycheck.hip")
    # the range kernel has one loop, whose bound is the parameter set's, and leaves it by no other way; neither it nor the row kernel
    # asks the wave what its lanes found before the verdict byte
    rng_src = src[src.index("void k_kc_range"):src.index("// ---", src.index("void k_kc_range"))]
    assert rng_src.count("for (int u = lane; u < n_units; u += 64)") == 1 and "break" not in rng_src and "__ballot" not in rng_src
    assert rng_src.count("return") == 1  # the wave-uniform bound check on the key's number
    row_src = src[src.index("void k_kc_row"):src.index("// ---", src.index("void k_kc_row"))]
    assert "break" not in row_src and "__ballot" not in row_src and row_src.count("return") == 1


# ------------------------------------------------------------------------------------------ the expected values themselves
@pytest.mark.parametrize("pset", kc.SETS)
def test_restatement_accepts_every_acvp_keygen_pair(pset):
    pairs = kc.acvp_pairs(pset)
    assert len(pairs) == 25
    for i, (sk, pk) in enumerate(pairs):
        assert kc.expected_flags(pset, sk, pk) == 0 and kc.expected_flags(pset, sk) == 0, (pset, i)
    # and a pair from two different keys is a PK fault only
    assert kc.expected_flags(pset, pairs[0][0], pairs[1][1]) == kc.PK


@pytest.mark.parametrize("pset", kc.SETS)
def test_restatement_gives_the_stated_bits_for_every_damage_class(pset):
    y = kc.Layout(pset)
    for sk0, pk0 in kc.acvp_pairs(pset)[:3]:
        cases = kc.damage_cases(pset, sk0, pk0)
        assert {c[0][0] for c in cases} == set("abcdefg")
        assert sum(c[0][0] == "a" for c in cases) == sum(c[0][0] == "b" for c in cases) == (16 if y.b == 3 else 8)
        for name, sk, pk, stated in cases:
            without, with_pk = kc.expected_flags(pset, sk), kc.expected_flags(pset, sk, pk)
            if stated is not None:
                assert (without, with_pk) == stated, (pset, name)
            else:  # b: a legal field never sets a range bit; the consistency bits are the restatement's
                assert not without & 3 and not with_pk & 3, (pset, name)
                assert with_pk & ~kc.PK == without and (sk != sk0 or with_pk == 0), (pset, name)
            assert without in (0, 1, 2, 3) or not without & 3


def _faults_by_big_integers(pset, sk):
    """a second, independent decode: the s1 | s2 region as one Python integer, sliced field by field"""
    y = kc.Layout(pset)
    region = int.from_bytes(sk[128:y.t0], "little")
    mask = (1 << y.b) - 1
    out = 0
    for c in range((y.l + y.k) * 256):
        if (region >> (y.b * c)) & mask > 2 * y.eta:
            out |= kc.S1_RANGE if c < y.l * 256 else kc.S2_RANGE
    return out


@pytest.mark.parametrize("pset", kc.SETS)
def test_private_key_faults_agrees_with_a_second_decode(pset):
    from fips204_amd.ml_dsa import private_key_faults
    y = kc.Layout(pset)
    sk0, pk0 = kc.acvp_pairs(pset)[0]
    rows = [sk0] + [c[1] for c in kc.damage_cases(pset, sk0, pk0)]
    both = kc.set_field(kc.set_field(sk0, y, "s1", 1, 100, 2 * y.eta + 1), y, "s2", 2, 31, (1 << y.b) - 1)
    rows += [both, bytes(y.sk_len), bytes([0xFF]) * y.sk_len]
    want = [_faults_by_big_integers(pset, r) for r in rows]
    assert want[0] == 0 and want[-3:] == [3, 0, 3] and set(want) == {0, 1, 2, 3}
    # a list of keys, one array, one key
    assert private_key_faults(pset, rows).tolist() == want
    assert private_key_faults(pset, np.frombuffer(b"".join(rows), dtype=np.uint8)).tolist() == want
    assert private_key_faults(pset, rows[1]).tolist() == want[1:2]
    # ... which is the range part of the restatement
    assert [kc.expected_flags(pset, r) & 3 for r in rows] == want
    with pytest.raises(ValueError):
        private_key_faults(pset, sk0[:-1])
    with pytest.raises(ValueError):
        private_key_faults(45, sk0)
