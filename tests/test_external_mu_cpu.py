"""The external-mu library (include/mldsa_mu.h, fips204_amd/mu/libmldsa_mu.so) without a device: its C ABI, how it is linked against
the core, its host-only entry points, its kernels' resources and sources, and the host helper external_mu."""
import hashlib
import os

import pytest

from fips204_amd import _lib, _mu_lib
from layer_checks import (KL, ROOT, aligned_buffer, built, header_and_exports, includes_the_core_device_headers, kernel_resources,
                          layered_on_core, links_the_core_and_never_builds_it, scratch_sweep, sources_clean)

MU_DIR = os.path.join(ROOT, "fips204_amd", "mu")


@pytest.fixture(scope="module")
def mu():
    return built(_mu_lib, MU_DIR)


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(mu, tmp_path):
    declared, text = header_and_exports(
        _mu_lib, mu,
        "int main(void) { unsigned char m[MLDSA_MU_LEN]; m[0] = 0;\n"
        "  return mldsa_mu_abi_version() == MLDSA_MU_ABI_VERSION && mldsa_mu_sign_scratch_bytes(MLDSA_65, 1) > m[0] ? 0 : 1; }\n",
        r"\b(mldsa_mu_[a-z0-9_]+|mldsa_verify_mu|mldsa_sign_mu)\s*\(", tmp_path)
    assert {"mldsa_mu_compute", "mldsa_verify_mu", "mldsa_sign_mu", "mldsa_mu_verify_scratch_bytes", "mldsa_mu_sign_scratch_bytes"} <= declared
    assert "#define MLDSA_MU_LEN 64" in text and _mu_lib.MU_LEN == 64
    assert "#define MLDSA_MU_MAX_OPS ((size_t)1 << 30)" in text and _mu_lib.MAX_OPS == 1 << 30
    # the reference crate has no external-mu interface: the entries cite FIPS 204
    assert text.count("FIPS 204") >= 4 and "Algorithm 7" in text and "Algorithm 8" in text


def test_layered_on_the_one_core_library(mu):
    layered_on_core(
        _mu_lib.LIB_PATH,
        # the arithmetic and the codecs are the core's seams
        needs=("mldsa_sig_decode", "mldsa_sample_in_ball", "mldsa_expand_a", "mldsa_verify_arith", "mldsa_infinity_norm", "mldsa_expand_mask",
               "mldsa_ntt", "mldsa_inv_ntt", "mldsa_mat_vec_mul", "mldsa_pointwise_mont", "mldsa_sig_encode", "mldsa_get_params",
               "mldsa_ctx_device", "mldsa_last_error"),
        # ... and the op-level calls, which take messages, are not what it stands on
        never=("mldsa_verify", "mldsa_sign", "mldsa_rounding", "mldsa_w1_encode", "mldsa_xof"))
    links_the_core_and_never_builds_it(MU_DIR)
    from fips204_amd import build
    assert build.MU_LIB == _mu_lib.LIB_PATH


def _verify_formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (k * l + 3 * k + l + 1) + 128)


def _sign_formula(pset, n):
    k, l = KL[pset]
    return 256 + n * (1024 * (k * l + 5 * l + 6 * k + 1) + 400) + (n + 1) // 2 * (1024 * k * l + 192)


def test_scratch_sizes_follow_the_documented_formulas(mu):
    assert mu.mldsa_mu_abi_version() == _mu_lib.ABI_VERSION == 1
    scratch_sweep(mu.mldsa_mu_verify_scratch_bytes, _verify_formula, 1 << 30)
    scratch_sweep(mu.mldsa_mu_sign_scratch_bytes, _sign_formula, 1 << 30)
    # the formulas are the header's
    text = open(_mu_lib.HEADER_PATH).read()
    assert "n_ops (1024 (K L + 3 K + L + 1) + 128)" in text
    assert "256 + n_ops (1024 (K L + 5 L + 6 K + 1) + 400) + ceil(n_ops / 2) (1024 K L + 192)" in text


def test_argument_errors_never_abort(mu):
    null = None
    buf, p, odd = aligned_buffer()
    big = 1 << 40

    def compute(ctx=null, mode=0, tr=p, n_keys=4, kidx=null, msgs=p, moff=p, ctxs=null, coff=null, out=p, flag=null, n=4, stream=null):
        return mu.mldsa_mu_compute(ctx, mode, tr, n_keys, kidx, msgs, moff, ctxs, coff, out, flag, n, stream)

    def verify(ctx=null, pset=65, rho=p, t1=p, n_keys=4, kidx=null, m=p, flag=null, sigs=p, ok=p, n=4, scratch=p, sb=big, stream=null):
        return mu.mldsa_verify_mu(ctx, pset, rho, t1, n_keys, kidx, m, flag, sigs, ok, n, scratch, sb, stream)

    def sign(ctx=null, pset=65, rho=p, cap_k=p, s1=p, s2=p, t0=p, n_keys=4, kidx=null, m=p, flag=null, rnd=p, sigs=p, status=null, n=4,
             scratch=p, sb=big, stream=null):
        return mu.mldsa_sign_mu(ctx, pset, rho, cap_k, s1, s2, t0, n_keys, kidx, m, flag, rnd, sigs, status, n, scratch, sb, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (compute, verify, sign):
        assert call() == _lib.ERR_PARAM and b"context" in mu.mldsa_mu_last_error()
    for pset in (0, 45, -65):
        for call in (verify, sign):
            assert call(pset=pset) == _lib.ERR_PARAM and b"parameter set" in mu.mldsa_mu_last_error()
            assert call(pset=pset, n=0) == _lib.ERR_PARAM
    for mode in (-1, 3, 99):
        assert compute(mode=mode) == _lib.ERR_PARAM and b"mode" in mu.mldsa_mu_last_error()
    # a fake non-NULL context must still be refused before it is touched: the checks on pointers and scratch come first
    fake = p
    for kw in (dict(tr=null), dict(moff=null), dict(out=null)):
        assert compute(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in mu.mldsa_mu_last_error(), kw
    for kw in (dict(rho=null), dict(t1=null), dict(m=null), dict(sigs=null), dict(ok=null)):
        assert verify(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in mu.mldsa_mu_last_error(), kw
    for kw in (dict(rho=null), dict(cap_k=null), dict(s1=null), dict(s2=null), dict(t0=null), dict(m=null), dict(rnd=null), dict(sigs=null)):
        assert sign(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL" in mu.mldsa_mu_last_error(), kw
    for call in (compute, verify, sign):
        assert call(ctx=fake, n_keys=0) == _lib.ERR_PARAM and b"n_keys" in mu.mldsa_mu_last_error()
        assert call(ctx=fake, n=(1 << 30) + 1, n_keys=(1 << 30) + 1) == _lib.ERR_PARAM and b"MLDSA_MU_MAX_OPS" in mu.mldsa_mu_last_error()
    for call in (verify, sign):
        for kw in (dict(scratch=null), dict(scratch=odd)):
            assert call(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch" in mu.mldsa_mu_last_error(), kw
    # a scratch below the minimum -- one pass over min(n_ops, 64) ops -- is MLDSA_ERR_NOMEM
    for pset in KL:
        for n in (1, 4, 64, 200):
            need_v, need_s = _verify_formula(pset, min(n, 64)), _sign_formula(pset, min(n, 64))
            for sb in (0, 1, need_v - 1):
                assert verify(ctx=fake, pset=pset, n=n, n_keys=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in mu.mldsa_mu_last_error()
            for sb in (0, 1, need_s - 1):
                assert sign(ctx=fake, pset=pset, n=n, n_keys=n, sb=sb) == _lib.ERR_NOMEM and b"scratch" in mu.mldsa_mu_last_error()
    # empty calls succeed without a context
    assert compute(n=0, tr=null, moff=null, out=null) == _lib.OK
    assert verify(n=0, rho=null, t1=null, m=null, sigs=null, ok=null, scratch=null, sb=0) == _lib.OK
    assert sign(n=0, rho=null, cap_k=null, s1=null, s2=null, t0=null, m=null, rnd=null, sigs=null, scratch=null, sb=0) == _lib.OK


def test_kernels_do_not_spill_and_sources_are_clean(mu):
    kernels = kernel_resources(MU_DIR)
    for stem in ("k_mu_ext", "k_commit", "k_rhopp", "k_accept", "k_count", "k_offsets", "k_compact", "k_gather_rows", "k_gather_pk"):
        assert any(stem in nm for nm in kernels), stem
    assert sum("k_commit" in nm for nm in kernels) == 6 and sum("k_accept" in nm for nm in kernels) == 3  # per set, verify and sign
    sources_clean(MU_DIR, ["../../include/mldsa_mu.h", "../_mu_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"])
    includes_the_core_device_headers(MU_DIR, "mu.hip")


def test_external_mu_is_shake256_of_tr_and_the_formatted_message():
    from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PREHASH, MODE_PURE, PH_SHA512, external_mu, hash_message
    tr = hashlib.shake_256(b"tr").digest(64)
    for msg in (b"", b"a", bytes(range(200)), bytes(1000)):
        for ctx in (b"", b"c", bytes(255)):
            pre = bytes([len(ctx)]) + ctx
            assert external_mu(tr, msg, ctx, MODE_PURE) == hashlib.shake_256(tr + b"\x00" + pre + msg).digest(64)
            assert external_mu(tr, msg, ctx) == external_mu(tr, msg, ctx, MODE_PURE)
            ph = hash_message(msg, PH_SHA512)
            assert external_mu(tr, ph, ctx, MODE_PREHASH) == hashlib.shake_256(tr + b"\x01" + pre + ph).digest(64)
        assert external_mu(tr, msg, mode=MODE_INTERNAL) == hashlib.shake_256(tr + msg).digest(64)
        assert external_mu(tr, msg, b"ignored", MODE_INTERNAL) == hashlib.shake_256(tr + msg).digest(64)
    for mode in (MODE_PURE, MODE_PREHASH):
        with pytest.raises(ValueError):
            external_mu(tr, b"m", bytes(256), mode)
    with pytest.raises(ValueError):
        external_mu(tr[:63], b"m")
    with pytest.raises(ValueError):
        external_mu(tr, b"m", mode=3)
