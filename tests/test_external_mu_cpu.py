"""The external-mu library (include/mldsa_mu.h, fips204_amd/mu/libmldsa_mu.so) without a device: its C ABI, how it is linked against
the core, its host-only entry points, its kernels' resources and sources, and the host helper external_mu."""
import ctypes as C
import glob
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from fips204_amd import _lib, _mu_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU_DIR = os.path.join(ROOT, "fips204_amd", "mu")
KL = {44: (4, 4), 65: (6, 5), 87: (8, 7)}  # set -> K, L


@pytest.fixture(scope="module")
def mu():
    if not os.path.exists(_mu_lib.LIB_PATH) or not glob.glob(os.path.join(MU_DIR, "*.res")):
        from fips204_amd import build
        build.build()
    return _mu_lib.load()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(r"\b(mldsa_mu_[a-z0-9_]+|mldsa_verify_mu|mldsa_sign_mu)\s*\(", text))


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(mu, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "h.c"
    src.write_text('#include "mldsa_mu.h"\n'
                   "int main(void) { unsigned char m[MLDSA_MU_LEN]; m[0] = 0;\n"
                   "  return mldsa_mu_abi_version() == MLDSA_MU_ABI_VERSION && mldsa_mu_sign_scratch_bytes(MLDSA_65, 1) > m[0] ? 0 : 1; }\n")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _mu_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    exported = {n for n in exported if n.startswith("mldsa_")}
    declared = _declared(_mu_lib.HEADER_PATH)
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert declared == set(_mu_lib._SIGNATURES)
    assert {"mldsa_mu_compute", "mldsa_verify_mu", "mldsa_sign_mu", "mldsa_mu_verify_scratch_bytes", "mldsa_mu_sign_scratch_bytes"} <= declared
    # the new names are not the core's
    assert not declared & set(_lib.declared_symbols())
    text = open(_mu_lib.HEADER_PATH).read()
    assert '#include "mldsa_hip.h"' in text
    assert "#define MLDSA_MU_LEN 64" in text and _mu_lib.MU_LEN == 64
    assert "#define MLDSA_MU_MAX_OPS ((size_t)1 << 30)" in text and _mu_lib.MAX_OPS == 1 << 30
    # the reference crate has no external-mu interface: the entries cite FIPS 204
    assert text.count("FIPS 204") >= 4 and "Algorithm 7" in text and "Algorithm 8" in text


def test_layered_on_the_one_core_library(mu):
    dyn = subprocess.run(["readelf", "-d", _mu_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"NEEDED.*\[libmldsa_hip\.so\]", dyn)
    assert re.search(r"(RUNPATH|RPATH).*\$ORIGIN/\.\./csrc", dyn)
    mapped = set()
    for ln in open("/proc/self/maps"):
        if ln.rstrip().endswith("libmldsa_hip.so"):
            mapped.add(os.stat(ln.split()[-1]).st_ino)
    assert len(mapped) == 1, mapped  # two copies would be two HIP module registrations and a foreign mldsa_ctx
    out = subprocess.run(["nm", "-D", _mu_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    undefined = {ln.split()[-1] for ln in out.splitlines() if " U " in ln}
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    # the arithmetic and the codecs are the core's seams
    for name in ("mldsa_sig_decode", "mldsa_sample_in_ball", "mldsa_expand_a", "mldsa_verify_arith", "mldsa_infinity_norm", "mldsa_expand_mask",
                 "mldsa_ntt", "mldsa_inv_ntt", "mldsa_mat_vec_mul", "mldsa_pointwise_mont", "mldsa_sig_encode", "mldsa_get_params",
                 "mldsa_ctx_device", "mldsa_last_error"):
        assert name in undefined, name
    # ... and the op-level calls, which take messages, are not what it stands on
    for name in ("mldsa_verify", "mldsa_sign", "mldsa_rounding", "mldsa_w1_encode", "mldsa_xof"):
        assert name not in undefined, name
    assert not defined & set(_lib.declared_symbols())
    mk = open(os.path.join(MU_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk  # the recipe is the layers' shared one: read with the Makefile
    mk += open(os.path.join(MU_DIR, "..", "layer", "layer.mk")).read()
    assert "-lmldsa_hip" in mk and "make -C ../csrc" not in mk.replace('build the core first (make -C ../csrc)', "")
    assert "-Rpass-analysis=kernel-resource-usage" in mk
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
    for pset in KL:
        for n in (0, 1, 2, 63, 64, 65, 127, 128, 192, 264, 1000, 65536, 65537, 1 << 30):
            assert mu.mldsa_mu_verify_scratch_bytes(pset, n) == _verify_formula(pset, n), (pset, n)
            assert mu.mldsa_mu_sign_scratch_bytes(pset, n) == _sign_formula(pset, n), (pset, n)
        for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
            assert mu.mldsa_mu_verify_scratch_bytes(pset, n) == 0
            assert mu.mldsa_mu_sign_scratch_bytes(pset, n) == 0
    for bad in (0, 43, 66, -1, 128):
        assert mu.mldsa_mu_verify_scratch_bytes(bad, 10) == 0
        assert mu.mldsa_mu_sign_scratch_bytes(bad, 10) == 0
    # the formulas are the header's
    text = open(_mu_lib.HEADER_PATH).read()
    assert "n_ops (1024 (K L + 3 K + L + 1) + 128)" in text
    assert "256 + n_ops (1024 (K L + 5 L + 6 K + 1) + 400) + ceil(n_ops / 2) (1024 K L + 192)" in text


def test_argument_errors_never_abort(mu):
    null = None
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)  # 256-byte aligned
    odd = C.c_void_p(p.value + 8)
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
    res = sorted(glob.glob(os.path.join(MU_DIR, "*.res")))
    assert res, "no .res files under fips204_amd/mu"
    kernels = []
    for path in res:
        text = open(path).read()
        names = re.findall(r"Function Name: (\S+)", text)
        spills = re.findall(r"VGPRs Spill: (\d+)", text)
        sgpr_spills = re.findall(r"SGPRs Spill: (\d+)", text)
        scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(names) == len(spills) == len(sgpr_spills) == len(scratch)
        for nm, v, sg, sc in zip(names, spills, sgpr_spills, scratch):
            assert int(v) == 0 and int(sg) == 0 and int(sc) == 0, (nm, v, sg, sc)
        kernels += names
    for stem in ("k_mu_ext", "k_commit", "k_rhopp", "k_accept", "k_count", "k_offsets", "k_compact", "k_gather_rows", "k_gather_pk"):
        assert any(stem in nm for nm in kernels), stem
    assert sum("k_commit" in nm for nm in kernels) == 6 and sum("k_accept" in nm for nm in kernels) == 3  # per set, verify and sign
    checked = 0
    for f in sorted(os.listdir(MU_DIR)) + ["../../include/mldsa_mu.h", "../_mu_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]:
        path = os.path.normpath(os.path.join(MU_DIR, f))
        if not f.endswith((".hip", ".h", ".cpp", ".py")) and os.path.basename(f) != "Makefile":
            continue
        t = open(path, errors="replace").read()
        checked += 1
        assert "getenv" not in t and "printf" not in t, f
        # the guard words of tests/test_source_guards_cpu.py
        assert "__HIP_PLATFORM_AMD__" not in t and "__CUDACC__" not in t and "import triton" not in t, f
        assert "secure_getenv" not in t and "environ" not in re.sub(r"//[^\n]*", "", t), f
        # plain C++ only: every store is an ordinary vector store the compiler emits
        assert not re.search(r"\basm\b", t), f
        assert "__builtin_amdgcn_s_sleep" not in t, f
    assert checked >= 6
    # the core's device headers are included, never copied
    src = open(os.path.join(MU_DIR, "mu.hip")).read()
    assert '#include "../layer/layer_dev.h"' in src  # through the layers' shared device header: both links of the chain
    dev = open(os.path.join(MU_DIR, "..", "layer", "layer_dev.h")).read()
    for h in ("../csrc/keccak.h", "../csrc/field.h", "../csrc/rounding.h"):
        assert f'#include "{h}"' in dev


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
