"""The seed-form key library (include/mldsa_seed.h, fips204_amd/seed/libmldsa_seed.so) without a device: that a clean build produces it
and leaves the core untouched, its C ABI, how it is linked against the core, its scratch formulas, its host-only argument checks, its
kernels' resources and sources, and the host helper private_key_forms."""
import ctypes as C
import glob
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from fips204_amd import _lib, _seed_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_DIR = os.path.join(ROOT, "fips204_amd", "seed")
KL = {44: (4, 4), 65: (6, 5), 87: (8, 7)}  # set -> K, L
PK_SK = {44: (1312, 2560), 65: (1952, 4032), 87: (2592, 4896)}


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def seed():
    if not os.path.exists(_seed_lib.LIB_PATH) or not glob.glob(os.path.join(SEED_DIR, "*.res")):
        from fips204_amd import build
        build.build()
    return _seed_lib.load()


def test_a_clean_build_of_the_layer_produces_the_library_and_leaves_the_core_alone(seed, tmp_path):
    """The layer is compiled from scratch in a shadow of the tree (its own Makefile and source copied, the core's directory and
    include/ linked), so a failure half way leaves the checkout's libmldsa_seed.so in place for the tests that follow."""
    from fips204_amd import build
    assert build.SEED_LIB == _seed_lib.LIB_PATH
    before = _sha(build.LIB)
    build.build()  # the whole chain, as a checkout runs it: everything is up to date, so nothing is recompiled
    for lib in (build.LIB, build.PH_LIB, build.KEYS_LIB, build.MU_LIB, build.SEED_LIB):
        assert os.path.exists(lib), lib  # the five libraries of a checkout
    assert _sha(build.LIB) == before, "build() changed libmldsa_hip.so"
    shadow = tmp_path / "fips204_amd" / "seed"
    shadow.mkdir(parents=True)
    for f in ("Makefile", "seed.hip"):
        shutil.copy(os.path.join(SEED_DIR, f), shadow / f)
    os.symlink(build.CSRC, tmp_path / "fips204_amd" / "csrc")
    os.symlink(os.path.join(os.path.dirname(SEED_DIR), "layer"), tmp_path / "fips204_amd" / "layer")
    os.symlink(os.path.join(ROOT, "include"), tmp_path / "include")
    assert not (shadow / "libmldsa_seed.so").exists()
    subprocess.run(["make", "-C", str(shadow)], check=True, capture_output=True)
    assert (shadow / "libmldsa_seed.so").exists() and (shadow / "seed.res").exists()
    assert _sha(build.LIB) == before, "building the seed layer changed libmldsa_hip.so"
    subprocess.run(["make", "-C", str(shadow), "clean"], check=True, capture_output=True)
    assert not (shadow / "libmldsa_seed.so").exists() and not list(shadow.glob("*.res")) and not list(shadow.glob("*.o"))
    mk = open(os.path.join(SEED_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk  # the recipe is the layers' shared one: read with the Makefile
    mk += open(os.path.join(SEED_DIR, "..", "layer", "layer.mk")).read()
    assert "-lmldsa_hip" in mk and "make -C ../csrc" not in mk.replace('build the core first (make -C ../csrc)', "")
    assert "-Rpass-analysis=kernel-resource-usage" in mk


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(r"\b(mldsa_seed_[a-z0-9_]+|mldsa_sign_seed)\s*\(", text))


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(seed, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "h.c"
    src.write_text('#include "mldsa_seed.h"\n'
                   "int main(void) { unsigned char x[MLDSA_SEED_LEN]; x[0] = 0;\n"
                   "  return mldsa_seed_abi_version() == MLDSA_SEED_ABI_VERSION && mldsa_seed_sign_scratch_bytes(MLDSA_65, 1) > x[0] ? 0 : 1; }\n")
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _seed_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    exported = {n for n in exported if n.startswith("mldsa_")}
    declared = _declared(_seed_lib.HEADER_PATH)
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert declared == set(_seed_lib._SIGNATURES)
    assert {"mldsa_seed_expand", "mldsa_seed_check", "mldsa_sign_seed", "mldsa_seed_expand_scratch_bytes", "mldsa_seed_check_scratch_bytes",
            "mldsa_seed_sign_scratch_bytes", "mldsa_seed_abi_version", "mldsa_seed_last_error"} == declared
    for name in declared:  # ctypes finds every one of them
        assert getattr(seed, name) is not None
    # the new names are not the core's
    assert not declared & set(_lib.declared_symbols())
    text = open(_seed_lib.HEADER_PATH).read()
    assert '#include "mldsa_hip.h"' in text
    assert "#define MLDSA_SEED_ABI_VERSION 1" in text and seed.mldsa_seed_abi_version() == _seed_lib.ABI_VERSION == 1
    assert "#define MLDSA_SEED_LEN 32" in text and _seed_lib.SEED_LEN == 32
    assert "#define MLDSA_SEED_MAX_KEYS ((size_t)1 << 24)" in text and _seed_lib.MAX_KEYS == 1 << 24
    # the reference crate signs from no seed: the entries cite FIPS 204; the range of the int32 outputs is stated
    assert text.count("FIPS 204") >= 3 and "Algorithm 6" in text and "lies in (-q, q)" in text


def test_layered_on_the_one_core_library(seed):
    dyn = subprocess.run(["readelf", "-d", _seed_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"NEEDED.*\[libmldsa_hip\.so\]", dyn)
    assert re.search(r"(RUNPATH|RPATH).*\$ORIGIN/\.\./csrc", dyn)
    mapped = set()
    for ln in open("/proc/self/maps"):
        if ln.rstrip().endswith("libmldsa_hip.so"):
            mapped.add(os.stat(ln.split()[-1]).st_ino)
    assert len(mapped) == 1, mapped  # two copies would be two HIP module registrations and a foreign mldsa_ctx
    out = subprocess.run(["nm", "-D", _seed_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    undefined = {ln.split()[-1] for ln in out.splitlines() if " U " in ln}
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    # the sampling and the arithmetic are the core's seams, the check and the signer stand on its whole operations
    for name in ("mldsa_expand_a", "mldsa_expand_s", "mldsa_ntt", "mldsa_mat_vec_mul", "mldsa_inv_ntt", "mldsa_to_mont", "mldsa_keygen",
                 "mldsa_sign", "mldsa_memset", "mldsa_get_params", "mldsa_ctx_device", "mldsa_last_error"):
        assert name in undefined, name
    # ... and the wire private key is never decoded or encoded here
    for name in ("mldsa_sk_expand", "mldsa_sk_into_bytes", "mldsa_bit_pack", "mldsa_bit_unpack"):
        assert name not in undefined, name
    assert not defined & set(_lib.declared_symbols())


def _expand_formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (k * l + l + 2 * k) + 320 * k + 96)


def _check_formula(pset, n):
    return n * sum(PK_SK[pset])


def _sign_formula(pset, n):
    k, l = KL[pset]
    return n * (1024 * (l + 2 * k) + 128) + _expand_formula(pset, n)


def test_scratch_sizes_follow_the_documented_formulas(seed):
    fns = ((seed.mldsa_seed_expand_scratch_bytes, _expand_formula), (seed.mldsa_seed_check_scratch_bytes, _check_formula),
           (seed.mldsa_seed_sign_scratch_bytes, _sign_formula))
    for pset in KL:
        for fn, formula in fns:
            last = 0
            for n in (0, 1, 2, 63, 64, 65, 127, 128, 1000, 65536, 65537, 1 << 24):
                got = fn(pset, n)
                assert got == formula(pset, n), (pset, n)
                assert got >= last  # non-decreasing in n
                last = got
            for n in ((1 << 24) + 1, 2 ** 63, 2 ** 64 - 1):
                assert fn(pset, n) == 0
    for bad in (0, 43, 66, -1, 128):
        for fn, _ in fns:
            assert fn(bad, 10) == 0
    # the formulas are the header's
    text = open(_seed_lib.HEADER_PATH).read()
    assert "n_keys (1024 (K L + L + 2 K) + 320 K + 96)" in text
    assert "n_keys (PK_LEN + SK_LEN) = n_keys * 3872 / 5984 / 7488" in text
    assert "n_keys (1024 (L + 2 K) + 128) + expand(n_keys)" in text
    assert [sum(PK_SK[s]) for s in (44, 65, 87)] == [3872, 5984, 7488]
    for pset, (pk_len, sk_len) in PK_SK.items():
        p = _lib.get_params(pset)
        assert (p.pk_len, p.sk_len, p.k, p.l) == (pk_len, sk_len) + KL[pset]
        assert pk_len == 32 + 320 * p.k and sk_len % 16 == 0 and pk_len % 16 == 0  # what the layouts and the 16-byte compare rely on


def test_argument_errors_never_abort(seed):
    null = None
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)  # 256-byte aligned
    odd = C.c_void_p(p.value + 8)
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
    res = sorted(glob.glob(os.path.join(SEED_DIR, "*.res")))
    assert res, "no .res files under fips204_amd/seed"
    kernels = []
    for path in res:
        text = open(path).read()
        assert "warning" not in text, path
        names = re.findall(r"Function Name: (\S+)", text)
        spills = re.findall(r"VGPRs Spill: (\d+)", text)
        sgpr_spills = re.findall(r"SGPRs Spill: (\d+)", text)
        scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(names) == len(spills) == len(sgpr_spills) == len(scratch)
        for nm, v, sg, sc in zip(names, spills, sgpr_spills, scratch):
            assert int(v) == 0 and int(sg) == 0 and int(sc) == 0, (nm, v, sg, sc)
        kernels += names
    for stem in ("k_seed_h", "k_seed_rows", "k_seed_t", "k_seed_tr", "k_seed_cmp"):
        assert any(stem in nm for nm in kernels), stem
    assert sum("k_seed_tr" in nm for nm in kernels) == 3  # one per parameter set
    checked = 0
    for f in sorted(os.listdir(SEED_DIR)) + ["../../include/mldsa_seed.h", "../_seed_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]:
        path = os.path.normpath(os.path.join(SEED_DIR, f))
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
    src = open(os.path.join(SEED_DIR, "seed.hip")).read()
    assert '#include "../layer/layer_dev.h"' in src  # through the layers' shared device header: both links of the chain
    dev = open(os.path.join(SEED_DIR, "..", "layer", "layer_dev.h")).read()
    for h in ("../csrc/keccak.h", "../csrc/field.h", "../csrc/rounding.h"):
        assert f'#include "{h}"' in dev
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
