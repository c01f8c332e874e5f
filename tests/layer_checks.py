"""The CPU contract checks that every layered library (ph, keys, mu, seed, keycheck) must pass, once: how it is built, what its header
declares and its library exports, how it is linked against the core, the ladder of its scratch sizes, its kernels' resource files and
the guard words of its sources.  Each test file passes its layer's particulars -- name lists, patterns, formulas, file lists -- and
asserts what only its layer has (its #defines, kernel stems and counts, error words) after the shared check.  No fixtures live here:
import what a file needs by name, as with gpu_common and keycheck_cases."""
import ctypes as C
import glob
import hashlib
import os
import re
import shutil
import subprocess

from fips204_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KL = {44: (4, 4), 65: (6, 5), 87: (8, 7)}  # set -> K, L
PK_SK = {44: (1312, 2560), 65: (1952, 4032), 87: (2592, 4896)}


def core_params():
    """set -> the core's parameters, after checking KL and PK_SK against them"""
    out = {}
    for pset, (pk_len, sk_len) in PK_SK.items():
        p = out[pset] = _lib.get_params(pset)
        assert (p.pk_len, p.sk_len, p.k, p.l) == (pk_len, sk_len) + KL[pset]
        assert pk_len == 32 + 320 * p.k and sk_len % 16 == 0 and pk_len % 16 == 0  # what the layouts and the 16-byte accesses rely on
    return out


def built(loader, layer_dir):
    """the layer's library, built first when it or its kernels' resource files are missing"""
    if not os.path.exists(loader.LIB_PATH) or not glob.glob(os.path.join(layer_dir, "*.res")):
        from fips204_amd import build
        build.build()
    return loader.load()


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def links_the_core_and_never_builds_it(layer_dir):
    mk = open(os.path.join(layer_dir, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk  # the recipe is the layers' shared one: read with the Makefile
    mk += open(os.path.join(layer_dir, "..", "layer", "layer.mk")).read()
    assert "-lmldsa_hip" in mk and "make -C ../csrc" not in mk.replace('build the core first (make -C ../csrc)', "")
    assert "-Rpass-analysis=kernel-resource-usage" in mk


def clean_build(layer, loader, sources, libs, tmp_path):
    """The layer is compiled from scratch in a shadow of the tree (its own Makefile and source copied, the core's directory and
    include/ linked), so a failure half way leaves the checkout's library in place for the tests that follow."""
    from fips204_amd import build
    layer_dir = os.path.dirname(loader.LIB_PATH)
    so = os.path.basename(loader.LIB_PATH)
    before = _sha(build.LIB)
    build.build()  # the whole chain, as a checkout runs it: everything is up to date, so nothing is recompiled
    for lib in libs:
        assert os.path.exists(lib), lib  # the libraries of a checkout
    assert _sha(build.LIB) == before, "build() changed libmldsa_hip.so"
    shadow = tmp_path / "fips204_amd" / layer
    shadow.mkdir(parents=True)
    for f in sources:
        shutil.copy(os.path.join(layer_dir, f), shadow / f)
    os.symlink(build.CSRC, tmp_path / "fips204_amd" / "csrc")
    os.symlink(os.path.join(os.path.dirname(layer_dir), "layer"), tmp_path / "fips204_amd" / "layer")
    os.symlink(os.path.join(ROOT, "include"), tmp_path / "include")
    assert not (shadow / so).exists()
    subprocess.run(["make", "-C", str(shadow)], check=True, capture_output=True)
    assert (shadow / so).exists()
    for f in sources:
        if f.endswith(".hip"):
            assert (shadow / (f[:-4] + ".res")).exists(), f
    assert _sha(build.LIB) == before, f"building the {layer} layer changed libmldsa_hip.so"
    subprocess.run(["make", "-C", str(shadow), "clean"], check=True, capture_output=True)
    assert not (shadow / so).exists() and not list(shadow.glob("*.res")) and not list(shadow.glob("*.o"))
    links_the_core_and_never_builds_it(layer_dir)


def declared(header, pattern):
    """the names matching `pattern` that the header follows with a parenthesis, comments aside"""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(pattern, text))


def exported(lib_path):
    """the names in the text section of the library's dynamic symbol table"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}


def compiles_as_c99(source, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "h.c"
    src.write_text(source)
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True)


def header_and_exports(loader, lib, c_main, pattern, tmp_path):
    """The header is strict C99 and `c_main` compiles against it; what it declares, what the library exports and what the loader
    lists are one set of names, none of them the core's.  Returns (declared names, header text) for the layer's own assertions."""
    compiles_as_c99('#include "%s"\n' % os.path.basename(loader.HEADER_PATH) + c_main, tmp_path)
    names = declared(loader.HEADER_PATH, pattern)
    exports = {n for n in exported(loader.LIB_PATH) if n.startswith("mldsa_")}
    assert names == exports, (sorted(names - exports), sorted(exports - names))
    assert names == set(loader._SIGNATURES)
    for name in names:  # ctypes finds every one of them
        assert getattr(lib, name) is not None
    # the new names are not the core's
    assert not names & set(_lib.declared_symbols())
    text = open(loader.HEADER_PATH).read()
    assert '#include "mldsa_hip.h"' in text
    return names, text


def layered_on_core(lib_path, needs=(), never=()):
    """The library needs the one libmldsa_hip.so beside it, takes every name of `needs` from it, none of `never`, and defines no name
    of the core's itself."""
    dyn = subprocess.run(["readelf", "-d", lib_path], check=True, capture_output=True, text=True).stdout
    assert re.search(r"NEEDED.*\[libmldsa_hip\.so\]", dyn)
    assert re.search(r"(RUNPATH|RPATH).*\$ORIGIN/\.\./csrc", dyn)
    mapped = set()
    for ln in open("/proc/self/maps"):
        if ln.rstrip().endswith("libmldsa_hip.so"):
            mapped.add(os.stat(ln.split()[-1]).st_ino)
    assert len(mapped) == 1, mapped  # two copies would be two HIP module registrations and a foreign mldsa_ctx
    # no core object is linked in: every core entry point the library uses is an undefined symbol, and it defines none of them
    out = subprocess.run(["nm", "-D", lib_path], check=True, capture_output=True, text=True).stdout
    undefined = {ln.split()[-1] for ln in out.splitlines() if " U " in ln}
    defined = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in needs:
        assert name in undefined, name
    for name in never:
        assert name not in undefined, name
    assert not defined & set(_lib.declared_symbols())


def scratch_sweep(fn, formula, max_n):
    """fn(pset, n) is formula(pset, n) up to max_n and never decreases; past max_n, where the size does not fit, and for an unknown
    parameter set it is 0"""
    for pset in KL:
        last = 0
        for n in (0, 1, 2, 63, 64, 65, 127, 128, 192, 264, 1000, 65536, 65537, max_n):
            got = fn(pset, n)
            assert got == formula(pset, n), (pset, n)
            assert got >= last  # non-decreasing in n
            last = got
        for n in (max_n + 1, 2 ** 63, 2 ** 64 - 1):
            assert fn(pset, n) == 0
    for bad in (0, 43, 66, -1, 128):
        assert fn(bad, 10) == 0


def kernel_resources(layer_dir, lds_zero=False):
    """The names of the layer's kernels, after asserting that the compiler warned of nothing and that no kernel spills a register or
    uses scratch memory (with lds_zero: or LDS)."""
    res = sorted(glob.glob(os.path.join(layer_dir, "*.res")))
    assert res, "no .res files under " + os.path.relpath(layer_dir, ROOT)
    kernels = []
    for path in res:
        text = open(path).read()
        assert "warning" not in text, path
        names = re.findall(r"Function Name: (\S+)", text)
        spills = re.findall(r"VGPRs Spill: (\d+)", text)
        sgpr_spills = re.findall(r"SGPRs Spill: (\d+)", text)
        scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        lds = re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)
        assert len(names) == len(spills) == len(sgpr_spills) == len(scratch) == len(lds)
        for nm, v, sg, sc, ld in zip(names, spills, sgpr_spills, scratch, lds):
            assert int(v) == 0 and int(sg) == 0 and int(sc) == 0, (nm, v, sg, sc)
            assert not lds_zero or int(ld) == 0, (nm, ld)
        kernels += names
    return kernels


def sources_clean(layer_dir, extra_files, asm_free=True):
    """The layer's sources and `extra_files` (relative to layer_dir) hold none of the guard words.  Returns [(file, text)] of what was
    read, for a search of the layer's own."""
    read = []
    for f in sorted(os.listdir(layer_dir)) + list(extra_files):
        path = os.path.normpath(os.path.join(layer_dir, f))
        if not f.endswith((".hip", ".h", ".cpp", ".py")) and os.path.basename(f) != "Makefile":
            continue
        t = open(path, errors="replace").read()
        read.append((f, t))
        assert "getenv" not in t and "printf" not in t, f
        # the guard words of tests/test_source_guards_cpu.py
        assert "__HIP_PLATFORM_AMD__" not in t and "__CUDACC__" not in t and "import triton" not in t, f
        assert "secure_getenv" not in t and "environ" not in re.sub(r"//[^\n]*", "", t), f
        if asm_free:  # plain C++ and the HIP builtins only: every store is an ordinary vector store the compiler emits, no wave waits
            assert not re.search(r"\basm\b", t), f
            assert "__builtin_amdgcn_s_sleep" not in t, f
    assert len(read) >= 6
    return read


def shared_plan_is_shared_once(src, scan, wave, host, makefile, scan_h, wave_h, host_h):
    """The record libraries' plan (fips204_amd/rec/rec_scan.h with rec_wave.h, rec_host.h) is used by the library's .hip `src`, not
    restated in it: `src` includes the scan and the host header under the names `scan_h` and `host_h`, the scan includes the wave
    helpers, the library's Makefile names all three, the scan's LDS and every shared definition are in the headers alone, and the
    headers give everything internal linkage."""
    for h in (scan_h, host_h):
        assert f'#include "{h}"' in src and h in makefile, h  # a change of a shared header rebuilds the library
    assert '#include "rec_wave.h"' in scan and wave_h in makefile and '#include "rec_scan.h"' not in wave
    # LDS: the per-wave partial sums of the two scan kernels only
    assert scan.count("__shared__") == 2 and "__shared__" not in src + host + wave and "extern __shared__" not in scan
    for name in ("op_values", "wave_inclusive", "copy_field", "k_classify", "k_offsets", "k_apply", "plan_layout", "front_layout",
                 "check_plan_memory", "launch_plan", "totals_consistent", "read_totals"):
        defined = r"^[^\n;=/]*\b(void|bool|int|uint64_t|size_t)\s+%s\s*\(" % name
        assert not re.search(defined, src, flags=re.M), name
        assert len(re.findall(defined, scan + wave + host, flags=re.M)) == 1, name
    for name in ("wave_inclusive", "copy_field"):  # the two that the certificate layers take too: in the header without kernels
        assert re.search(r"\b(void|uint64_t)\s+%s\s*\(" % name, wave), name
    for word in ("SCAN_WAVES =", "SLOT_MASK =", "struct PlanLayout", "struct FrontLayout"):
        assert word not in src and (scan + wave + host).count(word) == 1, word
    for text in (scan, wave, host):  # layer_host.h's style: two libraries in one process share no kernel stub and no function
        assert re.search(r"\nnamespace mldsa_rec \{\nnamespace \{\n", text) and text.rstrip().endswith("}  // namespace\n}  // namespace mldsa_rec")
        assert not re.search(r"\bextern\b", text)
    assert "__global__" not in host + wave and "hipLaunchKernelGGL" not in scan + wave  # device code in two headers, host code in the third


# ---- what the certificate layers share (x509, x509sign, csr, crl, path, find) -------------------------------------------------------
CERT_LAYERS = ("x509", "x509sign", "csr", "crl", "path", "find")
# helper -> the one file that defines it (relative to fips204_amd/); the pattern of its definition is SHARED_DEFINED % name
CERT_SHARED = {
    "BlobBytes": "x509/x509_dev.h", "wave_names_differ": "x509/x509_dev.h", "write_link_op": "x509/x509_dev.h",
    "place_block_sums": "rec/rec_place.h", "place_block_offsets": "rec/rec_place.h", "place_wave_scan": "rec/rec_place.h",
    "place_before": "rec/rec_place.h", "place_totals": "rec/rec_place.h", "place_fits": "rec/rec_place.h",
    "wave_sum": "layer/layer_dev.h",
    "same_alg": "x509/x509_plan.h", "ranges_apart": "layer/layer_host.h",
    "scan_blocks": "rec/rec_plan.h", "place_sums_bytes": "rec/rec_plan.h", "place_plan_bytes": "rec/rec_plan.h",
}
SHARED_DEFINED = r"^[^\n;=/(]*\b(?:struct\s+%s\s*\{|(?:void|bool|int|uint32_t|uint64_t|size_t)\s+%s\s*\()"
# Pieces that did not pass the rule of layer_dev.h ("the same instructions as written out") and so are defined nowhere: they stay
# written out in the kernels and walks that use them, and the headers and DESIGN.md say why.
#   signed_envelope, alg_sig  as functions of x509_plan.h they change the registers of k_x509_parse, k_crl_parse and k_csr_parse
#   name_ranges               lane 0's decision on the two Name ranges in k_x509_link and k_crl_link, and the broadcast behind it
#   (k_crl_place keeps its scan written out too: with the placement helpers it takes two more VGPRs)
CERT_NOT_SHARED = ("signed_envelope", "alg_sig", "name_ranges")
CERT_NEW_HEADERS = {"x509/x509_dev.h": "mldsa_x509", "rec/rec_place.h": "mldsa_rec", "rec/rec_wave.h": "mldsa_rec"}


def certificate_helpers_shared_once(layer):
    """What the certificate layers share is defined exactly once in the tree and in none of their .hip files; the .hip of `layer` that
    uses a helper includes its header (directly, or for the plan headers through its own plan header) and its Makefile names it; the
    new headers keep everything in an unnamed namespace inside their named one and hold no kernel and no `extern`."""
    base = os.path.join(ROOT, "fips204_amd")
    tree = {}
    for path in glob.glob(os.path.join(base, "**", "*"), recursive=True):
        if path.endswith((".h", ".hip", ".cpp", ".hpp")):
            tree[os.path.relpath(path, base)] = open(path, errors="replace").read()
    hips = ["%s/%s.hip" % (l, l) for l in CERT_LAYERS]
    for name, home in CERT_SHARED.items():
        pat = SHARED_DEFINED % (name, name)
        where = sorted(f for f, text in tree.items() if re.search(pat, text, flags=re.M))
        assert where == [home], (name, where)
        assert len(re.findall(pat, tree[home], flags=re.M)) == 1, name
    for name in ("wave_inclusive", "copy_field"):  # rec_wave.h's (shared_plan_is_shared_once counts them among the record headers)
        assert not any(re.search(SHARED_DEFINED % (name, name), tree[f], flags=re.M) for f in hips), name
    for name in CERT_NOT_SHARED:
        assert not any(re.search(SHARED_DEFINED % (name, name), text, flags=re.M) for text in tree.values()), name
    assert set(hips) <= set(tree)
    src, mk = tree["%s/%s.hip" % (layer, layer)], open(os.path.join(base, layer, "Makefile")).read()
    code = re.sub(r"//[^\n]*", "", src)
    plan = tree["%s/%s_plan.h" % (layer, layer)]
    used = 0
    for name, home in CERT_SHARED.items():
        if not re.search(r"\b%s\b" % name, code + re.sub(r"//[^\n]*", "", plan)):
            continue
        used += 1
        rel = os.path.basename(home) if home.startswith(layer + "/") else "../" + home
        assert rel in mk, (layer, name, rel)  # a change of the shared header rebuilds the library
        reached = [src, plan] + [tree[h] for h in CERT_NEW_HEADERS] + [tree["x509/x509_plan.h"], tree["x509sign/x509sign_plan.h"]]
        assert any('#include "%s"' % inc in text for text in reached for inc in (rel, os.path.basename(home), "../" + home)), (layer, name)
    assert used >= 1, layer  # BlobBytes at the least
    assert '#include "%s"' % ("x509_dev.h" if layer == "x509" else "../x509/x509_dev.h") in src
    assert "rec_scan.h" not in src + mk  # the class scan's kernels are the record libraries' alone
    for h, ns in CERT_NEW_HEADERS.items():
        text = tree[h]
        assert re.search(r"\nnamespace %s \{\nnamespace \{\n" % ns, text) and text.rstrip().endswith("}  // namespace\n}  // namespace " + ns), h
        body = re.sub(r"//[^\n]*", "", text)  # (the comments say what stays in the kernels)
        assert "__global__" not in body and "__shared__" not in body and not re.search(r"\bextern\b", body), h
        assert "hipLaunchKernelGGL" not in body and "#pragma once" in body, h


# what libmldsa_rec.so and libmldsa_recsign.so exported beside their entry points before the plan was shared: libstdc++'s inline functions
STD_WEAK = {"_ZNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEC2IS3_EEPKcRKS3_", "_ZNSt7__cxx119to_stringEm",
            "_ZStplIcSt11char_traitsIcESaIcEENSt7__cxx1112basic_stringIT_T0_T1_EEOS8_PKS5_",
            "_ZStplIcSt11char_traitsIcESaIcEENSt7__cxx1112basic_stringIT_T0_T1_EEOS8_S9_"}


def no_new_dynamic_symbol(lib_path, prefix):
    """The shared plan adds nothing to the library's dynamic symbol table: a kernel template with external linkage would put a weak host
    stub of one name into both record libraries, and the loader would bind both to the first."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    for ln in out.splitlines():
        kind, name = ln.split()[-2:]
        if kind in "WwVv":
            for word in ("k_classify", "k_offsets", "k_apply", "k_pack", "k_scatter", "copy_field", "mldsa_rec", "_GLOBAL__N"):
                assert word not in name, ln
        assert (kind == "T" and name.startswith(prefix)) or name in STD_WEAK or re.fullmatch(r"__hip_cuid_[0-9a-f]+", name), ln


def includes_the_core_device_headers(layer_dir, source):
    """the core's device headers are included, never copied: through the layers' shared device header, both links of the chain"""
    src = open(os.path.join(layer_dir, source)).read()
    assert '#include "../layer/layer_dev.h"' in src
    dev = open(os.path.join(layer_dir, "..", "layer", "layer_dev.h")).read()
    for h in ("../csrc/keccak.h", "../csrc/field.h", "../csrc/rounding.h"):
        assert f'#include "{h}"' in dev
    return src


def sanitized_program(tmp_path, name, sources, ok_line, hip_host=False, env=None):
    """tests/cpp/<sources> compiled into the stand-alone program `name` under ASan + UBSan (with hip_host: host-only by hipcc, as
    tests/test_sanitizers_cpu.py compiles the core's host code) and run as a child: it ends with status 0 and prints `ok_line`.  `env`
    is added to the child's environment; nothing else is set there."""
    exe = str(tmp_path / name)
    src = [os.path.join(ROOT, "tests", "cpp", f) for f in sources]
    if hip_host:
        cmd = ["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unused-function", "-x", "hip"] + src + ["-o", exe]
    else:
        cxx = "g++" if subprocess.run(["which", "g++"], capture_output=True).returncode == 0 else "/opt/rocm/lib/llvm/bin/clang++"
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-o", exe] + src
    subprocess.check_call(cmd)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=None if env is None else dict(os.environ, **env))
    assert run.returncode == 0 and ok_line in run.stdout, (run.stdout[-500:], run.stderr[-4000:])


def aligned_buffer():
    """(the buffer to keep alive, a 256-byte aligned pointer into it with 3840 bytes behind it, that pointer + 8)"""
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)
    return buf, p, C.c_void_p(p.value + 8)
