"""What the layered libraries share (fips204_amd/layer/: layer_host.h, layer_dev.h, layer.mk, host_feed.h, host_chunks.h) -- CPU only.

The five libraries (ph, keys, mu, seed, keycheck) are loaded into one process.  The shared host scaffold must therefore stay private to
each of them: an error slot per library, and no symbol of the scaffold in any dynamic symbol table.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from fips204_amd import _keycheck_lib, _keys_lib, _lib, _mu_lib, _ph_lib, _seed_lib
from layer_checks import ROOT, sanitized_program

PKG = os.path.join(ROOT, "fips204_amd")
LAYER_DIR = os.path.join(PKG, "layer")
SHARED = [os.path.join(LAYER_DIR, f) for f in ("layer_host.h", "layer_dev.h", "layer.mk", "host_feed.h", "host_chunks.h")]
LOADERS = {"ph": _ph_lib, "keys": _keys_lib, "mu": _mu_lib, "seed": _seed_lib, "keycheck": _keycheck_lib}

_STRING_CTOR = "_ZNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEC2IS3_EEPKcRKS3_"
_STRING_PLUS = "_ZStplIcSt11char_traitsIcESaIcEENSt7__cxx1112basic_stringIT_T0_T1_EEOS8_PKS5_"
# `nm -D --defined-only` of the libraries as they were before the scaffold was shared: (type, name), every type.  The compilation-unit
# ids (__hip_cuid_<hash of the build's paths>, one per object) are written without their hash.
SYMBOLS_BEFORE = {
    "ph": [("B", "__hip_cuid_*")] * 3 + [("W", _STRING_CTOR), ("W", _STRING_PLUS), ("W", "_ZN8mldsa_ph11DeviceScopeD2Ev")] + [("T", s) for s in (
        "_ZN8mldsa_ph10row_len_ofEi", "_ZN8mldsa_ph11core_failedEPKci", "_ZN8mldsa_ph11launch_initEiPjmP12ihipStream_t",
        "_ZN8mldsa_ph12launch_finalEiPKjPhPmS2_mP12ihipStream_t", "_ZN8mldsa_ph13launch_updateEiPjPKhPKmmmmmmmP12ihipStream_t",
        "_ZN8mldsa_ph14state_bytes_ofEim", "_ZN8mldsa_ph4failEiRKNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE",
        "mldsa_hash_sign", "mldsa_hash_sign_host", "mldsa_hash_verify", "mldsa_hash_verify_host", "mldsa_hash_verify_pk",
        "mldsa_ph_abi_version", "mldsa_ph_final", "mldsa_ph_host_create", "mldsa_ph_host_destroy", "mldsa_ph_init", "mldsa_ph_last_error",
        "mldsa_ph_row_len", "mldsa_ph_scratch_bytes", "mldsa_ph_state_bytes", "mldsa_ph_update", "mldsa_prehash")],
    "keys": [("B", "__hip_cuid_*"), ("W", _STRING_CTOR), ("W", _STRING_PLUS)] + [("T", s) for s in (
        "mldsa_keys_abi_version", "mldsa_keys_dedup", "mldsa_keys_dedup_scratch_bytes", "mldsa_keys_last_error",
        "mldsa_keys_verify_scratch_bytes", "mldsa_verify_pk_dedup")],
    "mu": [("B", "__hip_cuid_*"), ("W", _STRING_CTOR), ("W", _STRING_PLUS)] + [("T", s) for s in (
        "mldsa_mu_abi_version", "mldsa_mu_compute", "mldsa_mu_last_error", "mldsa_mu_sign_scratch_bytes", "mldsa_mu_verify_scratch_bytes",
        "mldsa_sign_mu", "mldsa_verify_mu")],
    "seed": [("B", "__hip_cuid_*"), ("W", _STRING_CTOR), ("W", _STRING_PLUS)] + [("T", s) for s in (
        "mldsa_seed_abi_version", "mldsa_seed_check", "mldsa_seed_check_scratch_bytes", "mldsa_seed_expand",
        "mldsa_seed_expand_scratch_bytes", "mldsa_seed_last_error", "mldsa_seed_sign_scratch_bytes", "mldsa_sign_seed")],
    "keycheck": [("B", "__hip_cuid_*"), ("W", _STRING_CTOR), ("W", _STRING_PLUS)] + [("T", s) for s in (
        "mldsa_keycheck_abi_version", "mldsa_keycheck_last_error", "mldsa_keycheck_scratch_bytes", "mldsa_keypair_check", "mldsa_sk_import",
        "mldsa_sk_range_check")],
}
# The one symbol that leaves: libmldsa_ph.so used to export the destructor of its own DeviceScope (an inline member of a class with
# external linkage).  It now uses the scaffold's, which has internal linkage like everything else there.
SYMBOLS_GONE = {"ph": [("W", "_ZN8mldsa_ph11DeviceScopeD2Ev")]}
SCAFFOLD_WORDS = ("g_err", "DeviceScope", "largest_pass", "mldsa_layer")


@pytest.fixture(scope="module")
def libs():
    if not all(os.path.exists(m.LIB_PATH) for m in LOADERS.values()):
        from fips204_amd import build
        build.build()
    return {name: m.load() for name, m in LOADERS.items()}


def _failures(libs):
    """name -> (a call that fails before it touches a context or a device, the library's last_error, a word of the message)."""
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)  # 256-byte aligned; also the fake non-NULL context
    null, big = None, 1 << 50
    ph, keys, mu, seed, kc = (libs[n] for n in ("ph", "keys", "mu", "seed", "keycheck"))
    return {
        "seed": (lambda: seed.mldsa_seed_expand(null, 65, p, p, p, p, p, p, p, null, 4, p, big, null), seed.mldsa_seed_last_error,
                 b"mldsa_seed_expand: NULL context"),
        "keycheck": (lambda: kc.mldsa_keypair_check(p, 7, p, null, p, 4, p, big, null), kc.mldsa_keycheck_last_error,
                     b"mldsa_keypair_check: unknown parameter set"),
        "mu": (lambda: mu.mldsa_verify_mu(p, 65, null, p, 4, null, p, null, p, p, 4, p, big, null), mu.mldsa_mu_last_error,
               b"mldsa_verify_mu: NULL pointer"),
        "keys": (lambda: keys.mldsa_keys_dedup(p, 65, p, 4, bytes(16), 65, p, p, 4, p, p, big, null), keys.mldsa_keys_last_error,
                 b"mldsa_keys_dedup: hash_bits outside 1 ... 64"),
        "ph": (lambda: ph.mldsa_prehash(p, 99, p, p, p, null, 4, null), ph.mldsa_ph_last_error, b"mldsa_prehash: unknown ph"),
    }


def test_error_slots_stay_separate(libs):
    """One thread, five libraries: a failure in one library leaves the message of every other library where it was."""
    fails = _failures(libs)
    for first in fails:
        call, last_error, message = fails[first]
        assert call() == _lib.ERR_PARAM and last_error() == message
        for other in fails:
            if other == first:
                continue
            o_call, o_last_error, o_message = fails[other]
            assert o_message != message
            assert o_call() == _lib.ERR_PARAM and o_last_error() == o_message
            assert last_error() == message, f"a failure in {other} overwrote the message of {first}"
    # and all five at once, each still its own
    for call, _, _ in fails.values():
        assert call() == _lib.ERR_PARAM
    assert [last_error() for _, last_error, _ in fails.values()] == [message for _, _, message in fails.values()]


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = []
    for line in out.splitlines():
        parts = line.split()
        syms.append((parts[-2], re.sub(r"^__hip_cuid_[0-9a-f]+$", "__hip_cuid_*", parts[-1])))
    return sorted(syms)


@pytest.mark.parametrize("name", sorted(LOADERS))
def test_nothing_of_the_scaffold_is_exported(libs, name):
    defined = _defined(LOADERS[name].LIB_PATH)
    gone = SYMBOLS_GONE.get(name, [])
    assert all(s in SYMBOLS_BEFORE[name] for s in gone)
    assert defined == sorted(s for s in SYMBOLS_BEFORE[name] if s not in gone)
    for _, sym in defined:
        for word in SCAFFOLD_WORDS:
            assert word not in sym, (sym, word)
    # the scaffold is in the library all the same: local symbols of an unnamed namespace (checked where the library is not stripped)
    local = subprocess.run(["nm", LOADERS[name].LIB_PATH], check=True, capture_output=True, text=True).stdout
    for line in local.splitlines():
        parts = line.split()
        if any(word in parts[-1] for word in SCAFFOLD_WORDS):
            assert parts[-2].islower(), line  # lower case: a local symbol


def test_the_shared_files_pass_the_guard_words():
    """The guard words of tests/test_source_guards_cpu.py and of the layers' own source checks."""
    for path in SHARED + [os.path.join(PKG, "_layer.py")]:
        t = open(path).read()
        assert "getenv" not in t and "printf" not in t, path
        assert not re.search(r"\basm\b", t), path
        assert "__CUDACC__" not in t and "__HIP_PLATFORM_AMD__" not in t and "import triton" not in t, path
        assert "environ" not in re.sub(r"//[^\n]*", "", t), path
    host = open(SHARED[0]).read()
    # internal linkage for the whole host scaffold: one unnamed namespace from the first definition to the end of the header
    body = host[host.index("namespace mldsa_layer {"):]
    assert re.match(r"namespace mldsa_layer \{\nnamespace \{\n", body)
    assert body.rstrip().endswith("}  // namespace\n}  // namespace mldsa_layer")
    assert body.count("namespace") == 4 and "extern" not in body
    dev = open(SHARED[1]).read()
    code = re.sub(r"//[^\n]*", "", dev + host)
    assert "__global__" not in code  # helpers only: every kernel stays in its library's .hip file
    for m in re.finditer(r"^[^/\n]*\b__device__\b[^\n]*$", dev, flags=re.M):
        assert "__device__ __forceinline__" in m.group(0), m.group(0)


def test_one_scaffold_only():
    defs, slots = [], []
    for root, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith((".hip", ".h", ".hpp", ".cpp")):
                continue
            path = os.path.join(root, f)
            t = open(path, errors="replace").read()
            defs += [os.path.relpath(path, PKG)] * len(re.findall(r"\bstruct DeviceScope\b", t))
            slots += [os.path.relpath(path, PKG)] * t.count("thread_local std::string g_err")
    assert defs == [os.path.join("layer", "layer_host.h")]
    assert sorted(slots) == [os.path.join("layer", "layer_host.h"), os.path.join("ph", "prehash.hip")]
    # the four libraries that take the whole scaffold define none of it themselves
    for rel in ("mu/mu.hip", "seed/seed.hip", "keycheck/keycheck.hip", "keys/dedup.hip"):
        t = open(os.path.join(PKG, rel)).read()
        assert '#include "../layer/layer_host.h"' in t, rel
        for word in ("int fail(", "int core_failed(", "int hip_failed(", "bool aligned(", "struct Taker", "auto take = ", "_CORE(call, name)",
                     "_LAUNCHED(what)", "hipSetDevice"):
            assert word not in t, (rel, word)
    # one host-memory feed: the ring of staging chunks is written in layer/host_feed.h and nowhere else among the layers (csrc/ aside)
    feed_words = {"bool is_pinned(": [], "in_flight": [], "DEFAULT_STAGING": []}
    for root, _, files in os.walk(PKG):
        if os.path.relpath(root, PKG).split(os.sep)[0] == "csrc":
            continue
        for f in files:
            if f.endswith((".hip", ".h", ".hpp", ".cpp")):
                text = open(os.path.join(root, f), errors="replace").read()
                for word, where in feed_words.items():
                    if word in text:
                        where.append(os.path.relpath(os.path.join(root, f), PKG))
    for word, where in feed_words.items():
        assert where == [os.path.join("layer", "host_feed.h")], (word, where)
    for rel in ("ph/hostfed.hip", "mus/mus.hip"):
        assert '#include "../layer/host_feed.h"' in open(os.path.join(PKG, rel)).read(), rel
    # five Makefiles, one recipe
    for layer in LOADERS:
        mk = open(os.path.join(PKG, layer, "Makefile")).read()
        assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk, layer


def test_the_host_feed_under_asan_and_ubsan(tmp_path):
    """layer/host_feed.h, compiled host-only as tests/test_sanitizers_cpu.py compiles the core's host code and linked over the stand-in
    HIP runtime, driven by tests/cpp/host_feed_main.cpp: a stand-alone program, so the sanitizers' runtimes are linked in"""
    sanitized_program(tmp_path, "host_feed", ["host_feed_main.cpp", "stub_hip_full.cpp"], "host_feed OK", hip_host=True,
                      env={"ASAN_OPTIONS": "detect_leaks=1"})
