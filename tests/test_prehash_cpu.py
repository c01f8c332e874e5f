"""The pre-hash library (include/mldsa_ph.h, fips204_amd/ph/libmldsa_ph.so) without a device: its C ABI, how it is linked
against the core, its host-only entry points and its kernels' resources and sources."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

from fips204_amd import _lib, _ph_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PH_DIR = os.path.join(ROOT, "fips204_amd", "ph")


@pytest.fixture(scope="module")
def ph():
    if not os.path.exists(_ph_lib.LIB_PATH) or not glob.glob(os.path.join(PH_DIR, "*.res")):
        from fips204_amd import build
        build.build()
    return _ph_lib.load()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(r"\b(mldsa_ph_[a-z0-9_]+|mldsa_prehash|mldsa_hash_[a-z0-9_]+)\s*\(", text))


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(ph, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "h.c"
    src.write_text('#include "mldsa_ph.h"\nint main(void) { return mldsa_ph_row_len(MLDSA_PH_SHA256) == 43 ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True, capture_output=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _ph_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    exported = {n for n in exported if n.startswith("mldsa_")}
    declared = _declared(_ph_lib.HEADER_PATH)
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert declared == set(_ph_lib._SIGNATURES)
    # the new names are not the core's
    assert not declared & set(_lib.declared_symbols())


def test_layered_on_the_one_core_library(ph):
    dyn = subprocess.run(["readelf", "-d", _ph_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"NEEDED.*\[libmldsa_hip\.so\]", dyn)
    assert re.search(r"(RUNPATH|RPATH).*\$ORIGIN/\.\./csrc", dyn)
    mapped = set()
    for ln in open("/proc/self/maps"):
        if ln.rstrip().endswith("libmldsa_hip.so"):
            mapped.add(os.stat(ln.split()[-1]).st_ino)
    assert len(mapped) == 1, mapped  # two copies would be two HIP module registrations and a foreign mldsa_ctx


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
    res = sorted(glob.glob(os.path.join(PH_DIR, "*.res")))
    assert res, "no .res files under fips204_amd/ph"
    n = 0
    for path in res:
        text = open(path).read()
        names = re.findall(r"Function Name: (\S+)", text)
        spills = re.findall(r"VGPRs Spill: (\d+)", text)
        sgpr_spills = re.findall(r"SGPRs Spill: (\d+)", text)
        scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
        assert len(names) == len(spills) == len(sgpr_spills) == len(scratch)
        for nm, v, sg, sc in zip(names, spills, sgpr_spills, scratch):
            assert int(v) == 0 and int(sg) == 0 and int(sc) == 0, (nm, v, sg, sc)
        n += len(names)
    assert n >= 4  # k_prehash for three PH, k_ph_refuse
    # scalar-memory stores, scalar atomics, scalar-cache write-back / discard (spelled in pieces so that this file holds none of them)
    sp = "s" + "_"
    words = [sp + w for w in ("st" + "ore", "buffer_" + "st" + "ore", "scratch_" + "st" + "ore", "ato" + "mic", "buffer_" + "ato" + "mic",
                              "dca" + "che_wb", "dca" + "che_discard")]
    scalar_mem = re.compile("|".join(re.escape(w) for w in words), re.I)
    for f in sorted(os.listdir(PH_DIR)) + ["../../include/mldsa_ph.h"]:
        path = os.path.normpath(os.path.join(PH_DIR, f))
        if not f.endswith((".hip", ".h", ".cpp")) and os.path.basename(f) != "Makefile":
            continue
        t = open(path, errors="replace").read()
        assert not scalar_mem.search(t), f
        assert "getenv" not in t and "printf" not in t, f
        assert "__HIP_PLATFORM_AMD__" not in t and "__CUDACC__" not in t, f
