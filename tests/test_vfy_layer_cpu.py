"""The large-batch verify library (include/mldsa_vfy.h, fips204_amd/vfy/libmldsa_vfy.so) without a device: its C ABI, how it is linked
against the core, its scratch sizes, its argument checks, its kernels' resources and sources, the routing constants of the Python
binding, and the part plan and scratch carve as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from fips204_amd import _lib, _mus_lib, _vfy_lib
from layer_checks import (KL, ROOT, aligned_buffer, built, clean_build, core_params, header_and_exports, includes_the_core_device_headers,
                          kernel_resources, layered_on_core, links_the_core_and_never_builds_it, sanitized_program, scratch_sweep, sources_clean)

VFY_DIR = os.path.join(ROOT, "fips204_amd", "vfy")
SOURCES = ["Makefile", "vfy.hip", "keccak180.h", "vfy_parts.h"]


@pytest.fixture(scope="module")
def vfy():
    return built(_vfy_lib, VFY_DIR)


def test_clean_build_in_a_shadow_tree(vfy, tmp_path):
    from fips204_amd import build
    assert build.LAYERS["vfy"] == "libmldsa_vfy.so" and build.VFY_LIB == _vfy_lib.LIB_PATH
    assert list(build.LAYERS)[-1] == "vfy"  # one entry, behind the layers that were there
    clean_build("vfy", _vfy_lib, SOURCES, [os.path.join(build._HERE, d, f) for d, f in build.LAYERS.items()], tmp_path)
    mk = open(os.path.join(VFY_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(vfy, tmp_path):
    declared, text = header_and_exports(
        _vfy_lib, vfy,
        "int main(void) { return mldsa_vfy_abi_version() == MLDSA_VFY_ABI_VERSION && mldsa_vfy_scratch_bytes(MLDSA_65, MLDSA_VFY_MAX_OPS) >\n"
        "  MLDSA_VFY_PART_OPS ? 0 : 1; }\n",
        r"\b(mldsa_vfy_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_vfy_abi_version", "mldsa_vfy_last_error", "mldsa_vfy_scratch_bytes", "mldsa_vfy_verify", "mldsa_vfy_expand_a",
                        "mldsa_vfy_set_part_ops", "mldsa_vfy_profile_enable", "mldsa_vfy_profile_report"}
    assert "#define MLDSA_VFY_ABI_VERSION 1" in text and vfy.mldsa_vfy_abi_version() == _vfy_lib.ABI_VERSION == 1
    assert "#define MLDSA_VFY_MAX_OPS ((size_t)1 << 22)" in text and _vfy_lib.MAX_OPS == 1 << 22
    # the part size: a documented, measured macro that a build may override
    assert re.search(r"#ifndef MLDSA_VFY_PART_OPS\n#define MLDSA_VFY_PART_OPS \d+\n#endif", text)
    assert _vfy_lib.part_ops() >= 64 and "profiles/vfy_layer_ab.jsonl" in text
    # what the pass promises: A_hat per op, the core's stage names, the way back into the core
    for word in ("derived again for every op", "expand_a, verify_main,", "ctilde_hash, mu, sample_in_ball", "folds back into the core"):
        assert word in text, word


def test_layered_on_the_one_core_library(vfy):
    layered_on_core(
        _vfy_lib.LIB_PATH,
        # (the two generators of the NTT twiddle tables are the core's, ../csrc/tables.h)
        needs=("mldsa_ctx_device", "mldsa_get_params", "_ZN5mldsa21gen_fwd_lane_twiddlesEv", "_ZN5mldsa21gen_inv_lane_twiddlesEv"),
        # the pass is the library's own: no op-level or seam call of the core's, and nothing of another layer
        never=("mldsa_verify", "mldsa_verify_cached_a", "mldsa_verify_pk", "mldsa_expand_a", "mldsa_sample_in_ball", "mldsa_verify_arith",
               "mldsa_verify_mu", "mldsa_mu_compute", "mldsa_prehash"))
    links_the_core_and_never_builds_it(VFY_DIR)
    dyn = subprocess.run(["readelf", "-d", _vfy_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck)\.so", dyn)


def _formula(part):
    params = core_params()

    def up(x):
        return (x + 255) // 256 * 256

    def f(pset, n):
        if pset not in KL:
            return 0
        k, l = KL[pset]
        half = min(n, part)
        halves = 2 if n > part else 1
        return (halves * up(half * k * l * 768) + up(n * 256) + 5 * up(n * 4) + up(n * (64 + params[pset].w1_len)) + 256)
    return f


def test_scratch_bytes(vfy):
    assert vfy.mldsa_vfy_set_part_ops(0) >= 64  # the default is in force
    try:
        for part in (_vfy_lib.part_ops(), 64, 4096):
            vfy.mldsa_vfy_set_part_ops(part)
            scratch_sweep(vfy.mldsa_vfy_scratch_bytes, _formula(part), _vfy_lib.MAX_OPS)
        # the ring of 4 096-op parts of ML-DSA-65: 2 x 92 MB where the core keeps 1.5 GB of A_hat for 65 536 ops
        vfy.mldsa_vfy_set_part_ops(4096)
        assert vfy.mldsa_vfy_scratch_bytes(65, 65536) < 2 * 4096 * 30 * 768 + 65536 * 1200
    finally:
        assert vfy.mldsa_vfy_set_part_ops(0) == 4096
    assert vfy.mldsa_vfy_set_part_ops(0) == _vfy_lib.part_ops()


def test_argument_errors_never_abort(vfy):
    null = None
    buf, p, odd = aligned_buffer()
    big = 1 << 50
    err = vfy.mldsa_vfy_last_error

    def verify(ctx=null, pset=65, mode=0, rho=p, tr=p, t1=p, n_keys=4, kidx=null, msgs=p, moff=p, ctxs=null, coff=null, sigs=p, ok=p, n=4,
               scratch=p, sb=big, stream=null):
        return vfy.mldsa_vfy_verify(ctx, pset, mode, rho, tr, t1, n_keys, kidx, msgs, moff, ctxs, coff, sigs, ok, n, scratch, sb, stream)

    def expand(ctx=null, pset=65, rho=p, a_hat=p, n=4, stream=null):
        return vfy.mldsa_vfy_expand_a(ctx, pset, rho, a_hat, n, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    assert verify() == _lib.ERR_PARAM and b"NULL context" in err()
    assert expand() == _lib.ERR_PARAM and b"NULL context" in err()
    assert vfy.mldsa_vfy_profile_enable(null, 1) == _lib.ERR_PARAM and b"NULL context" in err()
    assert vfy.mldsa_vfy_profile_report(null, C.create_string_buffer(64), 64) == _lib.ERR_PARAM and b"NULL context" in err()
    # a fake non-NULL context must still be refused before it is touched
    fake = p
    for pset in (0, 43, 66, -1):
        assert verify(ctx=fake, pset=pset) == _lib.ERR_PARAM and b"unknown parameter set" in err()
        assert expand(ctx=fake, pset=pset) == _lib.ERR_PARAM and b"unknown parameter set" in err()
    for mode in (-1, 3, 99):
        assert verify(ctx=fake, mode=mode) == _lib.ERR_PARAM and b"bad mode" in err()
        assert verify(ctx=fake, mode=mode, n=0) == _lib.ERR_PARAM
    for kw in (dict(rho=null), dict(tr=null), dict(t1=null), dict(moff=null), dict(sigs=null), dict(ok=null)):
        assert verify(ctx=fake, **kw) == _lib.ERR_PARAM and err() == b"mldsa_vfy_verify: NULL pointer", kw
    # the key table covers the batch: with key_idx any non-empty table, without one a key per op
    assert verify(ctx=fake, n_keys=3) == _lib.ERR_PARAM and b"n_keys does not cover the batch" in err()
    assert verify(ctx=fake, n_keys=0, kidx=p) == _lib.ERR_PARAM and b"n_keys does not cover the batch" in err()
    assert verify(ctx=fake, n=_vfy_lib.MAX_OPS + 1, n_keys=1 << 40) == _lib.ERR_PARAM and b"MLDSA_VFY_MAX_OPS" in err()
    assert verify(ctx=fake, t1=odd) == _lib.ERR_PARAM and b"16-byte aligned" in err()
    assert verify(ctx=fake, scratch=null) == _lib.ERR_PARAM and b"scratch is NULL or not 256-byte aligned" in err()
    assert verify(ctx=fake, scratch=odd) == _lib.ERR_PARAM and b"scratch is NULL or not 256-byte aligned" in err()
    for kw in (dict(rho=null), dict(a_hat=null)):
        assert expand(ctx=fake, **kw) == _lib.ERR_PARAM and err() == b"mldsa_vfy_expand_a: NULL pointer", kw
    assert expand(ctx=fake, a_hat=odd) == _lib.ERR_PARAM and b"16-byte aligned" in err()
    assert expand(ctx=fake, n=_vfy_lib.MAX_OPS + 1) == _lib.ERR_PARAM and b"MLDSA_VFY_MAX_OPS" in err()
    assert vfy.mldsa_vfy_profile_report(fake, null, 64) == _lib.ERR_PARAM and b"bad argument" in err()
    assert vfy.mldsa_vfy_profile_report(fake, C.create_string_buffer(2), 2) == _lib.ERR_PARAM and b"bad argument" in err()
    # empty calls succeed, with a context that is never touched
    assert verify(ctx=fake, n=0, rho=null, tr=null, t1=null, moff=null, sigs=null, ok=null, scratch=null, sb=0) == _lib.OK
    assert expand(ctx=fake, n=0, rho=null, a_hat=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(vfy):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    mine, theirs = b"mldsa_vfy_expand_a: NULL pointer", b"mldsa_mus_final: NULL pointer"
    assert vfy.mldsa_vfy_expand_a(p, 65, null, p, 4, null) == _lib.ERR_PARAM and vfy.mldsa_vfy_last_error() == mine
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() == theirs
    assert vfy.mldsa_vfy_last_error() == mine
    assert vfy.mldsa_vfy_expand_a(p, 65, null, p, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() == theirs
    # nothing of the shared scaffold is exported
    out = subprocess.run(["nm", "-D", "--defined-only", _vfy_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "largest_pass", "mldsa_layer", "g_states", "g_mutex"):
        assert word not in out, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(vfy):
    kernels = kernel_resources(VFY_DIR)
    # the name-based tools find the two big kernels under the core's names, inside the library's namespace, once per parameter set
    for stem, count in (("9mldsa_vfy10k_expand_aI", 3), ("9mldsa_vfy13k_verify_mainI", 3), ("9mldsa_vfy16k_ctilde_verdictI", 3),
                        ("9mldsa_vfy16k_sample_in_ballI", 3), ("9mldsa_vfy4k_mu", 1), ("9mldsa_vfy15k_sanitize_keys", 1), ("9mldsa_vfy10k_unpack_a", 1)):
        assert sum(stem in nm for nm in kernels) == count, stem
    assert len(kernels) == 15
    # ExpandA is compiled for five waves per SIMD and fits them without a spill (102 VGPRs at most)
    res = open(os.path.join(VFY_DIR, "vfy.res")).read()
    found = re.findall(r"Function Name: \S*k_expand_aI[^\n]*\n(?:[^\n]*\n)*?[^\n]* VGPRs: (\d+)[^\n]*\n(?:[^\n]*\n)*?[^\n]*Occupancy \[waves/SIMD\]: (\d+)", res)
    assert len(found) == 3 and all(int(v) <= 102 and int(o) == 5 for v, o in found), found
    assert "amdgpu_waves_per_eu(MLDSA_VFY_EA_WAVES, MLDSA_VFY_EA_WAVES)" in open(os.path.join(VFY_DIR, "vfy.hip")).read()
    assert len(re.findall(r"Function Name: \S*k_expand_aI", res)) == 3
    # the empty asm statements of k_verify_main are the core's (the opaque lane index, the LDS twiddle reads kept in place): asm_free=False
    read = sources_clean(VFY_DIR, ["../../include/mldsa_vfy.h", "../_vfy_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"], asm_free=False)
    src = includes_the_core_device_headers(VFY_DIR, "vfy.hip")
    for h in ("../layer/layer_host.h", "../csrc/challenge_dev.h", "../csrc/ntt_wave.h", "../csrc/sampler_dev.h", "../csrc/verify_dev.h",
              "keccak180.h", "vfy_parts.h"):
        assert f'#include "{h}"' in src, h
    texts = dict(read)
    for f in ("vfy.hip", "keccak180.h", "vfy_parts.h"):
        t = texts[f]
        # every asm statement is empty; only stream events order the work: no flag another kernel waits for, no spin loop, no wave sleep
        assert all(m == '""' for m in re.findall(r"asm volatile\((\"[^\"]*\")", t)), f
        assert len(re.findall(r"\basm\b", t)) == len(re.findall(r"asm volatile\(\"\"", t)), f
        for word in ("struct DeviceScope", "thread_local", "int fail(", "atomicAdd", "atomicCAS", "s_sleep", "while (true)", "for (;;)",
                     "__threadfence", "hipGraph", "hipStreamBeginCapture"):
            assert word not in t, (f, word)
    # the folded round: no D array, theta applied with xor3; rho / pi / chi / iota as in keccak.h
    k180 = texts["keccak180.h"]
    code = re.sub(r"//[^\n]*", "", k180)
    assert "dlo" not in code and "dhi" not in code and code.count("mldsa::xor3(") == 6 and "mldsa::chi(" in code and "mldsa::rotl64<ROT>" in code
    assert code.count("VFY_RHOPI(") == 25 + 1 and "keccak_f1600_180(st)" in code and "Packed3Unaligned" in code
    assert texts["vfy.hip"].count("180(") == 1  # only ExpandA runs on it; the other hashes are the core's
    # the plan has no HIP in it
    plan = texts["vfy_parts.h"]
    assert "hip" not in re.sub(r"//[^\n]*", "", plan).lower() and "__device__" not in plan and "__global__" not in plan
    # at most three streams in flight: the caller's and the library's two
    assert src.count("hipStreamCreateWithFlags(") == 2


def test_routing_constants():
    from fips204_amd import ml_dsa
    text = open(os.path.join(ROOT, "fips204_amd", "ml_dsa.py")).read()
    # never below the core's single-launch limit (MLDSA_OPT_SMALL_FUSED = 256 ops), measured, with the file the value came from
    assert sorted(ml_dsa.VFY_MIN_OPS) == [44, 65, 87] and all(1024 <= v <= 65536 for v in ml_dsa.VFY_MIN_OPS.values())
    assert "profiles/vfy_layer_ab.jsonl" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"VFY_MIN_OPS = {ml_dsa.VFY_MIN_OPS}" in design and f"MLDSA_VFY_PART_OPS = {_vfy_lib.part_ops()}" in design
    rows = [ln for ln in open(os.path.join(ROOT, "profiles", "vfy_layer_ab.jsonl")) if ln.strip()]
    assert len(rows) >= 6
    # the thresholds come from rows measured on the library as it ships (ExpandA at the waves per SIMD the source is compiled for)
    waves = re.search(r"#define MLDSA_VFY_EA_WAVES (\d)", open(os.path.join(VFY_DIR, "vfy.hip")).read()).group(1)
    import json as _json
    shipped = [r for r in map(_json.loads, rows) if r.get("kind") == "min_ops" and r.get("build") == "w" + waves]
    for pset, lo in ml_dsa.VFY_MIN_OPS.items():
        at = [r for r in shipped if r["set"] == pset and r["n"] >= lo]
        assert len(at) >= 4 and all(r["vfy_ms"] < min(r["core_ms"], r["core_again_ms"]) for r in at), pset
    import json
    for ln in rows:
        json.loads(ln)


def test_the_part_plan_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "vfy_parts", ["vfy_parts_main.cpp"], "vfy_parts OK")
