"""The mu-stream library (include/mldsa_mus.h, fips204_amd/mus/libmldsa_mus.so) without a device: its C ABI, how it is linked against
the core, its host-only entry points, its kernels' resources and sources, the case generator of the GPU tests, and the chunk plan of
the host-memory call as a stand-alone program under the sanitizers."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import pytest

import mus_cases
from fips204_amd import _keycheck_lib, _keys_lib, _lib, _mu_lib, _mus_lib, _ph_lib, _seed_lib
from layer_checks import (ROOT, aligned_buffer, built, clean_build, header_and_exports, includes_the_core_device_headers, kernel_resources,
                          layered_on_core, links_the_core_and_never_builds_it, sanitized_program, sources_clean)

MUS_DIR = os.path.join(ROOT, "fips204_amd", "mus")
SOURCES = ["Makefile", "mus.hip"]


@pytest.fixture(scope="module")
def mus():
    return built(_mus_lib, MUS_DIR)


def test_clean_build_in_a_shadow_tree(mus, tmp_path):
    from fips204_amd import build
    assert build.LAYERS["mus"] == "libmldsa_mus.so" and build.MUS_LIB == _mus_lib.LIB_PATH
    clean_build("mus", _mus_lib, SOURCES, [os.path.join(build._HERE, d, f) for d, f in build.LAYERS.items()], tmp_path)
    mk = open(os.path.join(MUS_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(mus, tmp_path):
    declared, text = header_and_exports(
        _mus_lib, mus,
        "int main(void) { mldsa_mus_host *h = 0; mldsa_mus_host_destroy(h);\n"
        "  return mldsa_mus_abi_version() == MLDSA_MUS_ABI_VERSION && mldsa_mus_state_bytes(MLDSA_MUS_MAX_OPS) > MLDSA_MUS_WAVE_MAX_OPS ? 0 : 1; }\n",
        r"\b(mldsa_mus_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_mus_abi_version", "mldsa_mus_last_error", "mldsa_mus_state_bytes", "mldsa_mus_init", "mldsa_mus_update",
                        "mldsa_mus_final", "mldsa_mus_host_create", "mldsa_mus_host_destroy", "mldsa_mus_host_compute"}
    assert "#define MLDSA_MUS_ABI_VERSION 1" in text and mus.mldsa_mus_abi_version() == _mus_lib.ABI_VERSION == 1
    assert "#define MLDSA_MUS_MAX_OPS ((size_t)1 << 30)" in text and _mus_lib.MAX_OPS == 1 << 30
    # the threshold between the two kernel forms: a documented macro that a build may override, >= 0
    assert re.search(r"#ifndef MLDSA_MUS_WAVE_MAX_OPS\n#define MLDSA_MUS_WAVE_MAX_OPS \d+\n#endif", text)
    assert _mus_lib.wave_max_ops() >= 0 and "one op per WAVE" in text and "0 = never" in text
    # which pointers of the host-memory call are host pointers is said where it is declared
    assert "HOST pointers" in text and "DEVICE pointers" in text and "FIPS 204" in text


def test_layered_on_the_one_core_library(mus):
    layered_on_core(
        _mus_lib.LIB_PATH,
        needs=("mldsa_ctx_device", "mldsa_last_error", "mldsa_check_offsets"),
        # the core only: no op-level call, and nothing of another layer
        never=("mldsa_verify", "mldsa_sign", "mldsa_verify_host", "mldsa_sign_host", "mldsa_mu_compute", "mldsa_verify_mu", "mldsa_sign_mu",
               "mldsa_ph_update", "mldsa_xof"))
    links_the_core_and_never_builds_it(MUS_DIR)
    dyn = subprocess.run(["readelf", "-d", _mus_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|ph|keys|seed|keycheck)\.so", dyn)


def test_state_bytes(mus):
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 192, 264, 1000, 65536, 65537, 1 << 30):  # the ladder of layer_checks.scratch_sweep
        assert mus.mldsa_mus_state_bytes(n) == 208 * n == _mus_lib.STATE_BYTES_PER_OP * n
    for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
        assert mus.mldsa_mus_state_bytes(n) == 0
    assert "208 n_ops" in open(_mus_lib.HEADER_PATH).read()


def test_argument_errors_never_abort(mus):
    null = None
    buf, p, odd = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    big = 1 << 40
    err = mus.mldsa_mus_last_error

    def init(ctx=null, mode=0, tr=p, n_keys=4, kidx=null, ctxs=null, coff=null, state=p, sb=big, n=4, stream=null):
        return mus.mldsa_mus_init(ctx, mode, tr, n_keys, kidx, ctxs, coff, state, sb, n, stream)

    def update(ctx=null, state=p, sb=big, pieces=p, poff=p, n=4, stream=null):
        return mus.mldsa_mus_update(ctx, state, sb, pieces, poff, n, stream)

    def final(ctx=null, state=p, sb=big, mu=p, flag=null, n=4, stream=null):
        return mus.mldsa_mus_final(ctx, state, sb, mu, flag, n, stream)

    def compute(h=null, mode=0, tr=p, n_keys=4, kidx=null, msgs=p, moff=p, ctxs=null, coff=null, mu=p, flag=null, n=4):
        return mus.mldsa_mus_host_compute(h, mode, tr, n_keys, kidx, msgs, moff, ctxs, coff, mu, flag, n)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (init, update, final):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    assert compute() == _lib.ERR_PARAM and b"NULL mldsa_mus_host" in err()
    for mode in (-1, 3, 99):
        for call in (init, compute):
            assert call(mode=mode) == _lib.ERR_PARAM and b"unknown mode" in err()
            assert call(mode=mode, n=0) == _lib.ERR_PARAM
    # a fake non-NULL context (or object) must still be refused before it is touched
    fake = p
    assert init(ctx=fake, tr=null) == _lib.ERR_PARAM and b"mldsa_mus_init: NULL pointer" in err()
    assert update(ctx=fake, poff=null) == _lib.ERR_PARAM and b"mldsa_mus_update: NULL pointer" in err()
    assert final(ctx=fake, mu=null) == _lib.ERR_PARAM and b"mldsa_mus_final: NULL pointer" in err()
    for call, name in ((init, b"mldsa_mus_init"), (update, b"mldsa_mus_update"), (final, b"mldsa_mus_final")):
        assert call(ctx=fake, state=null) == _lib.ERR_PARAM and err() == name + b": NULL pointer"
        for bad in (odd4, C.c_void_p(p.value + 1)):
            assert call(ctx=fake, state=bad) == _lib.ERR_PARAM and b"not 8-byte aligned" in err()
        for n in (1, 4, 65, 1000):
            for sb in (0, 1, 208 * n - 1):
                assert call(ctx=fake, n=n, sb=sb) == _lib.ERR_PARAM and b"mldsa_mus_state_bytes" in err(), (n, sb)
        assert call(ctx=fake, n=(1 << 30) + 1, sb=1 << 62) == _lib.ERR_PARAM and b"MLDSA_MUS_MAX_OPS" in err()
    assert init(ctx=fake, n_keys=0) == _lib.ERR_PARAM and b"n_keys" in err()
    assert compute(h=fake, n_keys=0) == _lib.ERR_PARAM and b"n_keys" in err()
    assert compute(h=fake, n=(1 << 30) + 1) == _lib.ERR_PARAM and b"MLDSA_MUS_MAX_OPS" in err()
    for kw in (dict(tr=null), dict(moff=null), dict(mu=null)):
        assert compute(h=fake, **kw) == _lib.ERR_PARAM and b"mldsa_mus_host_compute: NULL pointer" in err(), kw
    # the host-memory call checks both tables before a byte is read: a decreasing entry, bytes of a NULL msgs / ctxs
    good = (C.c_uint64 * 5)(0, 3, 3, 10, 12)
    bad = (C.c_uint64 * 5)(0, 3, 2, 10, 12)
    g, b = C.cast(good, C.c_void_p), C.cast(bad, C.c_void_p)
    assert compute(h=fake, moff=b) == _lib.ERR_PARAM and b"mldsa_check_offsets(msg_off)" in err()
    assert compute(h=fake, moff=g, ctxs=p, coff=b) == _lib.ERR_PARAM and b"mldsa_check_offsets(ctx_off)" in err()
    assert compute(h=fake, moff=g, msgs=null) == _lib.ERR_PARAM and b"NULL msgs" in err()
    assert compute(h=fake, moff=g, ctxs=null, coff=g) == _lib.ERR_PARAM and b"NULL ctxs" in err()
    out = C.c_void_p(1)
    assert mus.mldsa_mus_host_create(null, 0, C.byref(out)) == _lib.ERR_PARAM and out.value is None and b"NULL pointer" in err()
    assert mus.mldsa_mus_host_create(fake, 0, None) == _lib.ERR_PARAM
    mus.mldsa_mus_host_destroy(null)  # a no-op
    # empty calls succeed without a context
    assert init(n=0, tr=null, state=null, sb=0) == _lib.OK and update(n=0, state=null, sb=0, poff=null) == _lib.OK
    assert final(n=0, state=null, sb=0, mu=null) == _lib.OK and compute(n=0, tr=null, moff=null, mu=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(mus):
    """six libraries in one thread: a failure here leaves the other five messages where they were, and theirs leave this one"""
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    others = {
        "seed": (lambda lib: lib.mldsa_seed_expand(null, 65, p, p, p, p, p, p, p, null, 4, p, big, null), _seed_lib, "mldsa_seed_last_error",
                 b"mldsa_seed_expand: NULL context"),
        "keycheck": (lambda lib: lib.mldsa_keypair_check(p, 7, p, null, p, 4, p, big, null), _keycheck_lib, "mldsa_keycheck_last_error",
                     b"mldsa_keypair_check: unknown parameter set"),
        "mu": (lambda lib: lib.mldsa_verify_mu(p, 65, null, p, 4, null, p, null, p, p, 4, p, big, null), _mu_lib, "mldsa_mu_last_error",
               b"mldsa_verify_mu: NULL pointer"),
        "keys": (lambda lib: lib.mldsa_keys_dedup(p, 65, p, 4, bytes(16), 65, p, p, 4, p, p, big, null), _keys_lib, "mldsa_keys_last_error",
                 b"mldsa_keys_dedup: hash_bits outside 1 ... 64"),
        "ph": (lambda lib: lib.mldsa_prehash(p, 99, p, p, p, null, 4, null), _ph_lib, "mldsa_ph_last_error", b"mldsa_prehash: unknown ph"),
    }
    mine = b"mldsa_mus_final: NULL pointer"
    fail_here = lambda: mus.mldsa_mus_final(p, p, big, null, null, 4, null)
    for name, (call, loader, last, message) in others.items():
        lib = loader.load()
        assert fail_here() == _lib.ERR_PARAM and mus.mldsa_mus_last_error() == mine
        assert call(lib) == _lib.ERR_PARAM and getattr(lib, last)() == message and message != mine
        assert mus.mldsa_mus_last_error() == mine, f"a failure in {name} overwrote the message of mus"
        assert fail_here() == _lib.ERR_PARAM and getattr(lib, last)() == message, f"a failure in mus overwrote the message of {name}"
    # nothing of the shared scaffold is exported
    out = subprocess.run(["nm", "-D", "--defined-only", _mus_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "largest_pass", "mldsa_layer"):
        assert word not in out, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(mus):
    kernels = kernel_resources(MUS_DIR)
    for stem in ("k_mus_init_lane", "k_mus_update_lane", "k_mus_final_lane", "k_mus_init_wave", "k_mus_update_wave", "k_mus_final_wave"):
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) >= 6
    read = sources_clean(MUS_DIR, ["../../include/mldsa_mus.h", "../_mus_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h", "../layer/host_feed.h",
                               "../layer/host_chunks.h"], asm_free=True)
    src = includes_the_core_device_headers(MUS_DIR, "mus.hip")
    assert '#include "../layer/layer_host.h"' in src and '#include "../csrc/keccak_coop2.h"' in src and '#include "../layer/host_chunks.h"' in src
    assert '#include "../layer/host_feed.h"' in src
    # the scaffold is the layers' shared one; no spin waits, no atomics, no wave sleeps
    for f, t in read:
        if f in ("mus.hip", "../layer/host_chunks.h"):
            for word in ("struct DeviceScope", "thread_local", "int fail(", "atomic", "s_sleep", "__builtin_amdgcn_s_", "while (true)", "volatile"):
                assert word not in t, (f, word)
    # the chunk plan has no HIP in it, and the kernels clip by its two functions
    plan = dict(read)["../layer/host_chunks.h"]
    assert "hip" not in re.sub(r"//[^\n]*", "", plan).lower() and "__device__" not in plan and "__global__" not in plan
    assert src.count("piece_lo(p0, win_lo)") == 2 and src.count("piece_hi(p1, win_hi)") == 2
    # the wave form runs on the core's interleaved cooperative sponge, converted at load, absorb and store
    for word in ("keccak_f1600_coop2", "coop2_from_lohi", "coop2_to_lohi", "mldsa::keccak_f1600(ks)"):
        assert word in src, word


@pytest.mark.parametrize("mode", mus_cases.MODES)
def test_the_case_generator_covers_what_the_gpu_tests_rely_on(mode):
    from fips204_amd.ml_dsa import external_mu
    ops = mus_cases.cases(mode)
    sched = mus_cases.schedules(ops, mode)
    assert len(ops) == (74 if mode == mus_cases.MODE_INTERNAL else 154)
    assert len(sched) == 1 + 12 + 1 + 3 and len(sched["bytes"][1][0]) == 301
    ctx_lens = {len(c) for c, _ in ops}
    assert ctx_lens == ({0} if mode == mus_cases.MODE_INTERNAL else set(mus_cases.CTX_LENS))
    assert sum(len(m) == mus_cases.BIG for _, m in ops) == 2 and len(ops[-1][1]) == 0
    cov = mus_cases.coverage(ops, sched, mode)
    assert len(cov) == (8 if mode == mus_cases.MODE_INTERNAL else 10)
    for name, count in cov.items():
        assert count > 0, name
    # the reference: hashlib fed the same pieces is external_mu() on the whole message, for every schedule
    trs = [hashlib.shake_256(b"mus-tr" + bytes([i % 7])).digest(64) for i in range(len(ops))]
    whole = [external_mu(trs[i], m, c, mode) for i, (c, m) in enumerate(ops)]
    for name, (idx, cuts) in sched.items():
        if name == "bytes" or name.startswith("random") or name in ("one_piece", "cut_0R-1", "cut_1R+0", "cut_3R+1"):
            assert mus_cases.hashlib_incremental(ops, trs, mode, idx, cuts) == [whole[i] for i in idx], name
    # a prefix of the updates is the mu of the prefix of the message
    idx, cuts = sched["random_2"]
    part = mus_cases.hashlib_incremental(ops, trs, mode, idx, cuts, upto=4)
    assert part == [external_mu(trs[i], ops[i][1][:cs[4]], ops[i][0], mode) for i, cs in zip(idx, cuts)]
    # HOST_LENS are those of the pre-hash host tests, and give what the host-fed test asserts with 4096-byte staging
    import numpy as np
    off = np.concatenate([[0], np.cumsum(mus_cases.HOST_LENS)])
    assert len(mus_cases.HOST_LENS) == 24 and max(mus_cases.HOST_LENS) == 200 << 10
    assert max((off[i + 1] - 1) // 4096 - off[i] // 4096 + 1 for i in range(24) if mus_cases.HOST_LENS[i]) > 40
    assert max(sum(1 for i in range(24) if mus_cases.HOST_LENS[i] and off[i] < c + 4096 and off[i + 1] > c) for c in range(0, int(off[-1]), 4096)) > 3


def test_the_chunk_plan_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "mus_chunks", ["host_chunks_main.cpp"], "mus_chunks OK")
