"""The request-signing library (include/mldsa_recsign.h, fips204_amd/recsign/libmldsa_recsign.so) without a device: its C ABI, how it is
linked against the core, its scratch formulas, its argument checks, its kernels' resources and sources, the numpy restatement of
tests/recsign_cases.py against the oracle, and the descriptor check and the scatter's copy plan as a stand-alone program under the
sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import recsign_cases as rs
from fips204_amd import _lib, _mus_lib, _recsign_lib
from fips204_amd.ml_dsa import sign_requests_blob
from layer_checks import (ROOT, aligned_buffer, built, clean_build, core_params, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, shared_plan_is_shared_once,
                          sources_clean)
from oracle import oracle as orc

RECSIGN_DIR = os.path.join(ROOT, "fips204_amd", "recsign")
SOURCES = ["Makefile", "recsign.hip", "recsign_plan.h"]
LADDER = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 65536, 65537, 1 << 30)


@pytest.fixture(scope="module")
def recsign():
    return built(_recsign_lib, RECSIGN_DIR)


def test_clean_build_in_a_shadow_tree(recsign, tmp_path):
    from fips204_amd import build
    assert len(build.LAYERS) == 8 and list(build.LAYERS)[-1] == "vfy" and "recsign" not in build.LAYERS
    assert build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"}
    assert build.RECSIGN_LIB == _recsign_lib.LIB_PATH and build.RECSIGN_DIR == RECSIGN_DIR
    # recsign_plan.h includes ../rec/rec_plan.h and recsign.hip the shared plan (../rec/rec_scan.h, ../rec/rec_host.h): the shadow links rec/ too
    (tmp_path / "fips204_amd").mkdir()
    os.symlink(build.REC_DIR, tmp_path / "fips204_amd" / "rec")
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS}.items()]
    clean_build("recsign", _recsign_lib, SOURCES, libs, tmp_path)  # build() builds it: the library is there after build()
    mk = open(os.path.join(RECSIGN_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../rec/rec_plan.h", "../rec/rec_scan.h", "../rec/rec_wave.h", "../rec/rec_host.h"):
        assert h in mk, h  # a change of the shared plan rebuilds this library
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_recsign_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(recsign, tmp_path):
    declared, text = header_and_exports(
        _recsign_lib, recsign,
        "int main(void) { mldsa_recsign_op o; mldsa_recsign_totals t; mldsa_recsign_packed p; mldsa_recsign_info i; mldsa_recsign_keys k[3];\n"
        "  o.set = MLDSA_65; o.flags = MLDSA_RECSIGN_RND; o.reserved = 0; t.n[MLDSA_RECSIGN_CLASS_REFUSED] = 0; p.c[MLDSA_RECSIGN_CLASS_87].n = 0;\n"
        "  p.rnd_region_bytes = 0; i.scratch_needed = 0; k[2].n_keys = 0;\n"
        "  return sizeof(mldsa_recsign_op) == 48 && sizeof(t) == 80 && mldsa_recsign_abi_version() == MLDSA_RECSIGN_ABI_VERSION && o.set && o.flags\n"
        "    && !t.n[3] && !p.c[2].n && !p.rnd_region_bytes && !i.scratch_needed && !k[2].n_keys\n"
        "    && mldsa_recsign_front_bytes(MLDSA_RECSIGN_MAX_OPS) > MLDSA_RECSIGN_SCAN_BLOCK ? 0 : 1; }\n",
        r"\b(mldsa_recsign_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_recsign_abi_version", "mldsa_recsign_last_error", "mldsa_recsign_plan", "mldsa_recsign_plan_bytes",
                        "mldsa_recsign_pack", "mldsa_recsign_arena_bytes", "mldsa_recsign_arena_bytes_max", "mldsa_recsign_scatter",
                        "mldsa_recsign_sign", "mldsa_recsign_front_bytes"}
    # the Python constants and layouts are the header's
    assert "#define MLDSA_RECSIGN_ABI_VERSION 1" in text and recsign.mldsa_recsign_abi_version() == _recsign_lib.ABI_VERSION == 1
    assert "#define MLDSA_RECSIGN_MAX_OPS ((size_t)1 << 30)" in text and _recsign_lib.MAX_OPS == 1 << 30
    assert f"#define MLDSA_RECSIGN_SCAN_BLOCK {_recsign_lib.SCAN_BLOCK}" in text and rs.SCAN_BLOCK == _recsign_lib.SCAN_BLOCK
    assert f"#define MLDSA_RECSIGN_RND {_recsign_lib.FLAG_RND}" in text and rs.FLAG_RND == _recsign_lib.FLAG_RND == 1
    for c, name in enumerate(("44", "65", "87", "REFUSED")):
        assert f"#define MLDSA_RECSIGN_CLASS_{name} {c}" in text
    assert (_recsign_lib.CLASS_44, _recsign_lib.CLASS_65, _recsign_lib.CLASS_87, _recsign_lib.CLASS_REFUSED) == (0, 1, 2, 3)
    assert _recsign_lib.OP_DTYPE.itemsize == 48 and C.sizeof(_recsign_lib.RecsignTotals) == 80 and C.sizeof(_recsign_lib.RecsignInfo) == 56
    assert C.sizeof(_recsign_lib.RecsignPacked) == 3 * 9 * 8 + 16 and C.sizeof(_recsign_lib.RecsignKeys) == 7 * 8
    names = ("msg_off", "ctx_off", "rnd_off", "sig_off", "msg_len", "key", "ctx_len", "set", "flags", "reserved")
    assert [_recsign_lib.OP_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 36, 40, 42, 43, 44]
    # the status codes and the lengths the restatement uses are the core's
    assert (rs.OK, rs.ERR_PARAM, rs.ERR_CTX_LEN) == (_lib.OK, _lib.ERR_PARAM, _lib.ERR_CTX_LEN)
    params = core_params()
    for pset in (44, 65, 87):
        assert params[pset].sig_len == rs.SIG_LEN[pset]
    # rnd is named as the scratch's only secret, and a measurement is stated only where its file exists
    assert "rnd is the only secret the" in text and "ONLY secret the scratch ever holds" in text
    if not os.path.exists(os.path.join(ROOT, "profiles", "recsign_bench.jsonl")):
        assert "not measured" in text
        readme = open(os.path.join(ROOT, "README.md")).read()
        row = [ln for ln in readme.splitlines() if "libmldsa_recsign.so" in ln and ln.startswith("|")]
        assert row and all("not measured" in ln.lower() for ln in row)


def test_layered_on_the_one_core_library(recsign):
    dyn_syms = subprocess.run(["nm", "-D", _recsign_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    undefined = {ln.split()[-1] for ln in dyn_syms.splitlines() if " U " in ln}
    core = [n for n in undefined if n.startswith("mldsa_")]
    never = [n for n in _lib.declared_symbols() if n.startswith(("mldsa_verify", "mldsa_keygen", "mldsa_sk_expand"))]
    assert len(never) > 5 and "mldsa_verify_pk" in never and "mldsa_keygen" in never and "mldsa_sk_expand" in never
    layered_on_core(_recsign_lib.LIB_PATH, needs=("mldsa_sign", "mldsa_memset", "mldsa_ctx_device", "mldsa_last_error"), never=never)
    # every signature is mldsa_sign's: the one signing call of the core's, no other op-level or seam call
    assert sorted(core) == ["mldsa_ctx_device", "mldsa_last_error", "mldsa_memset", "mldsa_sign"], core
    links_the_core_and_never_builds_it(RECSIGN_DIR)
    dyn = subprocess.run(["readelf", "-d", _recsign_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec)\.so", dyn)


def test_scratch_sizes_follow_the_documented_formulas(recsign):
    last = 0
    for n in LADDER:
        assert recsign.mldsa_recsign_plan_bytes(n) == rs.plan_bytes(n), n
        assert recsign.mldsa_recsign_front_bytes(n) == rs.front_bytes(n) >= last, n
        last = rs.front_bytes(n)
    bytes_ladder = (0, 1, 255, 256, 257, 10 ** 6, 1 << 40)
    for n44 in LADDER:
        for n65, n87 in ((0, 0), (1, 0), (0, 1), (n44, n44), (65, 257), (1 << 30, 3)):
            last = 0
            for mb in bytes_ladder:
                cb = 255 * min(n44 + n65 + n87, 1000)
                want = rs.arena_bytes(n44, n65, n87, mb, cb)
                assert recsign.mldsa_recsign_arena_bytes(n44, n65, n87, mb, cb) == want >= last, (n44, n65, n87, mb)
                last = want
                n = n44 + n65 + n87
                if n <= 1 << 30:  # the bound covers every mix of n ops, and stays close to the all-87 mix
                    bound = recsign.mldsa_recsign_arena_bytes_max(n, mb, cb)
                    assert bound == rs.arena_bytes_max(n, mb, cb) and bound >= want, (n44, n65, n87, mb)
                    for mix in ((0, 0, n), (n, 0, 0), (0, n, 0), (n // 3, n // 3, n - 2 * (n // 3)), (1 if n else 0, 0, max(n - 1, 0)), (0, 0, 0)):
                        assert bound >= rs.arena_bytes(*mix, mb, cb), (n, mix)
                    assert bound < rs.arena_bytes(0, 0, n, mb, cb) + 4096
    last = 0
    for n in LADDER:  # monotonic in n
        bound = recsign.mldsa_recsign_arena_bytes_max(n, 1000, 10)
        assert bound >= last and recsign.mldsa_recsign_arena_bytes(0, n, 0, 1000, 10) <= bound
        last = bound
    # an even three-way mix of 65 536 ops with 32-byte messages: about what the signatures take
    assert recsign.mldsa_recsign_arena_bytes(21846, 21845, 21845, 32 * 65536, 0) < 65536 * 3600  # (3452 on average, + 32 + 32 + 24 + ...)
    # past MLDSA_RECSIGN_MAX_OPS, or a size that does not fit: 0
    big = (1 << 30) + 1
    for args in ((big, 0, 0, 0, 0), (0, big, 0, 0, 0), (0, 0, big, 0, 0), (0, 0, 2 ** 63, 0, 0), (1, 1, 1, 2 ** 63, 0), (1, 1, 1, 0, 2 ** 64 - 1)):
        assert recsign.mldsa_recsign_arena_bytes(*args) == 0, args
    for args in ((big, 0, 0), (2 ** 64 - 1, 0, 0), (1, 2 ** 63, 0), (1, 0, 2 ** 64 - 1)):
        assert recsign.mldsa_recsign_arena_bytes_max(*args) == 0, args
    for n in (big, 2 ** 63, 2 ** 64 - 1):
        assert recsign.mldsa_recsign_plan_bytes(n) == 0 and recsign.mldsa_recsign_front_bytes(n) == 0


def test_argument_errors_never_abort(recsign):
    null = None
    buf, p, odd = aligned_buffer()
    odd4, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    big = 1 << 50
    err = recsign.mldsa_recsign_last_error
    nk = (C.c_size_t * 3)(4, 4, 4)
    tot = _recsign_lib.RecsignTotals()
    tot.n[:] = [2, 1, 1, 0]
    packed, info = _recsign_lib.RecsignPacked(), _recsign_lib.RecsignInfo()
    for c in range(3):
        packed.c[c].n, packed.c[c].sigs, packed.c[c].status = 1, p.value, p.value
    keys = (_recsign_lib.RecsignKeys * 3)()
    for c in range(3):
        keys[c].n_keys = 4
        keys[c].rho = keys[c].cap_k = keys[c].tr = keys[c].s_1_hat_mont = keys[c].s_2_hat_mont = keys[c].t_0_hat_mont = p.value

    def plan(ctx=null, blob_len=4096, out_len=4096, ops=p, n=4, n_keys=nk, cs=p, totals=p, pl=p, pb=big, stream=null):
        return recsign.mldsa_recsign_plan(ctx, blob_len, out_len, ops, n, n_keys, cs, totals, pl, pb, stream)

    def pack(ctx=null, blob=p, blob_len=4096, out_len=4096, ops=p, n=4, n_keys=nk, cs=p, pl=p, pb=big, totals=C.byref(tot), arena=p, ab=big,
             out=C.byref(packed), stream=null):
        return recsign.mldsa_recsign_pack(ctx, blob, blob_len, out_len, ops, n, n_keys, cs, pl, pb, totals, arena, ab, out, stream)

    def scatter(ctx=null, ops=p, n=4, blob_len=4096, out=p, out_len=4096, n_keys=nk, cs=p, pk=C.byref(packed), status=p, stream=null):
        return recsign.mldsa_recsign_scatter(ctx, ops, n, blob_len, out, out_len, n_keys, cs, pk, status, stream)

    def sign(ctx=null, mode=0, k=keys, blob=p, blob_len=4096, ops=p, n=4, out=p, out_len=4096, status=p, scratch=p, sb=big, inf=C.byref(info),
             stream=null):
        return recsign.mldsa_recsign_sign(ctx, mode, k, blob, blob_len, ops, n, out, out_len, status, scratch, sb, inf, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (plan, pack, scatter, sign):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    # a fake non-NULL context must still be refused before it is touched
    fake = p
    for call in (plan, pack, scatter, sign):
        assert call(ctx=fake, ops=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, ops=odd4) == _lib.ERR_PARAM and b"ops must be 8-byte aligned" in err()
        assert call(ctx=fake, n=_recsign_lib.MAX_OPS + 1) == _lib.ERR_PARAM and b"MLDSA_RECSIGN_MAX_OPS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_RECSIGN_MAX_OPS" in err()
    for call in (plan, pack, scatter):
        assert call(ctx=fake, n_keys=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, n_keys=(C.c_size_t * 3)(4, 2 ** 32, 4)) == _lib.ERR_PARAM and b"n_keys above UINT32_MAX" in err()
        assert call(ctx=fake, cs=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, cs=odd2) == _lib.ERR_PARAM and b"aligned" in err()
    for call in (pack, sign):  # a NULL blob is an empty blob's: only with blob_len > 0 is it an error
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert plan(ctx=fake, totals=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert plan(ctx=fake, totals=odd4) == _lib.ERR_PARAM and b"aligned" in err()
    need = recsign.mldsa_recsign_plan_bytes(4)
    for kw in (dict(pl=null), dict(pl=odd), dict(pb=need - 1), dict(pb=0)):
        assert plan(ctx=fake, **kw) == _lib.ERR_PARAM and b"plan is NULL" in err(), kw
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"plan is NULL" in err(), kw
    for kw in (dict(totals=null), dict(out=null)):
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL pointer" in err(), kw
    assert pack(ctx=fake, n=5) == _lib.ERR_PARAM and b"totals do not describe" in err()  # 2 + 1 + 1 + 0 ops
    for kw in (dict(arena=null), dict(arena=odd)):
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"arena is NULL or not 256-byte aligned" in err(), kw
    assert pack(ctx=fake, ab=recsign.mldsa_recsign_arena_bytes(2, 1, 1, 0, 0) - 1) == _lib.ERR_NOMEM and b"arena smaller" in err()
    for kw in (dict(out=null), dict(pk=null), dict(status=null)):
        assert scatter(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL pointer" in err(), kw
    assert scatter(ctx=fake, status=odd2) == _lib.ERR_PARAM and b"aligned" in err()
    assert scatter(ctx=fake, n=0) == _lib.OK
    packed.c[1].n = 5
    assert scatter(ctx=fake) == _lib.ERR_PARAM and b"packed does not describe" in err()
    packed.c[1].n, packed.c[1].sigs = 1, None
    assert scatter(ctx=fake) == _lib.ERR_PARAM and b"packed does not describe" in err()
    for mode in (-1, 3, 99):  # refused before anything is launched, as the core does
        assert sign(ctx=fake, mode=mode) == _lib.ERR_PARAM and b"unknown mode" in err(), mode
    for kw in (dict(k=null), dict(out=null), dict(status=null)):
        assert sign(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL pointer" in err(), kw
    assert sign(ctx=fake, status=odd2) == _lib.ERR_PARAM and b"aligned" in err()
    for kw in (dict(scratch=null), dict(scratch=odd), dict(scratch=C.c_void_p(p.value + 128)), dict(sb=recsign.mldsa_recsign_front_bytes(4) - 1),
               dict(sb=0)):
        assert sign(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch is NULL" in err(), kw
    for field in ("rho", "cap_k", "tr", "s_1_hat_mont", "s_2_hat_mont", "t_0_hat_mont"):  # a served set with a NULL table pointer
        setattr(keys[1], field, None)
        assert sign(ctx=fake) == _lib.ERR_PARAM and b"key table has a NULL pointer" in err(), field
        setattr(keys[1], field, p.value)
    keys[2].n_keys = 2 ** 32
    assert sign(ctx=fake) == _lib.ERR_PARAM and b"n_keys above UINT32_MAX" in err()
    keys[2].n_keys = 4
    # empty calls succeed without a context, and touch nothing
    assert plan(n=0, ops=null, n_keys=null, cs=null, totals=null, pl=null, pb=0) == _lib.OK
    packed.c[1].n = 7
    assert pack(n=0, blob=null, ops=null, n_keys=null, cs=null, pl=null, pb=0, totals=null, arena=null, ab=0) == _lib.OK and packed.c[1].n == 0
    assert scatter(n=0, ops=null, out=null, n_keys=null, cs=null, pk=null, status=null) == _lib.OK
    assert sign(n=0, k=null, blob=null, ops=null, out=null, status=null, scratch=null, sb=0, inf=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(recsign):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    keys = (_recsign_lib.RecsignKeys * 3)()
    assert recsign.mldsa_recsign_sign(p, 7, keys, p, 16, p, 4, p, 16, p, p, big, null, null) == _lib.ERR_PARAM
    mine = recsign.mldsa_recsign_last_error()
    assert mine == b"mldsa_recsign_sign: unknown mode"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert recsign.mldsa_recsign_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _recsign_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "copy_plan", "check_op", "k_pack", "k_scatter"):
        assert word not in exported, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(recsign):
    kernels = kernel_resources(RECSIGN_DIR)
    for stem in ("k_classify", "k_offsets", "k_apply", "k_pack", "k_scatter"):
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == 5
    read = dict(sources_clean(RECSIGN_DIR, ["../../include/mldsa_recsign.h", "../_recsign_lib.py", "../layer/layer_host.h", "../rec/rec_plan.h",
                                            "../rec/rec_scan.h", "../rec/rec_wave.h", "../rec/rec_host.h"]))
    src, plan, scan, host = read["recsign.hip"], read["recsign_plan.h"], read["../rec/rec_scan.h"], read["../rec/rec_host.h"]
    wave = read["../rec/rec_wave.h"]
    for h in ("../layer/layer_host.h", "../../include/mldsa_recsign.h", "recsign_plan.h", "../rec/rec_scan.h", "../rec/rec_host.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../rec/rec_plan.h"' in plan and '#include "rec_plan.h"' not in src and "namespace mldsa_rec " not in src + plan
    # the kernel boundaries do the ordering: no atomics, no flag another workgroup waits for, no spin loop; the scaffold is shared, not copied
    for word in ("atomic", "__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "struct DeviceScope",
                 "thread_local", "int fail(", "getenv", "printf"):
        assert word not in src + plan + scan + wave + host, word
    assert not re.search(r"\basm\b", src + plan + scan + wave + host)
    # LDS (the per-wave partial sums of the two scan kernels only), the definitions and the includes of the shared plan
    shared_plan_is_shared_once(src, scan, wave, host, open(os.path.join(RECSIGN_DIR, "Makefile")).read(), "../rec/rec_scan.h", "../rec/rec_wave.h",
                               "../rec/rec_host.h")
    no_new_dynamic_symbol(_recsign_lib.LIB_PATH, "mldsa_recsign_")
    # the plan has no HIP in it, and neither file keeps a second copy of the shared arithmetic: they call rec_plan.h's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan
    own_code = re.sub(r"//[^\n]*", "", src)
    kernel_code = own_code + re.sub(r"//[^\n]*", "", scan + wave)
    for call in ("copy_plan(", "chunk_src(", "funnel16(", "check_op(", "in_range("):
        assert call in kernel_code and "constexpr" in plan, call
    host_code = own_code + re.sub(r"//[^\n]*", "", host)
    for name in ("copy_plan", "chunk_src", "funnel16", "funnel_at", "in_range", "sig_len", "class_of_set", "up256"):
        assert not re.search(r"constexpr[^;{]*\b%s\s*\(" % name, code + kernel_code + host_code), name  # used, not restated
    assert len(re.findall(r"constexpr Verdict check_op\(", code)) == 1 and "in_range(" in code and "sig_len(" in code
    assert "check_op(" in own_code  # the verdict function is called from the library's own file
    assert own_code.count("mldsa_sign(") == 1 and host_code.count("hipStreamSynchronize(") == 1
    assert "mldsa_memset(" in own_code  # the rnd rows are cleared


# ---- the restatement against the oracle ------------------------------------------------------------------------------------------
N_KEYS = rs.ORACLE_N_KEYS


@pytest.fixture(scope="module")
def oracle_requests():
    return rs.oracle_requests()


def oracle_signed(keys, packed):
    """{pset: sigs [n, SIG_LEN]}, {pset: status [n]}: the restated packed arrays signed by the oracle"""
    sigs, status = {}, {}
    for pset in rs.SETS:
        rows = [orc.sign_internal(pset, keys[pset][key][1], msg, rnd, ctx=ctx, mode=orc.MODE_PURE) for key, msg, ctx, rnd in rs.requests_of(packed[pset])]
        sigs[pset] = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, rs.SIG_LEN[pset])
        status[pset] = np.zeros(len(rows), dtype=np.int32)
    return sigs, status


@pytest.mark.parametrize("in_place", [False, True])
def test_restated_output_holds_the_oracles_signatures(oracle_requests, in_place):
    q = oracle_requests
    for front, gaps in ((0, 0), (1, list(range(16))), (3, [5, 0, 11])):
        blob, ops, out_len = sign_requests_blob(q["requests"], pad=gaps, front=front, in_place=in_place)
        assert out_len == blob.size if in_place else out_len != blob.size
        want = rs.expected(blob, ops, N_KEYS, out_len)
        assert want["totals"][:4] == [4, 4, 4, 0] and not want["status"].any()
        assert [int(x) >> 30 for x in want["class_slot"]] == [0, 1, 2] * 4 and [int(x) & 0x3FFFFFFF for x in want["class_slot"]] == \
            [i // 3 for i in range(12)]
        for c, pset in enumerate(rs.SETS):  # slots follow input order; no flag = 32 zero bytes
            assert [r[1] for r in rs.requests_of(want["packed"][pset])] == [q["requests"][i][2] for i in range(c, 12, 3)]
            assert [r[3] for r in rs.requests_of(want["packed"][pset])] == [q["requests"][i][4] or bytes(32) for i in range(c, 12, 3)]
        before = blob if in_place else np.full(out_len, 0xC3, dtype=np.uint8)
        out, status = rs.scattered(before, ops, want, *oracle_signed(q["keys"], want["packed"]))
        assert not status.any()
        untouched = np.ones(out_len, dtype=bool)
        for i, (pset, key, msg, ctx, rnd) in enumerate(q["requests"]):
            at = int(ops[i]["sig_off"])
            sig = out[at:at + rs.SIG_LEN[pset]].tobytes()
            assert sig == q["sigs"][i], i  # the oracle's signature for the request's own inputs
            assert orc.verify_internal(pset, q["keys"][pset][key][0], msg, sig, ctx=ctx, mode=orc.MODE_PURE), i
            untouched[at:at + rs.SIG_LEN[pset]] = False
        assert np.array_equal(out[untouched], before[untouched])  # every other byte is as it was


def test_restated_output_with_four_damaged_descriptors(oracle_requests):
    q = oracle_requests
    blob, ops, out_len = sign_requests_blob(q["requests"], pad=list(range(16)), front=2, in_place=True)
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, rs.PATTERN, dtype=np.uint8)])
    out_len = blob.size
    ops = ops.copy()
    damage = {2: "ctx_len_256", 4: "key_is_n_keys", 7: "rnd_one_past_end", 9: "flag_bit_1"}
    for i, name in damage.items():
        rs.make_refused(ops, i, name, blob.size, out_len, region, N_KEYS)
    want = rs.expected(blob, ops, N_KEYS, out_len)
    assert want["totals"][:4] == [3, 2, 3, 4]  # ops 9 (44), 4 and 7 (65), 2 (87) are refused
    assert want["status"].tolist() == [{2: rs.ERR_CTX_LEN, 4: rs.ERR_PARAM, 7: rs.ERR_PARAM, 9: rs.ERR_PARAM}.get(i, 0) for i in range(12)]
    out, status = rs.scattered(blob, ops, want, *oracle_signed(q["keys"], want["packed"]))
    assert np.array_equal(status, want["status"])
    for i, (pset, key, msg, ctx, rnd) in enumerate(q["requests"]):
        at = int(ops[i]["sig_off"])
        hole = out[at:at + rs.SIG_LEN[pset]].tobytes()
        assert hole == (bytes([0xC3]) * rs.SIG_LEN[pset] if i in damage else q["sigs"][i]), i  # a refused op's hole keeps the fill byte
    for pset in rs.SETS:  # nothing of the region the refused ops point into
        for name in ("rnd", "msgs", "ctxs"):
            assert bytes([rs.PATTERN]) * 8 not in want["packed"][pset][name].tobytes()
    assert (out[region:] == rs.PATTERN).all()


def test_refusal_rules_of_the_restatement():
    blob, ops, out_len = rs.seam_case(12, "mod3", seed=1)
    region = blob.size - 6000
    assert all(rs.verdict(op, blob.size, out_len, rs.N_KEYS) == (i % 3, 0) for i, op in enumerate(ops))
    assert int(ops[0]["sig_off"]) == 0 and int(ops[11]["sig_off"]) + rs.SIG_LEN[87] == out_len  # a hole at 0, one flush with out_len
    assert ops[2]["msg_off"] == ops[1]["msg_off"] and ops[4]["rnd_off"] == ops[3]["msg_off"] and ops[4]["flags"] == 1
    assert [int(f) for f in ops["flags"]] == [0 if i % 3 == 2 else 1 for i in range(12)]
    for d, name in enumerate(rs.DEFECTS):
        o = ops.copy()
        rs.make_refused(o, 4, d, blob.size, out_len, region)
        assert [rs.verdict(op, blob.size, out_len, rs.N_KEYS) for op in o] == \
            [(3, rs.DEFECT_STATUS[name]) if i == 4 else (i % 3, 0) for i in range(12)], name
    # a set with no keys is not served: all its ops are refused, whatever their key
    assert [rs.verdict(op, blob.size, out_len, (4, 0, 4))[0] for op in ops] == [3 if i % 3 == 1 else i % 3 for i in range(12)]
    # the order of the rules: the context's length goes before key and ranges, after set, flags and reserved
    o = ops.copy()
    o[0]["ctx_len"], o[0]["key"], o[0]["sig_off"] = 256, 99, 2 ** 64 - 1
    assert rs.verdict(o[0], blob.size, out_len, rs.N_KEYS) == (3, rs.ERR_CTX_LEN)
    o[0]["reserved"] = 1
    assert rs.verdict(o[0], blob.size, out_len, rs.N_KEYS) == (3, rs.ERR_PARAM)
    # without the flag rnd_off is neither followed nor checked
    o = ops.copy()
    o[2]["rnd_off"] = 2 ** 64 - 1
    assert rs.verdict(o[2], blob.size, out_len, rs.N_KEYS) == (2, 0)
    # the empty range at the very end is inside; one byte further is not
    o[0]["msg_off"], o[0]["msg_len"] = blob.size, 0
    assert rs.verdict(o[0], blob.size, out_len, rs.N_KEYS) == (0, 0)
    o[0]["msg_off"] = blob.size + 1
    assert rs.verdict(o[0], blob.size, out_len, rs.N_KEYS) == (3, rs.ERR_PARAM)


def test_the_descriptor_check_and_the_scatter_plan_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "recsign_plan", ["recsign_plan_main.cpp"], "recsign_plan OK")
