"""The wire-record library (include/mldsa_rec.h, fips204_amd/rec/libmldsa_rec.so) without a device: its C ABI, how it is linked against
the core, its scratch formulas, its argument checks, its kernels' resources and sources, the numpy restatement of tests/rec_cases.py
against the oracle, and the copy plan and range check as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rec_cases as rc
from fips204_amd import _lib, _mus_lib, _rec_lib
from fips204_amd.ml_dsa import records_blob
from layer_checks import (PK_SK, ROOT, aligned_buffer, built, clean_build, core_params, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, shared_plan_is_shared_once,
                          sources_clean)
from oracle import oracle as orc

REC_DIR = os.path.join(ROOT, "fips204_amd", "rec")
SOURCES = ["Makefile", "rec.hip", "rec_plan.h", "rec_scan.h", "rec_wave.h", "rec_host.h"]


@pytest.fixture(scope="module")
def rec():
    return built(_rec_lib, REC_DIR)


def test_clean_build_in_a_shadow_tree(rec, tmp_path):
    from fips204_amd import build
    assert build.LAYERS["rec"] == "libmldsa_rec.so" and build.REC_LIB == _rec_lib.LIB_PATH and len(build.LAYERS) == 8
    clean_build("rec", _rec_lib, SOURCES, [os.path.join(build._HERE, d, f) for d, f in build.LAYERS.items()], tmp_path)
    mk = open(os.path.join(REC_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_rec_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(rec, tmp_path):
    declared, text = header_and_exports(
        _rec_lib, rec,
        "int main(void) { mldsa_rec_op o; mldsa_rec_totals t; mldsa_rec_packed p; mldsa_rec_info i;\n"
        "  o.set = MLDSA_65; o.reserved = 0; t.n[MLDSA_REC_CLASS_REFUSED] = 0; p.c[MLDSA_REC_CLASS_87].n = 0; i.scratch_needed = 0;\n"
        "  return sizeof(mldsa_rec_op) == 40 && sizeof(t) == 80 && mldsa_rec_abi_version() == MLDSA_REC_ABI_VERSION && o.set && !t.n[3]\n"
        "    && !p.c[2].n && !i.scratch_needed && mldsa_rec_front_bytes(MLDSA_REC_MAX_OPS) > MLDSA_REC_SCAN_BLOCK ? 0 : 1; }\n",
        r"\b(mldsa_rec_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_rec_abi_version", "mldsa_rec_last_error", "mldsa_rec_plan", "mldsa_rec_plan_bytes", "mldsa_rec_pack",
                        "mldsa_rec_scratch_bytes", "mldsa_rec_scratch_bytes_max", "mldsa_rec_verify", "mldsa_rec_front_bytes"}
    # the Python constants and layouts are the header's
    assert "#define MLDSA_REC_ABI_VERSION 1" in text and rec.mldsa_rec_abi_version() == _rec_lib.ABI_VERSION == 1
    assert "#define MLDSA_REC_MAX_OPS ((size_t)1 << 30)" in text and _rec_lib.MAX_OPS == 1 << 30
    assert f"#define MLDSA_REC_SCAN_BLOCK {_rec_lib.SCAN_BLOCK}" in text and rc.SCAN_BLOCK == _rec_lib.SCAN_BLOCK
    for c, name in enumerate(("44", "65", "87", "REFUSED")):
        assert f"#define MLDSA_REC_CLASS_{name} {c}" in text
    assert (_rec_lib.CLASS_44, _rec_lib.CLASS_65, _rec_lib.CLASS_87, _rec_lib.CLASS_REFUSED) == (0, 1, 2, 3)
    assert _rec_lib.OP_DTYPE.itemsize == 40 and C.sizeof(_rec_lib.RecTotals) == 80 and C.sizeof(_rec_lib.RecInfo) == 56
    assert C.sizeof(_rec_lib.RecPacked) == 3 * 8 * 8
    assert [_rec_lib.OP_DTYPE.fields[f][1] for f in ("pk_off", "sig_off", "msg_off", "ctx_off", "msg_len", "ctx_len", "set", "reserved")] == \
        [0, 8, 16, 24, 32, 36, 38, 39]
    # the lengths the restatement and the plan use are the core's
    params = core_params()
    plan = open(os.path.join(REC_DIR, "rec_plan.h")).read()
    for pset in (44, 65, 87):
        assert (params[pset].pk_len, params[pset].sig_len) == (rc.PK_LEN[pset], rc.SIG_LEN[pset]) and rc.PK_LEN[pset] == PK_SK[pset][0]
        assert str(rc.PK_LEN[pset]) in plan and str(rc.SIG_LEN[pset]) in plan
    # a measurement is stated only where its file exists
    if not os.path.exists(os.path.join(ROOT, "profiles", "rec_bench.jsonl")):
        assert "not measured" in text


def test_layered_on_the_one_core_library(rec):
    layered_on_core(
        _rec_lib.LIB_PATH, needs=("mldsa_verify_pk", "mldsa_ctx_device", "mldsa_last_error"),
        # the verdicts are mldsa_verify_pk's alone: no other op-level or seam call of the core's
        never=("mldsa_verify", "mldsa_verify_cached_a", "mldsa_pk_expand", "mldsa_expand_a", "mldsa_sign", "mldsa_keygen", "mldsa_verify_mu"))
    links_the_core_and_never_builds_it(REC_DIR)
    dyn = subprocess.run(["readelf", "-d", _rec_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy)\.so", dyn)


def test_scratch_sizes_follow_the_documented_formulas(rec):
    ladder = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 65536, 65537, 1 << 30)
    last = 0
    for n in ladder:
        assert rec.mldsa_rec_plan_bytes(n) == rc.plan_bytes(n), n
        assert rec.mldsa_rec_front_bytes(n) == rc.front_bytes(n) >= last, n
        last = rc.front_bytes(n)
    bytes_ladder = (0, 1, 255, 256, 257, 10 ** 6, 1 << 40)
    for n44 in ladder:
        for n65, n87 in ((0, 0), (1, 0), (0, 1), (n44, n44), (65, 257), (1 << 30, 3)):
            for mb in bytes_ladder:
                cb = 255 * min(n44 + n65 + n87, 1000)
                want = rc.arena_bytes(n44, n65, n87, mb, cb)
                assert rec.mldsa_rec_scratch_bytes(n44, n65, n87, mb, cb) == want, (n44, n65, n87, mb)
                n = n44 + n65 + n87
                if n <= 1 << 30:  # the bound covers every mix of n ops, and grows with n
                    bound = rec.mldsa_rec_scratch_bytes_max(n, mb, cb)
                    assert bound == rc.arena_bytes_max(n, mb, cb) and bound >= want, (n44, n65, n87, mb)
                    assert bound >= rc.arena_bytes(0, 0, n, mb, cb) and bound >= rc.arena_bytes(n, 0, 0, mb, cb)
                    assert bound < rc.arena_bytes(0, 0, n, mb, cb) + 4096  # tight: an all-87 mix is within 4 KiB of it
    # an even three-way mix of 65 536 ops with 32-byte messages: about what the key and signature bytes take
    assert rec.mldsa_rec_scratch_bytes(21846, 21845, 21845, 32 * 65536, 0) < 65536 * 5500  # (1952 + 3452 on average, + 32 + 17)
    # past MLDSA_REC_MAX_OPS, or a size that does not fit: 0
    big = (1 << 30) + 1
    for args in ((big, 0, 0, 0, 0), (0, big, 0, 0, 0), (0, 0, big, 0, 0), (0, 0, 2 ** 63, 0, 0), (1, 1, 1, 2 ** 63, 0), (1, 1, 1, 0, 2 ** 64 - 1)):
        assert rec.mldsa_rec_scratch_bytes(*args) == 0, args
    for args in ((big, 0, 0), (2 ** 64 - 1, 0, 0), (1, 2 ** 63, 0), (1, 0, 2 ** 64 - 1)):
        assert rec.mldsa_rec_scratch_bytes_max(*args) == 0, args
    for n in (big, 2 ** 63, 2 ** 64 - 1):
        assert rec.mldsa_rec_plan_bytes(n) == 0 and rec.mldsa_rec_front_bytes(n) == 0


def test_argument_errors_never_abort(rec):
    null = None
    buf, p, odd = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    big = 1 << 50
    err = rec.mldsa_rec_last_error
    tot = _rec_lib.RecTotals()
    tot.n[:] = [2, 1, 1, 0]
    out, info = _rec_lib.RecPacked(), _rec_lib.RecInfo()

    def plan(ctx=null, blob=p, blob_len=4096, ops=p, n=4, cs=p, totals=p, pl=p, pb=big, stream=null):
        return rec.mldsa_rec_plan(ctx, blob, blob_len, ops, n, cs, totals, pl, pb, stream)

    def pack(ctx=null, blob=p, blob_len=4096, ops=p, n=4, cs=p, pl=p, pb=big, totals=C.byref(tot), arena=p, ab=big, packed=C.byref(out), stream=null):
        return rec.mldsa_rec_pack(ctx, blob, blob_len, ops, n, cs, pl, pb, totals, arena, ab, packed, stream)

    def verify(ctx=null, mode=0, blob=p, blob_len=4096, ops=p, n=4, ok=p, scratch=p, sb=big, inf=C.byref(info), stream=null):
        return rec.mldsa_rec_verify(ctx, mode, blob, blob_len, ops, n, ok, scratch, sb, inf, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (plan, pack, verify):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    # a fake non-NULL context must still be refused before it is touched
    fake = p
    for call in (plan, pack, verify):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, ops=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, ops=odd4) == _lib.ERR_PARAM and b"ops must be 8-byte aligned" in err()
        assert call(ctx=fake, n=_rec_lib.MAX_OPS + 1) == _lib.ERR_PARAM and b"MLDSA_REC_MAX_OPS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_REC_MAX_OPS" in err()
    for kw in (dict(cs=null), dict(totals=null)):
        assert plan(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL pointer" in err(), kw
    assert plan(ctx=fake, cs=C.c_void_p(p.value + 2)) == _lib.ERR_PARAM and b"aligned" in err()
    assert plan(ctx=fake, totals=odd4) == _lib.ERR_PARAM and b"aligned" in err()
    need = rec.mldsa_rec_plan_bytes(4)
    for kw in (dict(pl=null), dict(pl=odd), dict(pb=need - 1), dict(pb=0)):
        assert plan(ctx=fake, **kw) == _lib.ERR_PARAM and b"plan is NULL" in err(), kw
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"plan is NULL" in err(), kw
    for kw in (dict(cs=null), dict(totals=null), dict(packed=null)):
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"NULL pointer" in err(), kw
    assert pack(ctx=fake, n=5) == _lib.ERR_PARAM and b"totals do not describe" in err()  # 2 + 1 + 1 + 0 ops
    for kw in (dict(arena=null), dict(arena=odd)):
        assert pack(ctx=fake, **kw) == _lib.ERR_PARAM and b"arena is NULL or not 256-byte aligned" in err(), kw
    assert pack(ctx=fake, ab=rec.mldsa_rec_scratch_bytes(2, 1, 1, 0, 0) - 1) == _lib.ERR_NOMEM and b"arena smaller" in err()
    for mode in (-1, 3, 99):  # refused before anything is launched, as the core does
        assert verify(ctx=fake, mode=mode) == _lib.ERR_PARAM and b"unknown mode" in err(), mode
    assert verify(ctx=fake, ok=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    for kw in (dict(scratch=null), dict(scratch=odd), dict(scratch=C.c_void_p(p.value + 128)), dict(sb=rec.mldsa_rec_front_bytes(4) - 1), dict(sb=0)):
        assert verify(ctx=fake, **kw) == _lib.ERR_PARAM and b"scratch is NULL" in err(), kw
    # a NULL blob is an empty blob's: only with blob_len > 0 is it an error (the checks go on to the next one)
    assert plan(ctx=fake, blob=null, blob_len=0, cs=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    # empty calls succeed without a context, and touch nothing
    assert plan(n=0, blob=null, ops=null, cs=null, totals=null, pl=null, pb=0) == _lib.OK
    out.c[1].n = 7
    assert pack(n=0, blob=null, ops=null, cs=null, pl=null, pb=0, totals=null, arena=null, ab=0) == _lib.OK and out.c[1].n == 0
    assert verify(n=0, blob=null, ops=null, ok=null, scratch=null, sb=0, inf=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(rec):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert rec.mldsa_rec_verify(p, 7, p, 16, p, 4, p, p, big, null, null) == _lib.ERR_PARAM
    mine = rec.mldsa_rec_last_error()
    assert mine == b"mldsa_rec_verify: unknown mode"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert rec.mldsa_rec_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _rec_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "copy_plan", "k_pack"):
        assert word not in exported, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(rec):
    kernels = kernel_resources(REC_DIR)
    for stem in ("k_classify", "k_offsets", "k_apply", "k_pack", "k_scatter"):
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == 5
    # sources_clean reads the whole directory: rec_scan.h and rec_host.h, which libmldsa_recsign.so shares, are among its files
    read = dict(sources_clean(REC_DIR, ["../../include/mldsa_rec.h", "../_rec_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]))
    src, plan, scan, wave, host = read["rec.hip"], read["rec_plan.h"], read["rec_scan.h"], read["rec_wave.h"], read["rec_host.h"]
    for h in ("../layer/layer_host.h", "../../include/mldsa_rec.h", "rec_plan.h", "rec_scan.h", "rec_host.h"):
        assert f'#include "{h}"' in src, h
    # the kernel boundaries do the ordering: no atomics, no flag another workgroup waits for, no spin loop; the scaffold is shared, not copied
    for word in ("atomic", "__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "struct DeviceScope",
                 "thread_local", "int fail("):
        assert word not in src + plan + scan + wave + host, word
    shared_plan_is_shared_once(src, scan, wave, host, open(os.path.join(REC_DIR, "Makefile")).read(), "rec_scan.h", "rec_wave.h", "rec_host.h")
    no_new_dynamic_symbol(_rec_lib.LIB_PATH, "mldsa_rec_")
    # the plan has no HIP in it, and the kernel keeps no second copy of its arithmetic: it calls the plan's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan
    own_code = re.sub(r"//[^\n]*", "", src)
    kernel_code = own_code + re.sub(r"//[^\n]*", "", scan + wave)
    for call in ("copy_plan(", "chunk_src(", "funnel16(", "classify(", "in_range("):
        assert call in kernel_code and "constexpr" in plan, call
    for name in ("copy_plan", "chunk_src", "funnel16", "funnel_at", "in_range", "sig_len", "class_of_set", "up256"):
        assert not re.search(r"constexpr[^;{]*\b%s\s*\(" % name, kernel_code + re.sub(r"//[^\n]*", "", host)), name  # used, not restated
    assert "classify(" in own_code  # the verdict function is called from the library's own file
    host_code = own_code + re.sub(r"//[^\n]*", "", host)
    assert own_code.count("mldsa_verify_pk(") == 1 and host_code.count("hipStreamSynchronize(") == 1


# ---- the restatement against the oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signed_records():
    """twelve valid records, four per parameter set, from the oracle: (pset, pk, message, sig, ctx)"""
    recs = []
    for i in range(12):
        pset = rc.SETS[i % 3]
        pk, sk = orc.keygen_from_seed(pset, bytes([i + 1]) * 32)
        msg, ctx = rc._bytes(b"cpu-msg", i, rc.MSG_LENS[i % len(rc.MSG_LENS)]), rc._bytes(b"cpu-ctx", i, (0, 1, 255)[i % 3 if i < 9 else 0])
        sig = orc.sign_internal(pset, sk, msg, bytes([0x80 + i]) * 32, ctx=ctx, mode=orc.MODE_PURE)
        recs.append((pset, orc.pk_into_bytes(pset, pk), msg, sig, ctx))
    return recs


def _oracle_verdicts(packed):
    out = {}
    for pset in rc.SETS:
        out[pset] = [orc.verify_internal(pset, orc.pk_try_from_bytes(pset, pk), msg, sig, ctx=ctx, mode=orc.MODE_PURE)
                     for pk, msg, sig, ctx in rc.records_of(packed[pset])]
    return out


def test_restated_packing_of_valid_records_verifies_under_the_oracle(signed_records):
    for shift, gaps in ((0, 0), (1, list(range(16))), (3, [5, 0, 11])):
        blob, ops = records_blob(signed_records, pad=gaps, front=shift)
        want = rc.expected(blob, ops)
        assert want["totals"][:4] == [4, 4, 4, 0]
        assert [int(x) >> 30 for x in want["class_slot"]] == [0, 1, 2] * 4 and [int(x) & 0x3FFFFFFF for x in want["class_slot"]] == \
            [i // 3 for i in range(12)]
        assert all(all(v) and len(v) == 4 for v in _oracle_verdicts(want["packed"]).values())
        for c, pset in enumerate(rc.SETS):  # slots follow input order
            assert [r[1] for r in rc.records_of(want["packed"][pset])] == [signed_records[i][2] for i in range(c, 12, 3)]


def test_restated_packing_of_damaged_records_does_not_verify(signed_records):
    blob, ops = records_blob(signed_records, pad=list(range(16)), front=2)
    blob = np.concatenate([blob, np.full(6000, rc.PATTERN, dtype=np.uint8)])
    region = blob.size - 6000
    bad = blob.copy()
    bad[int(ops[0]["sig_off"]) + 40] ^= 1        # op 0: a damaged signature
    bad[int(ops[1]["msg_off"])] ^= 0x10          # op 1: a damaged message (1 byte long)
    bad[int(ops[2]["pk_off"]) + 100] ^= 4        # op 2: a damaged key
    ops = ops.copy()
    ops[4]["ctx_len"] = 0                        # op 4: a wrong context (its own is 1 byte)
    rc.make_refused(ops, 7, "sig_off_top", blob.size, region)
    rc.make_refused(ops, 9, "ctx_len_256", blob.size, region)
    want = rc.expected(bad, ops)
    assert want["totals"][:4] == [3, 3, 4, 2]    # ops 7 (65) and 9 (44) are refused
    got = _oracle_verdicts(want["packed"])
    assert got[44] == [False, True, True] and got[65] == [False, False, True] and got[87] == [False, True, True, True]
    for pset in rc.SETS:  # nothing of the region the refused ops point into
        for name in ("pk", "sigs", "msgs", "ctxs"):
            assert bytes([rc.PATTERN]) * 8 not in want["packed"][pset][name].tobytes()


def test_refusal_rules_of_the_restatement():
    blob, ops = rc.seam_case(12, "mod3", seed=1)
    region = blob.size - 6000
    assert all(rc.class_of(op, blob.size) == i % 3 for i, op in enumerate(ops))
    for d, name in enumerate(rc.DEFECTS):
        o = ops.copy()
        rc.make_refused(o, 4, d, blob.size, region)
        assert [rc.class_of(op, blob.size) for op in o] == [3 if i == 4 else i % 3 for i in range(12)], name
    # the empty range at the very end is inside; one byte further is not
    o = ops.copy()
    o[0]["msg_off"], o[0]["msg_len"] = blob.size, 0
    assert rc.class_of(o[0], blob.size) == 0
    o[0]["msg_off"] = blob.size + 1
    assert rc.class_of(o[0], blob.size) == 3
    # shared ranges make the message bytes exceed what the blob holds of messages
    many = np.repeat(ops[1:2], 50)
    assert rc.expected(blob, many)["totals"][5] == 50 * int(ops[1]["msg_len"])


def test_the_copy_plan_and_range_check_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "rec_plan", ["rec_plan_main.cpp"], "rec_plan OK")
