"""The certificate-issuing library (include/mldsa_x509sign.h, fips204_amd/x509sign/libmldsa_x509sign.so) without a device: its C ABI, how
it is linked against the core, its host helpers and argument checks, its kernels' resources and sources, the restatement of
tests/x509sign_cases.py against itself, the verifying side's restatement, openssl and the oracle, and the rules, the walk and the frame
as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import x509_cases as xc
import x509sign_cases as xs
from fips204_amd import _lib, _mus_lib, _recsign_lib, _x509_lib, _x509sign_lib
from layer_checks import (ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, sources_clean)
from oracle import oracle as orc

X509SIGN_DIR = os.path.join(ROOT, "fips204_amd", "x509sign")
SOURCES = ["Makefile", "x509sign.hip", "x509sign_plan.h"]
KERNELS = ("k_x509sign_check", "k_x509sign_offsets", "k_x509sign_apply", "k_x509sign_frame")


@pytest.fixture(scope="module")
def lib():
    return built(_x509sign_lib, X509SIGN_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(lib, tmp_path):
    from fips204_amd import build
    assert build.ISSUE_LAYERS == {"x509sign": "libmldsa_x509sign.so"}
    assert build.X509SIGN_LIB == _x509sign_lib.LIB_PATH and build.X509SIGN_DIR == X509SIGN_DIR
    # the three older dicts as they were
    assert len(build.LAYERS) == 8 and build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"} and build.PARSE_LAYERS == {"x509": "libmldsa_x509.so"}
    # x509sign_plan.h includes ../x509/x509_plan.h and ../rec/rec_plan.h: the shadow links both directories
    (tmp_path / "fips204_amd").mkdir()
    os.symlink(build.REC_DIR, tmp_path / "fips204_amd" / "rec")
    os.symlink(build.X509_DIR, tmp_path / "fips204_amd" / "x509")
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS, **build.ISSUE_LAYERS}.items()]
    assert libs[-1] == _x509sign_lib.LIB_PATH  # built last, behind the parse layers
    clean_build("x509sign", _x509sign_lib, SOURCES, libs, tmp_path)
    mk = open(os.path.join(X509SIGN_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../x509/x509_plan.h", "../x509/x509_dev.h", "../rec/rec_plan.h", "../rec/rec_wave.h", "../rec/rec_place.h", "x509sign_plan.h"):
        assert h in mk, h  # a change of a shared header rebuilds this library
    assert not re.search(r"-lmldsa_(rec|recsign|x509)\b", mk)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_x509sign_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(lib, tmp_path):
    declared, text = header_and_exports(
        _x509sign_lib, lib,
        "int main(void) { mldsa_x509sign_req r; mldsa_x509sign_totals t; mldsa_x509_cert c; mldsa_recsign_op o;\n"
        "  r.flags = MLDSA_X509SIGN_RND; r.set = MLDSA_87; t.out_bytes = 0; c.issuer = MLDSA_X509_NO_ISSUER; o.reserved = 0;\n"
        "  return sizeof(r) == 32 && sizeof(t) == 24 && sizeof(c) == 16 && sizeof(o) == 48 && r.flags == 1 && !t.out_bytes && !o.reserved\n"
        "    && mldsa_x509sign_abi_version() == MLDSA_X509SIGN_ABI_VERSION && MLDSA_X509SIGN_SPACE == 11 && c.issuer > MLDSA_X509SIGN_MAX_CERTS ? 0 : 1; }\n",
        r"\b(mldsa_x509sign_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_x509sign_abi_version", "mldsa_x509sign_last_error", "mldsa_x509sign_cert_len", "mldsa_x509sign_out_bytes_max",
                        "mldsa_x509sign_plan_bytes", "mldsa_x509sign_plan", "mldsa_x509sign_frame", "mldsa_x509sign_issue_ops"}
    assert '#include "mldsa_recsign.h"' in text and '#include "mldsa_x509.h"' in text  # for the two types only
    assert "#define MLDSA_X509SIGN_ABI_VERSION 1" in text and lib.mldsa_x509sign_abi_version() == _x509sign_lib.ABI_VERSION == 1
    assert "#define MLDSA_X509SIGN_MAX_CERTS (1u << 30)" in text and _x509sign_lib.MAX_CERTS == 1 << 30
    assert "#define MLDSA_X509SIGN_SCAN_BLOCK 256" in text and _x509sign_lib.SCAN_BLOCK == 256
    assert "#define MLDSA_X509SIGN_RND 1" in text and _x509sign_lib.FLAG_RND == xs.FLAG_RND == _recsign_lib.FLAG_RND == 1
    for name, code in (("ENTRY", 8), ("KEY", 9), ("LONG", 10), ("SPACE", 11)):
        assert re.search(r"#define MLDSA_X509SIGN_%s %d\b" % (name, code), text), name
        assert getattr(_x509sign_lib, name) == getattr(xs, name) == code
    # codes 1 ... 3 are the certificate library's, the new ones are disjoint from its 4 ... 7
    assert (_x509sign_lib.OK, _x509sign_lib.RANGE, _x509sign_lib.DER, _x509sign_lib.ALG) == (_x509_lib.OK, _x509_lib.RANGE, _x509_lib.DER, _x509_lib.ALG)
    assert not {8, 9, 10, 11} & set(range(8))
    # the layouts
    assert _x509sign_lib.REQ_DTYPE.itemsize == 32 and _x509sign_lib.TOTALS_DTYPE.itemsize == 24
    names = ("off", "rnd_off", "len", "key", "issuer", "set", "flags", "reserved")
    assert [_x509sign_lib.REQ_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 20, 24, 28, 29, 30]
    assert [_x509sign_lib.TOTALS_DTYPE.fields[f][1] for f in ("accepted", "refused", "out_bytes")] == [0, 8, 16]
    for word, at in (("uint64_t off;", 0), ("uint64_t rnd_off;", 1), ("uint32_t len;", 2), ("uint32_t key;", 3), ("uint32_t issuer;", 4),
                     ("uint8_t set;", 5), ("uint8_t flags;", 6), ("uint16_t reserved;", 7)):
        assert word in text, word
    order = [text.index(w) for w in ("uint64_t off;", "uint64_t rnd_off;", "uint32_t len;", "uint32_t key;", "uint32_t issuer;", "uint8_t set;",
                                     "uint8_t flags;", "uint16_t reserved;")]
    assert order == sorted(order)
    # what is out of scope is said, and a measurement is stated only where its file exists
    for word in ("NOT IN SCOPE", "validity dates", "extensions", "name chaining", "PEM", "CSRs", "CRLs", "HashML-DSA", "external-mu", "batcher",
                 "Rust", "the hole holds zeros", "63097 / 62208 / 60890"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "x509sign_bench.jsonl")):
        assert "not measured" in text


def test_layered_on_the_one_core_library(lib):
    layered_on_core(_x509sign_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_sign", "mldsa_verify", "mldsa_verify_pk", "mldsa_keygen", "mldsa_memset", "mldsa_rec_verify", "mldsa_rec_plan",
                           "mldsa_rec_pack", "mldsa_recsign_sign", "mldsa_recsign_plan", "mldsa_recsign_pack", "mldsa_recsign_scatter",
                           "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops"))
    links_the_core_and_never_builds_it(X509SIGN_DIR)
    dyn = subprocess.run(["readelf", "-d", _x509sign_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign|x509)\.so", dyn)
    no_new_dynamic_symbol(_x509sign_lib.LIB_PATH, "mldsa_x509sign_")


def test_host_helpers_against_the_restatement(lib):
    for pset in xs.SETS:
        for n in (0, 1, 2, 1000, xs.MAX_TBS[pset] - 1, xs.MAX_TBS[pset], xs.MAX_TBS[pset] + 1, 65536, 2 ** 32, 2 ** 64 - 1):
            assert lib.mldsa_x509sign_cert_len(pset, n) == xs.cert_len(pset, n), (pset, n)
        assert lib.mldsa_x509sign_cert_len(pset, xs.MAX_TBS[pset]) == 65539 and xs.MAX_TBS[pset] == {44: 63097, 65: 62208, 87: 60890}[pset]
    for bad in (0, 43, 66, -1, 128, 2 ** 31 - 1):
        assert lib.mldsa_x509sign_cert_len(bad, 10) == 0
    for n, b in ((0, 0), (1, 0), (1, 1), (65536, 10 ** 8), (1 << 30, 2 ** 40)):
        assert lib.mldsa_x509sign_out_bytes_max(n, b) == xs.out_bytes_max(n, b) == b + n * 4649
    # past the cap and on overflow: 0
    assert lib.mldsa_x509sign_out_bytes_max((1 << 30) + 1, 0) == 0 and lib.mldsa_x509sign_out_bytes_max(2 ** 64 - 1, 0) == 0
    assert lib.mldsa_x509sign_out_bytes_max(1, 2 ** 64 - 1) == 0 and lib.mldsa_x509sign_out_bytes_max(1, 2 ** 64 - 4649) == 0
    assert lib.mldsa_x509sign_out_bytes_max(1, 2 ** 64 - 4650) == 2 ** 64 - 1
    # the plan's working memory: the header's formula, never decreasing, 0 past the cap (layer_checks.scratch_sweep's ladder)
    last = 0
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 192, 255, 256, 257, 264, 1000, 65536, 65537, 1 << 30):
        got = lib.mldsa_x509sign_plan_bytes(n)
        assert got == xs.plan_bytes(n) and got >= last and got % 256 == 0, n
        last = got
    for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
        assert lib.mldsa_x509sign_plan_bytes(n) == 0
    text = open(_x509sign_lib.HEADER_PATH).read()
    assert "R(16 B) + R(4 n)" in text and "tbs_bytes + n (22 + 4627)" in text


def test_argument_errors_never_abort(lib):
    null = None
    buf, p, _ = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    other = (C.c_uint8 * 8192)()
    q = C.c_void_p((C.addressof(other) + 255) // 256 * 256)  # a second buffer: apart from the first
    nk = (C.c_size_t * 3)(4, 4, 4)
    err = lib.mldsa_x509sign_last_error

    def plan(ctx=null, blob=p, blob_len=1024, reqs=p, n=4, n_keys=nk, out_len=4096, out_certs=p, ops=p, status=p, totals=p, mem=p, mem_bytes=3840,
             stream=null):
        return lib.mldsa_x509sign_plan(ctx, blob, blob_len, reqs, n, n_keys, out_len, out_certs, ops, status, totals, mem, mem_bytes, stream)

    def frame(ctx=null, blob=p, blob_len=1024, reqs=p, n=4, out=q, out_len=4096, out_certs=p, status=p, stream=null):
        return lib.mldsa_x509sign_frame(ctx, blob, blob_len, reqs, n, out, out_len, out_certs, status, stream)

    def issue(ctx=null, blob=p, blob_len=1024, reqs=p, n=4, n_keys=nk, out=q, out_len=4096, out_certs=p, ops=p, status=p, totals=p, mem=p,
              mem_bytes=3840, stream=null):
        return lib.mldsa_x509sign_issue_ops(ctx, blob, blob_len, reqs, n, n_keys, out, out_len, out_certs, ops, status, totals, mem, mem_bytes, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (plan, frame, issue):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    fake = p  # a fake non-NULL context must still be refused before it is touched
    for call in (plan, frame, issue):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, reqs=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, out_certs=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, status=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, reqs=odd4) == _lib.ERR_PARAM and b"reqs must be 8-byte aligned" in err()
        assert call(ctx=fake, out_certs=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n=_x509sign_lib.MAX_CERTS + 1) == _lib.ERR_PARAM and b"MLDSA_X509SIGN_MAX_CERTS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_X509SIGN_MAX_CERTS" in err()
    for call in (plan, issue):
        for name in ("n_keys", "ops", "totals"):
            assert call(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
        assert call(ctx=fake, ops=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, totals=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n_keys=(C.c_size_t * 3)(4, 2 ** 32, 4)) == _lib.ERR_PARAM and b"n_keys above UINT32_MAX" in err()
        assert call(ctx=fake, mem=null) == _lib.ERR_PARAM and b"mldsa_x509sign_plan_bytes" in err()
        assert call(ctx=fake, mem=C.c_void_p(p.value + 128)) == _lib.ERR_PARAM and b"256-byte aligned" in err()
        assert call(ctx=fake, mem_bytes=lib.mldsa_x509sign_plan_bytes(4) - 1) == _lib.ERR_PARAM and b"smaller than" in err()
    # out must not overlap the blob: decided from the two pointer ranges
    for call in (frame, issue):
        assert call(ctx=fake, out=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        for out, out_len in ((p, 4096), (C.c_void_p(p.value + 1023), 16), (C.c_void_p(p.value - 15), 16), (C.c_void_p(p.value - 100), 4096)):
            assert call(ctx=fake, out=out, out_len=out_len) == _lib.ERR_PARAM and b": out overlaps the blob" in err(), (out, out_len)
    # flush against the blob on either side is apart: the next check is reached (the fake context is refused by the core, not touched)
    assert frame(ctx=null, out=C.c_void_p(p.value + 1024), out_len=16) == _lib.ERR_PARAM and b"NULL context" in err()
    # a NULL blob is an empty blob's: only with blob_len > 0 is it an error (the checks go on to the next one)
    assert frame(ctx=fake, blob=null, blob_len=0, out=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    # empty calls succeed without a context, and touch nothing
    assert plan(n=0, blob=null, reqs=null, n_keys=None, out_certs=null, ops=null, status=null, totals=null, mem=null, mem_bytes=0) == _lib.OK
    assert frame(n=0, blob=null, reqs=null, out=null, out_certs=null, status=null) == _lib.OK
    assert issue(n=0, blob=null, reqs=null, n_keys=None, out=null, out_certs=null, ops=null, status=null, totals=null, mem=null, mem_bytes=0) == _lib.OK
    del buf, other


def test_the_error_slot_is_this_librarys_own(lib):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert lib.mldsa_x509sign_frame(p, p, 64, p, 4, p, 64, p, p, null) == _lib.ERR_PARAM
    mine = lib.mldsa_x509sign_last_error()
    assert mine == b"mldsa_x509sign_frame: out overlaps the blob"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert lib.mldsa_x509sign_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _x509sign_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "walk_tbs", "k_x509sign", "copy_field"):
        assert word not in exported, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(lib):
    kernels = kernel_resources(X509SIGN_DIR)
    for stem in KERNELS:
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == len(KERNELS)  # rec_wave.h and rec_place.h bring no kernel along: nothing is compiled that is not launched
    assert not any("k_classify" in nm or "k_apply" in nm for nm in kernels)
    read = dict(sources_clean(X509SIGN_DIR, ["../../include/mldsa_x509sign.h", "../_x509sign_lib.py", "../layer/layer_host.h", "../rec/rec_wave.h",
                                             "../rec/rec_place.h"]))
    src, plan, place = read["x509sign.hip"], read["x509sign_plan.h"], read["../rec/rec_place.h"]
    certificate_helpers_shared_once("x509sign")
    for h in ("../layer/layer_host.h", "../rec/rec_place.h", "../x509/x509_dev.h", "../../include/mldsa_x509sign.h", "x509sign_plan.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../rec/rec_plan.h"' in plan and '#include "../x509/x509_plan.h"' in plan
    # the kernel boundary does the ordering: no atomics, no flag another workgroup waits for, no host wait; the scaffold is shared, not copied
    for word in ("atomic", "__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "hipStreamSynchronize",
                 "hipMemcpy", "hipMalloc", "hipMemset", "struct DeviceScope", "thread_local", "int fail(", "mldsa_recsign_sign(", "mldsa_sign(",
                 "k_classify", "k_apply<", "launch_plan<"):
        assert word not in src and word not in plan, word
    # the plan has no HIP in it, and the kernels keep no second copy of its rules, of the TLV reader or of the wave copy
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan and "constexpr" in plan
    kernel_code = re.sub(r"//[^\n]*", "", src + place)  # (the scan is rec_place.h's, which libmldsa_csr.so shares)
    for call in ("entry_status(", "walk_tbs(", "cert_len(", "header_byte(", "trailer_byte(", "in_range(", "copy_field(", "wave_inclusive("):
        assert call in kernel_code, call
    for word in ("0x30", "0x82", "0x0B", "0xA0", "65535", "0x11"):  # the rules and the frame live in the plan alone
        assert word in plan and word not in kernel_code, word
    for word in ("Tlv read_tlv", "uint32_t oid_set", "uint64_t wave_inclusive", "void copy_field", "CopyPlan copy_plan"):  # included, not copied
        assert word not in src and word not in plan, word
    assert src.count("__shared__") == 2  # the per-wave partial sums of the check and the apply


# ---- the restatement against itself, the verifying side, openssl and the oracle ----------------------------------------------------
def one(pset, tbs, length=None, **fields):
    """status of one request, after checking the rows of the restatement against each other"""
    blob, reqs = xs.lay_out([(pset, 0, tbs, len(tbs) if length is None else length, None, 0)], pad=5)
    for k, v in fields.items():
        reqs[0][k] = v
    want = xs.expected(blob, reqs, xs.N_KEYS, 10 ** 6)
    return int(want["status"][0]), want, blob, reqs


def check_contract(out, want, reqs):
    """every accepted certificate of `out` (signatures in the holes) is OK to the verifying side's walk, at the contract's offsets"""
    raw = out.tobytes()
    for i in want["frames"]:
        c, op = want["out_certs"][i], want["ops"][i]
        der = raw[int(c["off"]):int(c["off"]) + int(c["len"])]
        w = xc.walk(der)
        assert w["status"] == xc.OK and w["sig_set"] == int(reqs[i]["set"]), i
        assert (w["tbs_off"], w["tbs_len"]) == (4, int(reqs[i]["len"])) and int(c["off"]) + w["sig_off"] == int(op["sig_off"]), i
        assert w["sig_off"] + xs.SIG_LEN[w["sig_set"]] == len(der)


@pytest.mark.parametrize("pset,cert_total", [(44, 3868), (65, 5397), (87, 7355)])
def test_valid_requests_give_the_pinned_rows(pset, cert_total):
    tbs = xc.tbs(pset, pset, b"root", b"leaf", xc._bytes(b"pk", 0, xc.PK_LEN[pset]))
    st, want, blob, reqs = one(pset, tbs)
    assert st == xs.OK and want["totals"] == (1, 0, cert_total)  # (the totals test_x509_cpu.py pins for the same certificate)
    c, op = want["out_certs"][0], want["ops"][0]
    assert (int(c["off"]), int(c["len"]), int(c["issuer"])) == (0, cert_total, 0) and cert_total == len(tbs) + 22 + xs.SIG_LEN[pset]
    assert (int(op["msg_off"]), int(op["msg_len"]), int(op["sig_off"])) == (5, len(tbs), len(tbs) + 22)
    assert (int(op["ctx_off"]), int(op["ctx_len"]), int(op["rnd_off"]), int(op["flags"]), int(op["key"]), int(op["set"]), int(op["reserved"])) == \
        (0, 0, 0, 0, 0, pset, 0)
    frame = want["frames"][0]
    assert frame[:4] == bytes([0x30, 0x82]) + (cert_total - 4).to_bytes(2, "big") and frame[4:4 + len(tbs)] == tbs
    assert frame[4 + len(tbs):len(tbs) + 22] == bytes.fromhex("300b06096086480165030403") + bytes([0x11 + xs.SETS.index(pset)]) + \
        b"\x03\x82" + (xs.SIG_LEN[pset] + 1).to_bytes(2, "big") + b"\x00"
    assert xs.SIG_LEN[pset] + 1 == {44: 0x0975, 65: 0x0CEE, 87: 0x1214}[pset]
    out = xs.framed(np.full(cert_total + 3, 0x77, dtype=np.uint8), want)
    assert (out[len(tbs) + 22:] == 0x77).all()  # the hole and what lies behind the certificate are untouched
    check_contract(xs.framed(np.zeros(cert_total, dtype=np.uint8), want, {0: xc._bytes(b"sig", 0, xs.SIG_LEN[pset])}), want, reqs)


def test_every_defect_gives_its_documented_status_and_neighbours_are_untouched():
    blob, reqs, at = xs.defect_batch()
    want = xs.expected(blob, reqs, xs.N_KEYS, 10 ** 7)
    assert set(at) == set(xs.DEFECTS) and len(reqs) == 3 * len(xs.DEFECTS)
    for name, i in at.items():
        assert want["status"][i] == xs.DEFECTS[name], name
        assert want["status"][i - 1] == want["status"][i + 1] == 0, name
        assert want["ops"][i].tobytes() == bytes(48) and want["out_certs"][i].tobytes() == bytes(12) + b"\xff" * 4 and i not in want["frames"], name
        # a refused certificate takes no room
        assert int(want["out_certs"][i + 1]["off"]) == int(want["out_certs"][i - 1]["off"]) + int(want["out_certs"][i - 1]["len"]), name
    assert want["totals"] == (2 * len(xs.DEFECTS), len(xs.DEFECTS), sum(len(f) for f in want["frames"].values()))
    # a set that is not served: every request of it is KEY
    served = (4, 0, 4)
    st = xs.expected(blob, reqs, served, 10 ** 7)["status"]
    assert all(s == xs.KEY for s, r in zip(st, reqs) if int(r["set"]) == 65 and int(r["flags"]) < 2 and int(r["reserved"]) == 0)
    assert (st == xs.KEY).sum() >= len(reqs) // 3 - 3
    # one byte short with the missing byte in the blob behind it
    i = at["len_one_short"]
    full = blob[int(reqs[i]["off"]):int(reqs[i]["off"]) + int(reqs[i]["len"]) + 1].tobytes()
    assert xs.walk_tbs(full, int(reqs[i]["set"])) == xs.OK and want["status"][i] == xs.DER


def test_precedence_the_earlier_rule_is_reported():
    tbs = xs.good_tbs(44, b"prec", 0)
    bad_der, n_der = xs.byte_defect(tbs, 44, "wrong_tag_validity")
    bad_alg, n_alg = xs.byte_defect(tbs, 44, "inner_oid_other_set")
    both, n_both = xs.byte_defect(bad_alg, 44, "wrong_tag_subject")
    long_tbs = xs.tbs_of_len(44, xs.MAX_TBS[44] + 1)
    assert one(44, tbs)[0] == xs.OK and one(44, bad_der)[0] == xs.DER and one(44, bad_alg)[0] == xs.ALG
    assert one(44, both)[0] == xs.DER                                               # DER before ALG
    assert one(44, bad_der, set=43)[0] == xs.ENTRY and one(44, tbs, set=65)[0] == xs.ALG  # the entry's set decides
    assert one(44, tbs, set=43, key=9, len=1)[0] == xs.ENTRY                         # ENTRY before KEY and RANGE
    assert one(44, tbs, key=4, len=1)[0] == xs.KEY                                   # KEY before RANGE
    assert one(44, long_tbs, off=2 ** 63)[0] == xs.RANGE                             # RANGE before LONG
    assert one(44, long_tbs, flags=1, rnd_off=2 ** 64 - 1)[0] == xs.RANGE            # ... the rnd range too
    assert one(44, long_tbs)[0] == xs.LONG and one(44, bytes(len(long_tbs)))[0] == xs.LONG  # LONG before DER
    assert one(44, bad_alg, flags=0, rnd_off=2 ** 64 - 1)[0] == xs.ALG               # without the flag rnd_off is not looked at
    # SPACE last: a defective TBS in too small a buffer keeps its own status
    blob, reqs = xs.lay_out([(44, 0, t, n, None, 0) for t, n in ((tbs, len(tbs)), (bad_der, n_der), (bad_alg, n_alg), (tbs, len(tbs)))])
    assert xs.expected(blob, reqs, xs.N_KEYS, 100)["status"].tolist() == [xs.SPACE, xs.DER, xs.ALG, xs.SPACE]


def test_length_edges_space_and_alignment_of_the_restatement():
    blob, reqs, status = xs.edge_batch()
    want = xs.expected(blob, reqs, xs.N_KEYS, 10 ** 7)
    assert want["status"].tolist() == status and status.count(xs.LONG) == 3
    assert sorted(int(c["len"]) for c in want["out_certs"])[-3:] == [65539] * 3
    assert [f[:4] for f in want["frames"].values() if len(f) == 65539] == [bytes.fromhex("3082ffff")] * 3
    # SPACE: the need, one byte less, and a value inside the middle certificate
    blob, reqs = xs.seam_case(65, "tenth_defect", seed=3)
    free = xs.expected(blob, reqs, xs.N_KEYS, 2 ** 62)
    need = free["totals"][2]
    assert xs.expected(blob, reqs, xs.N_KEYS, need)["status"].tolist() == free["status"].tolist()
    last = max(free["frames"])
    short = xs.expected(blob, reqs, xs.N_KEYS, need - 1)
    assert [i for i in range(65) if short["status"][i] != free["status"][i]] == [last] and short["status"][last] == xs.SPACE
    assert short["totals"] == (free["totals"][0] - 1, free["totals"][1] + 1, need)
    mid = sorted(free["frames"])[len(free["frames"]) // 2]
    cut = xs.expected(blob, reqs, xs.N_KEYS, int(free["out_certs"][mid]["off"]) + 100)
    assert all((cut["status"][i] == xs.SPACE) == (i >= mid) for i in free["frames"]) and cut["totals"][2] == need
    assert cut["totals"][0] == sum(1 for i in free["frames"] if i < mid)
    # alignment: every residue mod 16 on both sides, whatever the front
    blob, reqs = xs.alignment_batch()
    want = xs.expected(blob, reqs, xs.N_KEYS, 10 ** 7)
    assert not want["status"].any() and len(reqs) == 65
    assert {int(r["off"]) % 16 for r in reqs} == set(range(16)) == {int(c["off"]) % 16 for c in want["out_certs"]}


def test_mixes_and_the_mutation_sweep_of_the_restatement():
    for mix in xs.MIXES:
        blob, reqs = xs.seam_case(65, mix, seed=2)
        want = xs.expected(blob, reqs, xs.N_KEYS, 10 ** 7)
        hist = np.bincount(want["status"], minlength=12)
        if mix in ("mod3", "only44", "only87"):
            assert hist[0] == 65
        elif mix == "all_defect":
            assert hist[0] == 0 and min(hist[c] for c in (xs.ENTRY, xs.KEY, xs.RANGE, xs.DER, xs.ALG)) > 0
        else:
            assert hist[0] == 65 - 6
        check_contract(xs.framed(np.zeros(want["totals"][2], dtype=np.uint8), want, {i: bytes(len(f) - int(reqs[i]["len"]) - 22)
                                                                                        for i, f in want["frames"].items()}), want, reqs)
    tbs = xs.good_tbs(44, b"mut", 0)
    blob, reqs = xs.mutation_batch(tbs)
    assert len(reqs) == xc.MUTATION_SPAN * len(xc.MUTATION_VALUES) == 910
    hist = np.bincount(xs.expected(blob, reqs, xs.N_KEYS, 10 ** 7)["status"], minlength=12)
    # the sweep reaches the rules: headers (DER), the 11 bytes of the inner OID times seven values (ALG), content nobody looks at (accepted)
    assert hist[xs.ALG] == 77 and hist[xs.DER] > 0 and hist[xs.OK] > 0 and hist[xs.OK] + hist[xs.DER] + hist[xs.ALG] == 910


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the certificates independently")
def test_framed_certificates_parse_with_openssl_asn1parse(tmp_path):
    for pset in xs.SETS:
        tbs = xs.good_tbs(pset, b"ossl", pset, tail=xc.extensions(33))
        st, want, _, _ = one(pset, tbs)
        der = xs.framed(np.zeros(want["totals"][2], dtype=np.uint8), want, {0: xc._bytes(b"osig", pset, xs.SIG_LEN[pset])}).tobytes()
        path = tmp_path / ("c%d.der" % pset)
        path.write_bytes(der)
        run = subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(path)], capture_output=True, text=True)
        assert st == 0 and run.returncode == 0, run.stderr
        d1 = [ln for ln in run.stdout.splitlines() if ":d=1 " in ln]
        assert len(d1) == 3 and "SEQUENCE" in d1[0] and "SEQUENCE" in d1[1] and "BIT STRING" in d1[2]
        assert re.match(r"\s*4:d=1\s+hl=4\s+l=\s*%d\s" % (len(tbs) - 4), d1[0]) and re.search(r"l=\s*%d\s" % (xs.SIG_LEN[pset] + 1), d1[2])


def test_signing_cases_on_the_oracle():
    """Every batch the GPU file signs, signed by the oracle: the finished certificate verifies under the issuer's public key and is OK to
    the verifying side's walk, and no request needs more than ITER_BOUND iterations of the signing loop -- the candidates ONE round gives
    one op at most (MLDSA_OPT_SPEC_MAX as a context starts, tests/long_tail_cases.py).  mldsa_recsign_sign signs through the synchronous
    mldsa_sign, which adds rounds until every op is signed, so the GPU tests may demand sig_status == MLDSA_OK for every accepted
    certificate and leave no case out; ops that outlast a call's plan are tests/test_gpu_sign_long_tail.py's."""
    keys = xs.oracle_keys()
    for name, requests in xs.signing_cases().items():
        sigs, iters = xs.oracle_signed(name)
        assert max(iters) <= xs.ITER_BOUND, (name, max(iters))
        blob, reqs = xs.tbs_blob(requests, pad=list(range(16)))
        want = xs.expected(blob, reqs, xs.SIGN_N_KEYS, 10 ** 7)
        assert not want["status"].any(), name
        out = xs.framed(np.zeros(want["totals"][2], dtype=np.uint8), want, dict(enumerate(sigs)))
        check_contract(out, want, reqs)
        raw = out.tobytes()
        for i, (pset, key, tbs, rnd, issuer) in enumerate(requests):
            c = want["out_certs"][i]
            assert raw[int(c["off"]):int(c["off"]) + int(c["len"])] == xc.cert(tbs, pset, sigs[i]) and int(c["issuer"]) == issuer
            if i % 16 == 0 or name == "chains":
                assert orc.verify_internal(pset, keys[pset][key][0], tbs, sigs[i], ctx=b"", mode=orc.MODE_PURE), (name, i)
    # the chains link: the verifying side's restatement accepts every certificate under its issuer's subject key and Name
    requests = xs.signing_cases()["chains"]
    sigs, _ = xs.oracle_signed("chains")
    ders = [xc.cert(r[2], r[0], s) for r, s in zip(requests, sigs)]
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [r[4] for r in requests], pad=3)
    fields, ops, status = xc.expected(blob, certs)
    assert status.tolist() == [0] * 12
    raw = blob.tobytes()
    for op in ops:
        pset = int(op["set"])
        cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
        assert orc.verify_internal(pset, orc.pk_try_from_bytes(pset, cut(op["pk_off"], xc.PK_LEN[pset])), cut(op["msg_off"], op["msg_len"]),
                                   cut(op["sig_off"], xc.SIG_LEN[pset]), ctx=b"", mode=orc.MODE_PURE)


# ---- the rules, the walk and the frame under the sanitizers --------------------------------------------------------------------------
def test_the_rules_the_walk_and_the_frame_under_asan_and_ubsan(tmp_path):
    lines = []
    for pset in xs.SETS:
        tbs = xs.good_tbs(pset, b"san", pset, tail=xc.extensions(5))
        lines.append("W %d %d %s" % (pset, xs.OK, tbs.hex()))
        lines.append("W %d %d %s" % (pset, xs.OK, xs.good_tbs(pset, b"san1", pset, v3=False).hex()))
        lines.append("W %d %d %s" % (xs.SETS[(xs.SETS.index(pset) + 1) % 3], xs.ALG, tbs.hex()))
        for name in xs.BYTE_DEFECTS:
            data, n = xs.byte_defect(tbs, pset, name)
            assert xs.walk_tbs(data[:n], pset) == xs.BYTE_DEFECTS[name], name
            lines.append("W %d %d %s" % (pset, xs.BYTE_DEFECTS[name], data[:n].hex()))
        for pos in range(xc.MUTATION_SPAN):  # the single-byte sweep; the expected status is the restatement's
            for v in xc.MUTATION_VALUES:
                m = tbs[:pos] + bytes([v]) + tbs[pos + 1:]
                lines.append("W %d %d %s" % (pset, xs.walk_tbs(m, pset), m.hex()))
    # the entries' rules: the defect batch's requests (their status up to LONG; a walked one counts as 0), and the length edges
    blob, reqs, _ = xs.defect_batch()
    entries = [(r, blob.size) for r in reqs] + [(r, xs.edge_batch()[0].size) for r in xs.edge_batch()[1]]
    probe = np.zeros(4, dtype=_x509sign_lib.REQ_DTYPE)
    probe["set"], probe["len"] = 87, (2, 1, xs.MAX_TBS[87], xs.MAX_TBS[87] + 1)
    probe["off"] = (2 ** 64 - 1, 0, 100, 100)
    entries += [(r, 2 ** 64 - 1) for r in probe]
    for n_keys in (xs.N_KEYS, (0, 4, 1)):
        for r, blob_len in entries:
            pset, flags = int(r["set"]), int(r["flags"])
            if pset not in xs.SETS or flags & ~1 or int(r["reserved"]):
                st = xs.ENTRY
            elif int(r["key"]) >= n_keys[xs.SETS.index(pset)]:
                st = xs.KEY
            elif int(r["off"]) + int(r["len"]) > blob_len or int(r["len"]) < 2 or (flags & 1 and int(r["rnd_off"]) + 32 > blob_len):
                st = xs.RANGE
            else:
                st = xs.LONG if int(r["len"]) > xs.MAX_TBS[pset] else xs.OK
            lines.append("E %d %d %d %d %d %d %d %d %d %d %d %d" % (st, int(r["off"]), int(r["rnd_off"]), int(r["len"]), int(r["key"]), pset, flags,
                                                                   int(r["reserved"]), blob_len, *n_keys))
    kinds = {int(ln.split()[1]) for ln in lines if ln[0] == "E"}
    assert kinds == {xs.OK, xs.ENTRY, xs.KEY, xs.RANGE, xs.LONG}
    table = tmp_path / "x509sign_table.txt"
    table.write_text("\n".join(lines) + "\n")
    sanitized_program(tmp_path, "x509sign_plan", ["x509sign_plan_main.cpp"], "x509sign_plan OK", env={"X509SIGN_TABLE": str(table)})
