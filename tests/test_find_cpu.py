"""The path-building library (include/mldsa_find.h, fips204_amd/find/libmldsa_find.so) without a device: its C ABI, how it is linked
against the core, its host helpers and argument checks, its kernels' resources, the restatement of tests/find_cases.py against pinned
offsets and openssl, and the identifier walk, the key comparison, the hash and the slot count as a stand-alone program under the
sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crl_cases as cc
import find_cases as fc
import path_cases as pc
import x509_cases as xc
from fips204_amd import _crl_lib, _find_lib, _lib, _mus_lib, _path_lib, _x509_lib
from layer_checks import (ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, sources_clean)

FIND_DIR = os.path.join(ROOT, "fips204_amd", "find")
SOURCES = ["Makefile", "find.hip", "find_plan.h"]
KERNELS = ("k_find_ids", "k_find_claim", "k_find_confirm", "k_find_issuers", "k_find_crl_issuers", "k_find_ca_min", "k_find_cert_crl")
ENTRY_POINTS = {"mldsa_find_abi_version", "mldsa_find_last_error", "mldsa_find_table_slots", "mldsa_find_scratch_bytes", "mldsa_find_ids",
                "mldsa_find_table", "mldsa_find_issuers", "mldsa_find_build", "mldsa_find_crl_issuers", "mldsa_find_cert_crls"}


@pytest.fixture(scope="module")
def lib():
    return built(_find_lib, FIND_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(lib, tmp_path):
    from fips204_amd import build
    assert build.FIND_LAYERS == {"find": "libmldsa_find.so"} and build.PATH_LAYERS == {"path": "libmldsa_path.so"}
    assert build.FIND_LIB == _find_lib.LIB_PATH and build.FIND_DIR == FIND_DIR
    # find_plan.h includes the plan headers of two other layers: the shadow links their directories
    (tmp_path / "fips204_amd").mkdir()
    for d in (build.REC_DIR, build.X509_DIR):
        os.symlink(d, tmp_path / "fips204_amd" / os.path.basename(d))
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS, **build.ISSUE_LAYERS,
                                                         **build.REQUEST_LAYERS, **build.REVOCATION_LAYERS, **build.PATH_LAYERS,
                                                         **build.FIND_LAYERS}.items()]
    assert libs[-1] == _find_lib.LIB_PATH and libs[-2] == _path_lib.LIB_PATH  # built last, behind the path layer
    clean_build("find", _find_lib, SOURCES, libs, tmp_path)
    mk = open(os.path.join(FIND_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../x509/x509_plan.h", "../x509/x509_dev.h", "../rec/rec_plan.h", "find_plan.h", "mldsa_find.h", "mldsa_path.h", "mldsa_crl.h", "mldsa_x509.h", "mldsa_rec.h"):
        assert h in mk, h  # a change of a shared header rebuilds this library
    assert not re.search(r"-lmldsa_(rec|recsign|x509|x509sign|csr|crl|path)\b", mk)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_find_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(lib, tmp_path):
    declared, text = header_and_exports(
        _find_lib, lib,
        "#include <stddef.h>\n"
        "int main(void) { mldsa_find_id d; mldsa_find_result r; mldsa_find_totals t; mldsa_path_fields p;\n"
        "  d.reserved[4] = 0; r.reserved[2] = 0; t.overflow = 0; p.ext_len = 0;\n"
        "  return sizeof(d) == 24 && sizeof(r) == 12 && sizeof(t) == 16 && sizeof(p) == 48\n"
        "    && offsetof(mldsa_find_id, aki_off) == 8 && offsetof(mldsa_find_id, ski_len) == 16 && offsetof(mldsa_find_id, aki_len) == 17\n"
        "    && offsetof(mldsa_find_id, status) == 18 && offsetof(mldsa_find_result, candidates) == 4 && offsetof(mldsa_find_result, status) == 8\n"
        "    && offsetof(mldsa_find_totals, overflow) == 12\n"
        "    && mldsa_find_abi_version() == MLDSA_FIND_ABI_VERSION && MLDSA_FIND_EXT == 26 && MLDSA_FIND_EXT > MLDSA_PATH_CRITICAL\n"
        "    && MLDSA_FIND_MAX_CERTS <= MLDSA_X509_MAX_CERTS && MLDSA_FIND_SPACE == 3\n"
        "    && !d.reserved[4] && !r.reserved[2] && !t.overflow && !p.ext_len ? 0 : 1; }\n",
        r"\b(mldsa_find_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == ENTRY_POINTS
    for h in ("mldsa_rec.h", "mldsa_x509.h", "mldsa_crl.h", "mldsa_path.h"):
        assert '#include "%s"' % h in text  # for the types and the codes only
    assert "#define MLDSA_FIND_ABI_VERSION 1" in text and lib.mldsa_find_abi_version() == _find_lib.ABI_VERSION == 1
    assert "#define MLDSA_FIND_MAX_CERTS (1u << 28)" in text and _find_lib.MAX_CERTS == 1 << 28
    assert "#define MLDSA_FIND_MAX_KEYID 64" in text and _find_lib.MAX_KEYID == fc.MAX_KEYID == 64
    assert "#define MLDSA_FIND_PROBE_MAX 256" in text and _find_lib.PROBE_MAX == fc.PROBE_MAX == 256
    assert "#define MLDSA_FIND_OVERFLOW_MAX 1024" in text and _find_lib.OVERFLOW_MAX == fc.OVERFLOW_MAX == 1024
    assert re.search(r"#define MLDSA_FIND_EXT 26\b", text) and _find_lib.EXT == fc.EXT == 26
    for code, name in enumerate(("FOUND", "NONE", "CERT", "SPACE")):
        assert re.search(r"#define MLDSA_FIND_%s %d\b" % (name, code), text), name
        assert getattr(_find_lib, name) == getattr(fc, name) == code
    # codes 0 ... 2 are the certificate library's; the new one is behind every code of the other headers (0 ... 25)
    for name in ("OK", "RANGE", "DER"):
        assert getattr(_find_lib, name) == getattr(_x509_lib, name) == getattr(fc, name)
    assert _find_lib.EXT == max(_path_lib.VERSION, _path_lib.TIME, _path_lib.EXT, _path_lib.CRITICAL) + 1
    assert fc.NO_ISSUER == _find_lib.NO_ISSUER == _x509_lib.NO_ISSUER and fc.CRL_NONE == _find_lib.CRL_NONE == _crl_lib.NONE and fc.MAX_EXTS == pc.MAX_EXTS
    # the layouts
    assert (_find_lib.ID_DTYPE.itemsize, _find_lib.RESULT_DTYPE.itemsize, _find_lib.TOTALS_DTYPE.itemsize) == (24, 12, 16)
    assert [_find_lib.ID_DTYPE.fields[f][1] for f in ("ski_off", "aki_off", "ski_len", "aki_len", "status", "reserved")] == [0, 8, 16, 17, 18, 19]
    assert [_find_lib.RESULT_DTYPE.fields[f][1] for f in ("issuer", "candidates", "status", "reserved")] == [0, 4, 8, 9]
    assert [_find_lib.TOTALS_DTYPE.fields[f][1] for f in ("candidates", "keys", "slots", "overflow")] == [0, 4, 8, 12]
    # what is out of scope is said, and a measurement is stated only where its file exists
    for word in ("NOT IN SCOPE", "authorityCertIssuer / authorityCertSerialNumber", "string\n * preparation rules", "AIA fetching", "PEM",
                 "C++ / Rust mirrors", "walk_ids", "k_find_claim", "k_find_confirm", "55 1D 0E", "55 1D 23", "O(n), not O(n^2)",
                 "A wrong issuer is never named", "LOWEST index"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "find_bench.jsonl")):
        assert "not measured" in text and "from counts (an expectation)" in text


def test_layered_on_the_one_core_library(lib):
    layered_on_core(_find_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_sign", "mldsa_verify", "mldsa_verify_pk", "mldsa_keygen", "mldsa_rec_verify", "mldsa_rec_plan", "mldsa_rec_pack",
                           "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops", "mldsa_csr_parse", "mldsa_crl_parse", "mldsa_crl_ops",
                           "mldsa_crl_table", "mldsa_crl_check", "mldsa_path_parse", "mldsa_path_chain", "mldsa_keys_dedup"))
    links_the_core_and_never_builds_it(FIND_DIR)
    dyn = subprocess.run(["readelf", "-d", _find_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign|x509|x509sign|csr|crl|path)\.so", dyn)
    no_new_dynamic_symbol(_find_lib.LIB_PATH, "mldsa_find_")


def test_kernels_do_not_spill_and_sources_are_clean(lib):
    kernels = [k for k in kernel_resources(FIND_DIR) if "k_find" in k]
    for stem in KERNELS:
        assert sum(stem + "E" in nm for nm in kernels) == 1, stem  # (the mangled name: the stem, then its parameters)
    assert len(kernels) == len(KERNELS)
    read = dict(sources_clean(FIND_DIR, ["../../include/mldsa_find.h", "../_find_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]))
    src, plan = read["find.hip"], read["find_plan.h"]
    certificate_helpers_shared_once("find")
    for h in ("../layer/layer_host.h", "../layer/layer_dev.h", "../x509/x509_dev.h", "../../include/mldsa_find.h", "find_plan.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../x509/x509_plan.h"' in plan and '#include "../rec/rec_plan.h"' in open(os.path.join(FIND_DIR, "..", "x509", "x509_plan.h")).read()
    # no wave waits for another, no host wait, no allocation; the scaffold and the shared readers are included, not copied
    for word in ("__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "hipStreamSynchronize", "hipMemcpy",
                 "hipMalloc", "hipDeviceSynchronize", "struct DeviceScope", "thread_local", "int fail(", "mldsa_rec_verify(", "mldsa_x509_parse(",
                 "mldsa_crl_parse(", "mldsa_path_parse("):
        assert word not in src and word not in plan, word
    for name in ("read_tlv", "oid_set", "in_range", "wave_or", "wave_max", "walk"):
        defined = r"^[^\n;=/]*\b(void|bool|int|uint32_t|uint64_t|Tlv|Walk)\s+%s\s*\(" % name
        assert not re.search(defined, src + plan, flags=re.M), name
    # the plan has no HIP in it, and the kernels keep no second copy of its rules: they call the plan's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan and "atomic" not in code
    kernel_code = re.sub(r"//[^\n]*", "", src)
    for call in ("walk_ids(", "candidate_row(", "seeker_row(", "inside(", "in_range(", "same_shape(", "key_byte_diff(", "byte_term(", "finish_hash(",
                 "join(", "result_status(", "table_slots(", "layout(", "scratch_bytes("):
        assert call in kernel_code and "constexpr" in plan, call
    for word in ("read_tlv", "0x0E", "0x23", "0xA1", "0x1D", "0xBF58476D1CE4E5B9"):  # the rules live in the plan alone
        assert word in plan and word not in kernel_code, word
    # every loop of a kernel that probes or scans has a constant or table-size bound
    assert kernel_code.count("p < PROBE_MAX") == 2 and "q < n_overflow" in kernel_code and "n_overflow > OVERFLOW_MAX" in kernel_code
    assert "k < MAX_EXTS" in code and not re.search(r"\[\s*\w*\s*\]\s*=\s*\{", code)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_never_abort(lib):
    null = None
    room = lib.mldsa_find_scratch_bytes(4)
    buf = (C.c_uint8 * (room + 512))()  # (aligned_buffer's 3840 bytes are fewer than the scratch of four certificates)
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)
    odd4, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    err = lib.mldsa_find_last_error
    seed = bytes(16)

    def ids(ctx=null, blob=p, blob_len=1024, certs=p, policy=p, n=4, ids=p, stream=null):
        return lib.mldsa_find_ids(ctx, blob, blob_len, certs, policy, n, ids, stream)

    def table(ctx=null, blob=p, blob_len=1024, certs=p, fields=p, ids=p, n=4, seed=seed, hash_bits=64, totals=p, scratch=p, scratch_bytes=room,
              stream=null):
        return lib.mldsa_find_table(ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes, stream)

    def issuers(ctx=null, blob=p, blob_len=1024, certs=p, fields=p, ids=p, n=4, seed=seed, hash_bits=64, totals=p, scratch=p, scratch_bytes=room,
                certs_out=p, results=p, stream=null):
        return lib.mldsa_find_issuers(ctx, blob, blob_len, certs, fields, ids, n, seed, hash_bits, totals, scratch, scratch_bytes, certs_out, results,
                                      stream)

    def build(ctx=null, blob=p, blob_len=1024, certs=p, fields=p, policy=p, n=4, seed=seed, hash_bits=64, ids=p, totals=p, certs_out=p, results=p,
              scratch=p, scratch_bytes=room, stream=null):
        return lib.mldsa_find_build(ctx, blob, blob_len, certs, fields, policy, n, seed, hash_bits, ids, totals, certs_out, results, scratch,
                                    scratch_bytes, stream)

    def crl_issuers(ctx=null, blob=p, blob_len=1024, crls=p, crl_fields=p, n_crls=2, certs=p, fields=p, ids=p, n=4, seed=seed, hash_bits=64, totals=p,
                    scratch=p, scratch_bytes=room, crls_out=p, crl_results=p, stream=null):
        return lib.mldsa_find_crl_issuers(ctx, blob, blob_len, crls, crl_fields, n_crls, certs, fields, ids, n, seed, hash_bits, totals, scratch,
                                          scratch_bytes, crls_out, crl_results, stream)

    def cert_crls(ctx=null, certs=p, n=4, crls=p, n_crls=2, cert_crl=p, scratch=p, scratch_bytes=room, stream=null):
        return lib.mldsa_find_cert_crls(ctx, certs, n, crls, n_crls, cert_crl, scratch, scratch_bytes, stream)

    calls = (ids, table, issuers, build, crl_issuers, cert_crls)
    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in calls:
        assert call() == _lib.ERR_PARAM and b"NULL context" in err(), call.__name__
    fake = p  # a fake non-NULL context must still be refused before it is touched
    for call in (ids, table, issuers, build, crl_issuers):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    for call, pointers, aligned8, aligned4 in (
            (ids, ("certs", "ids"), ("certs", "policy", "ids"), ()),
            (table, ("certs", "fields", "ids", "seed", "totals"), ("certs", "fields", "ids"), ("totals",)),
            (issuers, ("certs", "fields", "ids", "seed", "totals", "certs_out", "results"), ("certs", "fields", "ids", "certs_out"), ("totals", "results")),
            (build, ("certs", "fields", "ids", "seed", "totals", "certs_out", "results"), ("certs", "fields", "policy", "ids", "certs_out"),
             ("totals", "results")),
            (crl_issuers, ("crls", "crl_fields", "certs", "fields", "ids", "seed", "totals", "crls_out", "crl_results"),
             ("crls", "crl_fields", "certs", "fields", "ids", "crls_out"), ("totals", "crl_results")),
            (cert_crls, ("certs", "crls", "cert_crl"), ("certs", "crls"), ("cert_crl",))):
        for name in pointers:
            assert call(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), (call.__name__, name)
        for name in aligned8:
            assert call(ctx=fake, **{name: odd4}) == _lib.ERR_PARAM and b"8-byte aligned" in err(), (call.__name__, name)
        for name in aligned4:
            assert call(ctx=fake, **{name: odd2}) == _lib.ERR_PARAM and b"4-byte aligned" in err(), (call.__name__, name)
    for call in calls:
        for n in (_find_lib.MAX_CERTS + 1, 2 ** 64 - 1):
            assert call(ctx=fake, n=n) == _lib.ERR_PARAM and b"MLDSA_FIND_MAX_CERTS certificates" in err(), call.__name__
    for call in (crl_issuers, cert_crls):
        assert call(ctx=fake, n_crls=_find_lib.MAX_CERTS + 1) == _lib.ERR_PARAM and b"MLDSA_FIND_MAX_CERTS CRLs" in err()
    for call in (table, issuers, build, crl_issuers):
        for bits in (0, 65, -1):
            assert call(ctx=fake, hash_bits=bits) == _lib.ERR_PARAM and b"hash_bits outside 1 ... 64" in err()
    for call in (table, issuers, build, crl_issuers, cert_crls):
        assert call(ctx=fake, scratch=null) == _lib.ERR_PARAM and b"mldsa_find_scratch_bytes" in err()
        assert call(ctx=fake, scratch=C.c_void_p(p.value + 128)) == _lib.ERR_PARAM and b"256-byte aligned" in err()
        assert call(ctx=fake, scratch_bytes=room - 1) == _lib.ERR_PARAM and b"smaller than" in err()
        assert call(ctx=fake, n=17, scratch_bytes=room) == _lib.ERR_PARAM and b"smaller than" in err()
    # a NULL blob is an empty blob's and policy may be NULL: the checks go on to the next one
    assert ids(ctx=fake, blob=null, blob_len=0, policy=null, ids=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert build(ctx=null, policy=null) == _lib.ERR_PARAM and b"NULL context" in err()
    assert cert_crls(ctx=null, crls=null, n_crls=0) == _lib.ERR_PARAM and b"NULL context" in err()
    # empty calls succeed without a context, and touch nothing
    assert ids(n=0, blob=null, certs=null, ids=null) == _lib.OK
    assert table(n=0, certs=null, fields=null, ids=null, seed=null, hash_bits=0, totals=null, scratch=null, scratch_bytes=0) == _lib.OK
    assert issuers(n=0, certs=null, fields=null, ids=null, seed=null, totals=null, scratch=null, scratch_bytes=0, certs_out=null, results=null) == _lib.OK
    assert build(n=0, certs=null, fields=null, ids=null, seed=null, totals=null, scratch=null, scratch_bytes=0, certs_out=null, results=null) == _lib.OK
    assert crl_issuers(n_crls=0, crls=null, crl_fields=null, crls_out=null, crl_results=null, scratch=null) == _lib.OK
    assert cert_crls(n=0, certs=null, cert_crl=null, scratch=null, scratch_bytes=0) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(lib):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert lib.mldsa_find_cert_crls(p, p, 4, p, 2, p, p, 255, null) == _lib.ERR_PARAM
    mine = lib.mldsa_find_last_error()
    assert mine == b"mldsa_find_cert_crls: scratch is NULL, not 256-byte aligned or smaller than mldsa_find_scratch_bytes"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert lib.mldsa_find_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _find_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "walk_ids", "key_hash", "k_find", "lookup"):
        assert word not in exported, word
    del buf


def test_scratch_bytes_and_table_slots(lib):
    last = 0
    for n in (0, 1, 15, 16, 17, 32, 33, 63, 64, 65, 257, 1000, 65536, 65537, 1 << 28):
        slots, got = lib.mldsa_find_table_slots(n), lib.mldsa_find_scratch_bytes(n)
        assert slots == fc.table_slots(n) and slots >= max(64, 4 * n) and slots & (slots - 1) == 0 and (slots == 64 or slots < 8 * n)
        assert got == fc.scratch_bytes(n) and got >= last and got % 256 == 0
        last = got
    for n in ((1 << 28) + 1, 2 ** 63, 2 ** 64 - 1):
        assert lib.mldsa_find_scratch_bytes(n) == 0 and lib.mldsa_find_table_slots(n) == 0


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
KID = fc.KID


def ext_range(der):
    w = pc.walk_policy(der)
    assert w["status"] == 0
    return w["ext_off"], w["ext_off"] + w["ext_len"]


def test_identifiers_have_the_pinned_offsets():
    name = xc.name(b"issuer")
    for exts, ski_at, aki_at in (([fc.ski_ext(KID)], 11, None), ([fc.aki_ext(KID)], None, 13),
                                 ([pc.basic(), fc.ski_ext(KID), fc.aki_ext(KID, name, b"\x12\x34")], None, None)):
        der = fc.cert(44, 44, name, xc.name(b"subject"), b"pin", 0, exts)
        lo, hi = ext_range(der)
        w = fc.walk_ids(der, lo, hi)
        assert w["status"] == fc.OK
        # 30 1D 06 03 55 1D 0E 04 16 04 14 <20 bytes>: the identifier lies 11 bytes into its extension; 30 1F 06 03 55 1D 23 04 18 30 16 80 14: 13
        if ski_at is not None:
            assert (w["ski_off"], w["ski_len"], w["aki_len"]) == (lo + ski_at, 20, 0)
        if aki_at is not None:
            assert (w["aki_off"], w["aki_len"], w["ski_len"]) == (lo + aki_at, 20, 0)
        for f in ("ski", "aki"):
            if w[f + "_len"]:
                assert der[w[f + "_off"]:w[f + "_off"] + w[f + "_len"]] == KID
                assert der[w[f + "_off"] - 2:w[f + "_off"]] == (b"\x04\x14" if f == "ski" else b"\x80\x14")
    # a certificate without extensions, and one whose extensions hold neither
    assert pc.walk_policy(fc.cert(44, 44, name, name, b"pin", 1))["ext_len"] == 0
    lo, hi = ext_range(fc.cert(44, 44, name, name, b"pin", 2, [pc.basic(), pc.other(1)]))
    assert fc.walk_ids(fc.cert(44, 44, name, name, b"pin", 2, [pc.basic(), pc.other(1)]), lo, hi) == dict(status=0, ski_off=0, ski_len=0, aki_off=0, aki_len=0)


def test_every_value_rule_gives_its_documented_status():
    seen = set()
    for content, status in fc.value_cases():
        w = fc.walk_ids(content, 0, len(content))
        assert w["status"] == status, (content.hex(), w)
        if status != fc.OK:
            assert not any(w[f] for f in w if f != "status")
        seen.add(status)
    assert seen == {fc.OK, fc.DER, fc.EXT}


def test_expected_ids_follows_only_what_it_may():
    name = xc.name(b"n")
    ders = [fc.cert(44, 44, name, name, b"ids", i, [fc.ski_ext(KID), fc.aki_ext(KID)]) for i in range(5)]
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [None] * 5, pad=3)
    policy = pc.expected_parse(blob, certs)
    assert (fc.expected_ids(blob, certs, None)["status"] == 0).all() and not fc.expected_ids(blob, certs, None)["ski_len"].any()
    policy[1]["ext_off"] = int(certs[1]["off"]) - 1                        # begins in front of the certificate
    policy[2]["ext_len"] = int(certs[2]["len"])                            # ends behind it
    policy[3]["status"] = pc.DER                                           # a row that says it found nothing is believed
    policy[4]["ext_off"] = 2 ** 64 - 8
    ids = fc.expected_ids(blob, certs, policy)
    assert ids["status"].tolist() == [0, fc.RANGE, fc.RANGE, 0, fc.RANGE] and ids["ski_len"].tolist() == [20, 0, 0, 0, 0]


def test_lookup_restatement_on_hand_made_batches():
    root, other_root, ca = xc.name(b"root"), xc.name(b"rooT"), xc.name(b"ca")
    k1, k2 = bytes([1] * 20), bytes([2] * 20)
    ders = [fc.cert(44, 44, root, root, b"t", 0, [fc.ski_ext(k1), fc.aki_ext(k1)]),      # 0 a self-signed root
            fc.cert(44, 44, root, root, b"t", 1, [fc.ski_ext(k2)]),                      # 1 the same Name, rolled over to another key
            fc.cert(44, 44, root, ca, b"t", 2, [fc.aki_ext(k2)]),                        # 2 issued under the new key
            fc.cert(44, 44, root, ca, b"t", 3),                                          # 3 no AKI: both roots match
            fc.cert(65, 44, root, ca, b"t", 4),                                          # 4 signed with another parameter set
            fc.cert(44, 44, other_root, ca, b"t", 5),                                    # 5 a Name that differs in its last byte
            fc.cert(44, 0, ca, xc.name(b"leaf"), b"t", 6, [fc.aki_ext(k1)]),             # 6 under 2 and 3, which carry no SKI
            fc.cert(44, 44, root, root, b"t", 7, [fc.aki_ext(k2)])]                      # 7 self-issued, its AKI is certificate 1's SKI
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [None] * len(ders), pad=[5, 0, 11])
    fields, _, _ = xc.expected(blob, certs)
    ids = fc.expected_ids(blob, certs, pc.expected_parse(blob, certs))
    res, out = fc.expected_issuers(blob, certs, fields, ids)
    assert res["status"].tolist() == [0, 0, 0, 0, fc.NONE, fc.NONE, 0, 0]
    assert res["issuer"].tolist() == [0, 0, 1, 0, fc.NO_ISSUER, fc.NO_ISSUER, 2, 1] and out["issuer"].tolist() == res["issuer"].tolist()
    # 7 carries no SKI: no AKI excludes it, while 0's own AKI excludes 1; 6 finds the four certificates named "ca", none of which has an SKI
    assert res["candidates"].tolist() == [2, 3, 2, 3, 0, 0, 4, 2]
    # by Name alone (no policy rows): the lowest index of every Name
    res, _ = fc.expected_issuers(blob, certs, fields, fc.expected_ids(blob, certs, None))
    assert res["issuer"].tolist() == [0, 0, 0, 0, fc.NO_ISSUER, fc.NO_ISSUER, 2, 0] and res["candidates"].tolist() == [3, 3, 3, 3, 0, 0, 4, 3]
    # CRLs: by Name and AKI, and the lowest CRL of every CA
    crls = [fc.crl(44, root, b"l", 0, ext=fc.aki_ext(k2) + cc.crl_number()), fc.crl(44, root, b"l", 1), fc.crl(44, xc.name(b"nobody"), b"l", 2),
            fc.crl(44, root, b"l", 3, ext=None)]
    blob2, rows = xc.lay_out([(d, len(d)) for d in ders + crls], [None] * (len(ders) + len(crls)), pad=[5, 0, 11])
    assert np.array_equal(blob2[:blob.size - 1], blob[:-1])
    items = rows[len(ders):].astype(_crl_lib.ITEM_DTYPE)
    crl_fields = cc.expected_parse(blob2, items)
    res_c, items_out = fc.expected_crl_issuers(blob2, items, crl_fields, certs, fields, ids)
    assert res_c["status"].tolist() == [0, 0, fc.NONE, 0] and res_c["issuer"].tolist() == [1, 0, fc.NO_ISSUER, 0] and res_c["candidates"].tolist() == [2, 3, 0, 3]
    assert fc.expected_cert_crls(out["issuer"], items_out["issuer"]).tolist() == [1, 1, 0, 1, fc.CRL_NONE, fc.CRL_NONE, fc.CRL_NONE, 0]
    # a table that ran over: only the keys known to lie in a group are answered
    first = fc.candidate_keys(blob.tobytes(), certs[0], fields[0], ids[0])[0]
    res, _ = fc.expected_issuers(blob, certs, fields, ids, in_group={first})
    assert res["status"].tolist() == [fc.SPACE, fc.FOUND, fc.SPACE, fc.FOUND, fc.SPACE, fc.SPACE, fc.SPACE, fc.SPACE]


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the certificates independently")
def test_builder_and_walk_agree_with_openssl_asn1parse(tmp_path):
    name = xc.name(b"issuer")
    for exts in ([fc.ski_ext(KID), fc.aki_ext(bytes(32))], [pc.basic(), fc.aki_ext(KID, name, b"\x12\x34"), fc.ski_ext(bytes(64))]):
        der = fc.cert(65, 65, name, xc.name(b"subject"), b"ossl", 0, exts)
        path = tmp_path / "c.der"
        path.write_bytes(der)
        run = subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        lines = [re.match(r"\s*(\d+):d=(\d+)\s+hl=\s*(\d+)\s+l=\s*(\d+)\s+(cons|prim):\s+(.*)", ln) for ln in run.stdout.splitlines()]
        rows = [(int(m.group(1)), int(m.group(3)), int(m.group(4)), m.group(6)) for m in lines if m]
        lo, hi = ext_range(der)
        w = fc.walk_ids(der, lo, hi)
        assert w["status"] == 0
        # the OCTET STRING that follows each of the two OIDs holds the value: its content begins where openssl says
        for label, field, inner in (("X509v3 Subject Key Identifier", "ski", 2), ("X509v3 Authority Key Identifier", "aki", 4)):
            at = [i for i, r in enumerate(rows) if label in r[3]]
            assert len(at) == 1
            octets = rows[at[0] + 1]
            assert "OCTET STRING" in octets[3]
            assert w[field + "_off"] == octets[0] + octets[1] + inner and octets[0] + octets[1] + octets[2] >= w[field + "_off"] + w[field + "_len"]


# ---- the plan under the sanitizers ---------------------------------------------------------------------------------------------------
def test_the_walk_the_compare_rule_the_hash_and_the_slot_count_under_asan_and_ubsan(tmp_path):
    hexed = lambda b: b.hex() if b else "-"  # noqa: E731
    lines, want = [], []
    contents = [c for c, _ in fc.value_cases()]
    base = pc.basic() + fc.ski_ext(KID) + fc.aki_ext(KID, xc.name(b"ca"), b"\x12\x34")
    contents = [base] + contents
    for pos in range(len(base)):  # every single-byte change of a content that holds everything
        contents += [base[:pos] + bytes([v]) + base[pos + 1:] for v in xc.MUTATION_VALUES]
    seen = set()
    for c in contents:
        w = fc.walk_ids(c, 0, len(c))
        lines.append("I " + hexed(c))
        want.append("%d %d %d %d %d" % (w["status"], w["ski_off"], w["ski_len"], w["aki_off"], w["aki_len"]))
        seen.add(w["status"])
    assert seen == {fc.OK, fc.DER, fc.EXT}
    # keys: every Name length of the compare step's edges, Names that differ in their last byte or in length alone, every kind
    kinds = {fc.ANY: 1, fc.SKI: 2, fc.NOSKI: 3}
    keys = []
    for length in fc.NAME_LENGTHS:
        nm = fc.name_of_len(length, b"k")
        keys += [(1, 44, nm, b""), (3, 44, nm, b""), (1, 65, nm, b""), (2, 44, nm, KID), (2, 44, nm, KID[:-1] + b"\x00"), (2, 44, nm, KID + b"\x00")]
        if length > 2:
            keys += [(1, 44, nm[:-1] + bytes([nm[-1] ^ 1]), b""), (1, 44, nm + b"\x00", b""), (1, 44, nm[:-1], b"")]
    keys += [(2, 44, b"\x30\x00", bytes(n)) for n in (1, 32, 64)]
    assert len(set(keys)) == len(keys) and set(kinds.values()) == {1, 2, 3}
    pairs = [(a, a) for a in keys] + [(keys[i], keys[j]) for i in range(len(keys)) for j in (i + 1, i + 2, i + 7) if j < len(keys)]
    for a, b in pairs:
        lines.append("K " + " ".join("%d %d %s %s" % (k[0], k[1], hexed(k[2]), hexed(k[3])) for k in (a, b)))
        want.append("%d %d 1" % (a == b, a == b))  # equal keys hash alike; unequal ones do not (a 64-bit collision aside)
    for n in (0, 1, 16, 17, 1000, 65536, 1 << 28, (1 << 28) + 1):
        lines.append("S %d" % n)
        want.append("%d %d" % ((fc.table_slots(n), fc.scratch_bytes(n)) if n <= 1 << 28 else (0, 0)))
    (tmp_path / "cases.txt").write_text("".join(ln + "\n" for ln in lines))
    rows_path = tmp_path / "rows.txt"
    sanitized_program(tmp_path, "find_plan", ["find_plan_main.cpp"], "find_plan OK", env={"FIND_CASES": str(tmp_path / "cases.txt"), "FIND_ROWS": str(rows_path)})
    rows = rows_path.read_text().splitlines()
    assert len(rows) == len(want)
    for i, (got, w) in enumerate(zip(rows, want)):
        assert got == w, (i, lines[i][:160], got, w)
