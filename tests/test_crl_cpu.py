"""The revocation-list library (include/mldsa_crl.h, fips204_amd/crl/libmldsa_crl.so) without a device: its C ABI, how it is linked against
the core, its host helpers and argument checks, its kernels' resources, the builder and the restatement of tests/crl_cases.py against
pinned offsets, openssl and the oracle, and the walks, the placement and the hash as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crl_cases as cc
import x509_cases as xc
from fips204_amd import _crl_lib, _csr_lib, _lib, _mus_lib, _x509_lib, _x509sign_lib
from layer_checks import (ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, sources_clean)
from oracle import oracle as orc

CRL_DIR = os.path.join(ROOT, "fips204_amd", "crl")
SOURCES = ["Makefile", "crl.hip", "crl_plan.h"]
KERNELS = ("k_crl_parse", "k_crl_place_sums", "k_crl_place_offsets", "k_crl_placeEP", "k_crl_entries", "k_crl_link", "k_crl_insert", "k_crl_check")


@pytest.fixture(scope="module")
def lib():
    return built(_crl_lib, CRL_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(lib, tmp_path):
    from fips204_amd import build
    assert build.REVOCATION_LAYERS == {"crl": "libmldsa_crl.so"}
    assert build.CRL_LIB == _crl_lib.LIB_PATH and build.CRL_DIR == CRL_DIR
    # the five older dicts as they were
    assert len(build.LAYERS) == 8 and build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"} and build.PARSE_LAYERS == {"x509": "libmldsa_x509.so"}
    assert build.ISSUE_LAYERS == {"x509sign": "libmldsa_x509sign.so"} and build.REQUEST_LAYERS == {"csr": "libmldsa_csr.so"}
    # crl_plan.h includes the plan headers of two other layers: the shadow links their directories
    (tmp_path / "fips204_amd").mkdir()
    for d in (build.REC_DIR, build.X509_DIR):
        os.symlink(d, tmp_path / "fips204_amd" / os.path.basename(d))
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS, **build.ISSUE_LAYERS,
                                                         **build.REQUEST_LAYERS, **build.REVOCATION_LAYERS}.items()]
    assert libs[-1] == _crl_lib.LIB_PATH and libs[-2] == _csr_lib.LIB_PATH  # built last, behind the request layers
    clean_build("crl", _crl_lib, SOURCES, libs, tmp_path)
    mk = open(os.path.join(CRL_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../x509/x509_plan.h", "../x509/x509_dev.h", "../rec/rec_plan.h", "../rec/rec_wave.h", "../rec/rec_place.h", "crl_plan.h", "mldsa_crl.h",
              "mldsa_x509.h", "mldsa_rec.h"):
        assert h in mk, h  # a change of a shared header rebuilds this library
    assert not re.search(r"-lmldsa_(rec|recsign|x509|x509sign|csr)\b", mk)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_crl_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(lib, tmp_path):
    declared, text = header_and_exports(
        _crl_lib, lib,
        "#include <stddef.h>\n"
        "int main(void) { mldsa_crl_item c; mldsa_crl_fields f; mldsa_crl_entry e; mldsa_crl_totals t; mldsa_rec_op o; mldsa_x509_fields x;\n"
        "  c.issuer = 0; f.reserved[5] = 0; e.reserved[2] = 0; e.serial[19] = 0; t.overflow = 0; o.reserved = 0; x.reserved = 0;\n"
        "  return sizeof(c) == 16 && sizeof(f) == 88 && sizeof(e) == 32 && sizeof(t) == 40 && sizeof(o) == 40 && sizeof(x) == 56\n"
        "    && offsetof(mldsa_crl_fields, tbs_len) == 56 && offsetof(mldsa_crl_fields, first) == 72 && offsetof(mldsa_crl_fields, sig_set) == 80\n"
        "    && offsetof(mldsa_crl_entry, serial_len) == 20 && offsetof(mldsa_crl_entry, crl) == 24 && offsetof(mldsa_crl_entry, off) == 28\n"
        "    && offsetof(mldsa_crl_totals, overflow) == 32 && offsetof(mldsa_crl_item, len) == 8\n"
        "    && mldsa_crl_abi_version() == MLDSA_CRL_ABI_VERSION && MLDSA_CRL_SPACE == 21 && MLDSA_CRL_CHECK_NAMES == MLDSA_X509_CHECK_NAMES\n"
        "    && MLDSA_CRL_NONE > MLDSA_CRL_MAX_CRLS && MLDSA_CRL_SCOPE == 6 && MLDSA_CRL_MAX_CERTS == MLDSA_X509_MAX_CERTS\n"
        "    && !c.issuer && !f.reserved[5] && !e.reserved[2] && !e.serial[19] && !t.overflow && !o.reserved && !x.reserved ? 0 : 1; }\n",
        r"\b(mldsa_crl_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_crl_abi_version", "mldsa_crl_last_error", "mldsa_crl_entries_bound", "mldsa_crl_table_slots",
                        "mldsa_crl_scratch_bytes", "mldsa_crl_parse", "mldsa_crl_ops", "mldsa_crl_table", "mldsa_crl_check"}
    for h in ("mldsa_rec.h", "mldsa_x509.h"):
        assert '#include "%s"' % h in text  # for the types and the codes only
    assert "#define MLDSA_CRL_ABI_VERSION 1" in text and lib.mldsa_crl_abi_version() == _crl_lib.ABI_VERSION == 1
    assert "#define MLDSA_CRL_MAX_CRLS (1u << 30)" in text and _crl_lib.MAX_CRLS == 1 << 30
    assert "#define MLDSA_CRL_MAX_ENTRIES (1u << 30)" in text and _crl_lib.MAX_ENTRIES == 1 << 30 and _crl_lib.MAX_CERTS == _x509_lib.MAX_CERTS
    assert "#define MLDSA_CRL_SCAN_BLOCK 256" in text and _crl_lib.SCAN_BLOCK == 256
    assert "#define MLDSA_CRL_SERIAL_MAX 20" in text and _crl_lib.SERIAL_MAX == cc.SERIAL_MAX == _csr_lib.SERIAL_MAX == 20
    assert "#define MLDSA_CRL_NONE 0xFFFFFFFFu" in text and _crl_lib.NONE == cc.NONE == 0xFFFFFFFF
    assert "#define MLDSA_CRL_CHECK_NAMES 1u" in text and _crl_lib.CHECK_NAMES == cc.CHECK_NAMES == 1
    codes = (("VERSION", 19), ("ENTRY", 20), ("SPACE", 21))
    for name, code in codes:
        assert re.search(r"#define MLDSA_CRL_%s %d\b" % (name, code), text), name
        assert getattr(_crl_lib, name) == getattr(cc, name) == code
    for code, name in enumerate(("GOOD", "REVOKED", "NO_CRL", "CRL_INDEX", "CRL_REFUSED", "CERT", "SCOPE")):
        assert re.search(r"#define MLDSA_CRL_%s %d\b" % (name, code), text), name
        assert getattr(_crl_lib, name) == getattr(cc, name) == code
    # codes 0 ... 6 are the certificate library's; the new ones are disjoint from every code of the x509, x509sign and csr headers (0 ... 18)
    for name in ("OK", "RANGE", "DER", "ALG", "SIG", "ISSUER", "NAME"):
        assert getattr(_crl_lib, name) == getattr(_x509_lib, name) == getattr(cc, name)
    used = set(range(8)) | {_x509sign_lib.ENTRY, _x509sign_lib.KEY, _x509sign_lib.LONG, _x509sign_lib.SPACE} | {
        _csr_lib.VERSION, _csr_lib.KEY, _csr_lib.POP, _csr_lib.ENTRY, _csr_lib.TEMPLATE, _csr_lib.LONG, _csr_lib.SPACE}
    assert used == set(range(19)) and not {c for _, c in codes} & used
    # the layouts
    assert (_crl_lib.ITEM_DTYPE.itemsize, _crl_lib.FIELDS_DTYPE.itemsize, _crl_lib.ENTRY_DTYPE.itemsize, _crl_lib.TOTALS_DTYPE.itemsize) == (16, 88, 32, 40)
    assert [_crl_lib.ITEM_DTYPE.fields[f][1] for f in ("off", "len", "issuer")] == [0, 8, 12]
    names = ("tbs_off", "sig_off", "issuer_off", "this_off", "next_off", "revoked_off", "ext_off", "tbs_len", "issuer_len", "revoked_len",
             "ext_len", "first", "count", "sig_set", "status", "reserved")
    assert [_crl_lib.FIELDS_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72, 76, 80, 81, 82]
    assert [_crl_lib.ENTRY_DTYPE.fields[f][1] for f in ("serial", "serial_len", "reserved", "crl", "off")] == [0, 20, 21, 24, 28]
    assert [_crl_lib.TOTALS_DTYPE.fields[f][1] for f in ("accepted", "refused", "entries", "slots", "overflow", "reserved")] == [0, 8, 16, 24, 32, 36]
    # what is out of scope is said, each item, and a measurement is stated only where its file exists
    for word in ("NOT IN SCOPE", "against a clock", "delta CRLs", "indirect CRLs", "certificateIssuer", "issuingDistributionPoint",
                 "critical extensions", "OCSP", "PEM", "serials longer than 20 bytes", "host-memory, group and batcher", "C++ / Rust mirrors",
                 "walk_crl", "walk_entry", "at most 12 read_tlv steps"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "crl_bench.jsonl")):
        assert "not measured" in text and "Expectation from counts" in text


def test_layered_on_the_one_core_library(lib):
    layered_on_core(_crl_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_sign", "mldsa_verify", "mldsa_verify_pk", "mldsa_keygen", "mldsa_rec_verify", "mldsa_rec_plan", "mldsa_rec_pack",
                           "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops", "mldsa_csr_parse"))
    links_the_core_and_never_builds_it(CRL_DIR)
    dyn = subprocess.run(["readelf", "-d", _crl_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign|x509|x509sign|csr)\.so", dyn)
    no_new_dynamic_symbol(_crl_lib.LIB_PATH, "mldsa_crl_")


def test_kernels_do_not_spill_and_sources_are_clean(lib):
    kernels = [k for k in kernel_resources(CRL_DIR) if "k_crl" in k]
    for stem in KERNELS:
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == len(KERNELS)
    read = dict(sources_clean(CRL_DIR, ["../../include/mldsa_crl.h", "../_crl_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h",
                                        "../rec/rec_place.h", "../x509/x509_dev.h"]))
    src, plan, shared = read["crl.hip"], read["crl_plan.h"], read["../rec/rec_place.h"] + read["../x509/x509_dev.h"]
    certificate_helpers_shared_once("crl")
    for h in ("../layer/layer_host.h", "../layer/layer_dev.h", "../../include/mldsa_crl.h", "../rec/rec_place.h", "../x509/x509_dev.h", "crl_plan.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../x509/x509_plan.h"' in plan
    # no wave waits for another, no host wait; the scaffold and the shared walks are included, not copied
    for word in ("__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "hipStreamSynchronize", "hipMemcpy",
                 "hipMalloc", "hipDeviceSynchronize", "struct DeviceScope", "thread_local", "int fail(", "mldsa_rec_verify(", "mldsa_x509_parse("):
        assert word not in src and word not in plan, word
    for name in ("read_tlv", "oid_set", "names_differ", "name_byte_diff", "in_range", "wave_inclusive", "wave_or"):
        defined = r"^[^\n;=/]*\b(void|bool|int|uint32_t|uint64_t|Tlv)\s+%s\s*\(" % name
        assert not re.search(defined, src + plan, flags=re.M), name
    # the plan has no HIP in it, and the kernels keep no second copy of its rules: they call the plan's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan
    kernel_code = re.sub(r"//[^\n]*", "", src + shared)  # (the placement scan and the link step's comparison are shared with other layers)
    for call in ("walk_crl(", "walk_entry(", "hop(", "load_serial(", "cert_serial(", "hash_serial(", "link_status(", "place_status(", "answer(",
                 "window_at(", "window_chunk(", "window_holds(", "entries_bound(", "name_byte_diff(", "in_range(", "wave_or(", "wave_inclusive("):
        assert call in kernel_code and "constexpr" in plan, call
    for word in ("read_tlv", "0x17", "0x18", "0xA0", "0x02", "0x9E3779B1", "0x85EBCA6B"):  # the rules live in the plan alone
        assert word in plan and word not in kernel_code, word
    # the table is claimed by compare-and-swap, and both probe loops run to table_slots at the most
    assert kernel_code.count("atomicCAS(") == 1 and kernel_code.count("probe < table_slots") == 2


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_never_abort(lib):
    null = None
    buf, p, _ = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    odd2 = C.c_void_p(p.value + 2)
    err = lib.mldsa_crl_last_error

    def parse(ctx=null, blob=p, blob_len=1024, crls=p, n=4, fields=p, stream=null):
        return lib.mldsa_crl_parse(ctx, blob, blob_len, crls, n, fields, stream)

    def ops(ctx=null, blob=p, blob_len=1024, crls=p, n=4, cert_fields=p, n_certs=2, flags=1, fields=p, entries=p, max_entries=8, ops=p, status=p,
            totals=p, scratch=p, scratch_bytes=256, stream=null):
        return lib.mldsa_crl_ops(ctx, blob, blob_len, crls, n, cert_fields, n_certs, flags, fields, entries, max_entries, ops, status, totals,
                                 scratch, scratch_bytes, stream)

    def table(ctx=null, entries=p, max_entries=8, table=p, slots=64, totals=p, stream=null):
        return lib.mldsa_crl_table(ctx, entries, max_entries, table, slots, totals, stream)

    def check(ctx=null, blob=p, blob_len=1024, certs=p, cert_fields=p, cert_crl=p, n_certs=2, crls=p, fields=p, crl_status=p, crl_ok=null, n=4,
              entries=p, max_entries=8, table=p, slots=64, revocation=p, stream=null):
        return lib.mldsa_crl_check(ctx, blob, blob_len, certs, cert_fields, cert_crl, n_certs, crls, fields, crl_status, crl_ok, n, entries,
                                   max_entries, table, slots, revocation, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (parse, ops, table, check):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    fake = p  # a fake non-NULL context must still be refused before it is touched
    for call in (parse, ops, check):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, crls=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, crls=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, fields=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n=_crl_lib.MAX_CRLS + 1) == _lib.ERR_PARAM and b"MLDSA_CRL_MAX_CRLS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_CRL_MAX_CRLS" in err()
    for call in (ops, check):
        assert call(ctx=fake, cert_fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, cert_fields=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n_certs=_crl_lib.MAX_CERTS + 1) == _lib.ERR_PARAM and b"MLDSA_CRL_MAX_CERTS" in err()
    for call in (ops, table, check):
        assert call(ctx=fake, entries=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, entries=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, max_entries=_crl_lib.MAX_ENTRIES + 1) == _lib.ERR_PARAM and b"MLDSA_CRL_MAX_ENTRIES" in err()
    for name in ("ops", "status", "totals"):
        assert ops(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
    for name in ("ops", "totals"):
        assert ops(ctx=fake, **{name: odd4}) == _lib.ERR_PARAM and b"8-byte aligned" in err(), name
    for flags in (2, 3, 0x80000000):
        assert ops(ctx=fake, flags=flags) == _lib.ERR_PARAM and b"unknown flag" in err(), flags
    assert ops(ctx=fake, scratch=null) == _lib.ERR_PARAM and b"mldsa_crl_scratch_bytes" in err()
    assert ops(ctx=fake, scratch=C.c_void_p(p.value + 128)) == _lib.ERR_PARAM and b"256-byte aligned" in err()
    assert ops(ctx=fake, scratch_bytes=lib.mldsa_crl_scratch_bytes(4) - 1) == _lib.ERR_PARAM and b"smaller than" in err()
    for call in (table, check):
        assert call(ctx=fake, table=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, table=odd2) == _lib.ERR_PARAM and b"4-byte aligned" in err()
        for slots in (0, 32, 63, 65, 96, 2 ** 32):
            assert call(ctx=fake, slots=slots) == _lib.ERR_PARAM and b"table_slots must be a power of two" in err(), slots
        assert call(ctx=fake, max_entries=33, slots=64) == _lib.ERR_PARAM and b"at least mldsa_crl_table_slots" in err()
    assert table(ctx=fake, totals=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert table(ctx=fake, totals=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
    for name in ("certs", "cert_crl", "revocation", "crl_status"):
        assert check(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
    assert check(ctx=fake, certs=odd4) == _lib.ERR_PARAM and b"certs must be 8-byte aligned" in err()
    assert check(ctx=fake, cert_crl=odd2) == _lib.ERR_PARAM and b"cert_crl must be 4-byte aligned" in err()
    # a NULL blob is an empty blob's, an empty table of entries or certificates needs no pointer: the checks go on to the next one
    assert parse(ctx=fake, blob=null, blob_len=0, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert ops(ctx=null, entries=null, max_entries=0, cert_fields=null, n_certs=0) == _lib.ERR_PARAM and b"NULL context" in err()
    # empty calls succeed without a context, and touch nothing
    assert parse(n=0, blob=null, crls=null, fields=null) == _lib.OK
    assert ops(n=0, blob=null, crls=null, cert_fields=null, fields=null, entries=null, ops=null, status=null, totals=null, scratch=null,
               scratch_bytes=0, flags=99) == _lib.OK
    assert check(n_certs=0, blob=null, certs=null, cert_fields=null, cert_crl=null, crls=null, fields=null, crl_status=null, entries=null,
                 table=null, revocation=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(lib):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert lib.mldsa_crl_table(p, p, 8, p, 48, p, null) == _lib.ERR_PARAM
    mine = lib.mldsa_crl_last_error()
    assert mine == b"mldsa_crl_table: table_slots must be a power of two, at least mldsa_crl_table_slots and at most 2^31"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert lib.mldsa_crl_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _crl_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "walk_crl", "k_crl", "wave_inclusive"):
        assert word not in exported, word
    del buf


def test_host_helpers_against_the_restatement(lib):
    for n in (0, 1, 19, 20, 21, 39, 40, 1000, 2 ** 32, 2 ** 40 + 7):
        assert lib.mldsa_crl_entries_bound(n) == n // cc.ENTRY_MIN
    last = 0
    for n in (0, 1, 31, 32, 33, 64, 65, 128, 129, 1000, 65536, 65537, 1 << 30):
        got = lib.mldsa_crl_table_slots(n)
        assert got == cc.table_slots(n) and got >= max(64, 2 * n) and got & (got - 1) == 0 and got >= last and (got == 64 or got < 4 * n), n
        last = got
    for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
        assert lib.mldsa_crl_table_slots(n) == 0 and cc.table_slots(n) == 0
    last = 0
    for n in (0, 1, 255, 256, 257, 8192, 8193, 65536, 1 << 30):
        got = lib.mldsa_crl_scratch_bytes(n)
        assert got == (8 * ((n + 255) // 256) + 255) // 256 * 256 and got >= last
        last = got
    for n in ((1 << 30) + 1, 2 ** 64 - 1):
        assert lib.mldsa_crl_scratch_bytes(n) == 0
    # the smallest entry the builder can make is the bound's 20 bytes
    assert len(cc.entry(b"\x01")) == cc.ENTRY_MIN and cc.walk_entry(cc.entry(b"\x01"), 0, 20) == (20, b"\x01")


# ---- the builder and the restatement ------------------------------------------------------------------------------------------------
def plain(pset, count=3, **kw):
    return cc.random_parts(pset, b"root", b"plain", pset, count, **kw)


@pytest.mark.parametrize("pset,total", [(44, 2639), (65, 3531), (87, 4835)])
def test_valid_crls_have_the_pinned_offsets(pset, total):
    p = plain(pset)
    der = cc.join(p)
    assert len(der) == total
    w = cc.walk_crl(der)
    assert (w["status"], w["tbs_off"], w["issuer_off"], w["issuer_len"], w["this_off"], w["next_off"], w["sig_set"]) == (0, 4, 23, 17, 40, 55, pset)
    assert w["revoked_off"] == 74 and w["revoked_len"] == sum(len(e) for e in p["entries"]) and w["sig_off"] == total - cc.SIG_LEN[pset]
    assert der[w["issuer_off"]:w["issuer_off"] + w["issuer_len"]] == xc.name(b"root") and der[w["this_off"]:w["this_off"] + 15] == cc.UTC
    assert der[w["next_off"]:w["next_off"] + 17] == cc.GENERALIZED and der[w["ext_off"]:w["ext_off"] + w["ext_len"]] == cc.crl_number()
    assert der[w["tbs_off"]:w["tbs_off"] + w["tbs_len"]] == cc.tbs_of(p)
    rows = cc.list_entries(der, w)
    assert [s for s, _ in rows] == [cc.serial_of(b"plain", pset, k) for k in range(3)] and rows[0][1] == 74
    assert [der[at:at + len(e)] for (_, at), e in zip(rows, p["entries"])] == p["entries"]
    # every optional field can be absent: v1 without extensions, no nextUpdate, no list
    for kw in (dict(v2=False), dict(next_update=False), dict(ext=None), dict(v2=False, next_update=False)):
        for count in (0, 2):
            d = cc.join(plain(pset, count, **kw))
            w = cc.walk_crl(d)
            assert w["status"] == 0 and (w["next_off"] != 0) == kw.get("next_update", True) and (w["revoked_len"] != 0) == (count != 0), (kw, count)
            assert (w["ext_len"] != 0) == (kw.get("v2", True) and "ext" not in kw)


@pytest.mark.parametrize("defect", list(cc.DEFECTS))
def test_every_defect_gives_its_documented_status(defect):
    cas = cc.ca_certs()
    for k, pset in enumerate(cc.SETS):
        good = cc.random_parts(pset, cc.CA_CN[pset], b"defect", pset, 3 + k)
        der = cc.join(good)
        blob, certs, items, cert_fields = cc.lay_out(cas, [0, 1, 2], [(der, len(der)), cc.make_defect(good, defect), (der, len(der))], [k, k, k],
                                                     pad=[2, 9, 4], front=1)
        fields, entries, ops, status, totals = cc.expected(blob, items, cert_fields, cc.max_entries_of(items))
        want = cc.DEFECTS[defect]
        assert status.tolist() == [0, want, 0], (defect, pset, status.tolist())
        assert int(fields[1]["status"]) == want and ops[1].tobytes() == bytes(40) and ops[0]["set"] == ops[2]["set"] == pset
        assert int(fields[1]["count"]) == 0 and int(fields[0]["count"]) == int(fields[2]["count"]) == 3 + k
        if want == cc.DER:
            assert fields[1].tobytes() == bytes(81) + bytes([cc.DER]) + bytes(6)
        assert not any(int(e["crl"]) == 1 for e in entries if e["serial_len"])  # a refused CRL lists nobody
        assert (int(totals[0]["accepted"]), int(totals[0]["refused"]), int(totals[0]["entries"])) == (2, 1, 2 * (3 + k))


def test_range_rule_and_precedence():
    cas = cc.ca_certs()
    good = cc.random_parts(44, cc.CA_CN[44], b"prec", 0, 4)
    der = cc.join(good)

    def status_of(*defects, issuer=0, length=None, off=None, flags=cc.CHECK_NAMES, max_entries=None):
        p, data, n = good, der, len(der)
        for d in defects:
            data, n = cc.make_defect(p, d)
        blob, certs, items, cert_fields = cc.lay_out(cas, [0, 1, 2], [(data, n if length is None else length)], [issuer])
        if off is not None:
            items[0]["off"] = off if off >= 0 else blob.size + off
        return int(cc.expected(blob, items, cert_fields, cc.max_entries_of(items) if max_entries is None else max_entries, flags)[3][0])

    assert status_of() == cc.OK
    for length, off in ((0, None), (1, None), (2, -1), (len(der), 2 ** 64 - 1), (2 ** 32 - 1, None), (len(der), 1 - len(der))):
        assert status_of(length=length, off=off) == cc.RANGE, (length, off)
    assert status_of(length=2, off=-3) == cc.DER                                       # inside the blob, and malformed
    assert status_of("wrong_tag_issuer", length=1) == cc.RANGE                         # RANGE before DER
    for d in ("sig_one_short", "version_v1", "empty_revoked", "serial_len_0"):
        assert status_of(d) == cc.DEFECTS[d]
    # two defects: the parts carry one defect at a time, so the order is pinned through crafted parts
    p = dict(good, version=cc.tlv(0x02, b"\x00"), sig_bits=good["sig_bits"][:-1])
    assert cc.walk_crl(cc.join(p))["status"] == cc.SIG                                 # SIG before VERSION
    p = dict(good, outer=xc.alg_id(65), sig_bits=good["sig_bits"][:-1])
    assert cc.walk_crl(cc.join(p))["status"] == cc.ALG                                 # ALG before SIG
    p = dict(good, version=b"", entries=[])
    assert cc.walk_crl(cc.join(p))["status"] == cc.VERSION                             # VERSION before ENTRY
    p = dict(good, outer=xc.alg_id(65), tbs_extra=b"\x05\x00")
    assert cc.walk_crl(cc.join(p))["status"] == cc.DER                                 # DER before ALG
    assert status_of("serial_len_21", issuer=7) == cc.ENTRY and status_of(issuer=7) == cc.ISSUER   # ENTRY before ISSUER
    assert status_of(issuer=1) == cc.ISSUER and status_of(issuer=2 ** 32 - 1) == cc.ISSUER          # cross-set; out of range by far
    assert status_of(max_entries=0) == cc.SPACE and status_of("serial_len_21", max_entries=0) == cc.SPACE  # SPACE before ENTRY
    assert status_of(max_entries=0, issuer=7) == cc.SPACE                                                  # ... and before ISSUER
    # NAME: the CRL names another issuer than the CA's subject
    other = cc.join(cc.random_parts(44, b"someone else", b"prec", 1, 2))
    blob, certs, items, cert_fields = cc.lay_out(cas, [0, 1, 2], [(other, len(other))], [0])
    assert cc.expected(blob, items, cert_fields, 8)[3].tolist() == [cc.NAME] and cc.expected(blob, items, cert_fields, 8, 0)[3].tolist() == [0]
    f, e, o, s, t = cc.expected(blob, items, cert_fields, 8)
    assert not e["serial_len"].any() and int(f[0]["count"]) == 0 and int(t[0]["slots"]) == int(f[0]["revoked_len"]) // 20 >= 2 and int(t[0]["entries"]) == 0


def test_placement_and_lookup_of_the_restatement():
    cas = cc.ca_certs()
    crls = [cc.random_crl(44, cc.CA_CN[44], b"place", i, count) for i, count in enumerate((3, 0, 5, 1))]
    bounds = [cc.walk_crl(d)["revoked_len"] // 20 for d in crls]
    assert bounds[1] == 0 and all(b >= c for b, c in zip(bounds, (3, 0, 5, 1)))
    leaves = [cc.cert_with_serial(44, 44, cc.CA_CN[44], b"leaf%d" % k, cc.serial_of(b"place", 2, k), b"leaf", k) for k in range(5)]
    leaves.append(cc.cert_with_serial(44, 44, cc.CA_CN[44], b"free", b"\x42\x42", b"leaf", 9))
    blob, certs, items, cert_fields = cc.lay_out(cas + leaves, [0, 1, 2] + [0] * 6, [(d, len(d)) for d in crls], [0] * 4, pad=5)
    total = sum(bounds)
    f, e, o, s, t = cc.expected(blob, items, cert_fields, total)
    assert s.tolist() == [0, 0, 0, 0] and f["first"].tolist() == [0, bounds[0], bounds[0], bounds[0] + bounds[2]] and f["count"].tolist() == [3, 0, 5, 1]
    assert (int(t[0]["accepted"]), int(t[0]["entries"]), int(t[0]["slots"])) == (4, 9, total)
    assert [int(x) for x in e["crl"][e["serial_len"] != 0]] == [0] * 3 + [2] * 5 + [3]
    # one slot short: the last CRL that has a list does not fit, the ones in front keep their slots
    f1, e1, _, s1, t1 = cc.expected(blob, items, cert_fields, total - 1)
    assert s1.tolist() == [0, 0, 0, cc.SPACE] and np.array_equal(e1, e[:total - 1]) and int(f1[3]["count"]) == 0
    assert int(t1[0]["slots"]) == total - bounds[3] and f1["first"].tolist()[:3] == f["first"].tolist()[:3]
    # first_i + bound_i > max_entries: a CRL without a list is SPACE too where its (empty) range begins behind the table's end
    assert cc.expected(blob, items, cert_fields, 0)[3].tolist() == [cc.SPACE] * 4
    assert cc.expected(blob, items[1:2], cert_fields, 0)[3].tolist() == [0]
    # the lookup: CRL 2 lists the five leaves; under CRL 0 the same certificates are good; the free one is good under both
    n = len(certs)
    cover = np.array([cc.NONE] * 3 + [2] * 6, dtype=np.uint32)
    got = cc.expected_check(blob, certs, cert_fields, cover, items, f, s, None, e)
    assert got.tolist() == [cc.NO_CRL] * 3 + [cc.REVOKED] * 5 + [cc.GOOD]
    cover[3:] = 0
    assert cc.expected_check(blob, certs, cert_fields, cover, items, f, s, None, e).tolist()[3:] == [cc.GOOD] * 6
    cover[3], cover[4] = 4, 2 ** 32 - 2
    ok = np.array([1, 1, 0, 1], dtype=np.uint8)
    cover[5:] = 2
    assert cc.expected_check(blob, certs, cert_fields, cover, items, f, s, ok, e).tolist()[3:] == [cc.CRL_INDEX] * 2 + [cc.CRL_REFUSED] * 4
    assert n == 9 and cc.table_is_sound(np.zeros(64, dtype=np.uint32), np.zeros(3, dtype=_crl_lib.ENTRY_DTYPE))


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the CRLs independently")
def test_builder_agrees_with_openssl_crl(tmp_path):
    for pset, count, kw in ((44, 0, {}), (44, 5, {}), (65, 70, dict(next_update=False)), (87, 3, dict(v2=False))):
        p = cc.random_parts(pset, b"openssl ca", b"ossl", pset, count, **kw)
        path = tmp_path / "c.der"
        path.write_bytes(cc.join(p))
        run = subprocess.run(["openssl", "crl", "-inform", "DER", "-noout", "-text", "-in", str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        serials = [ln.split(":", 1)[1].strip().lower() for ln in run.stdout.splitlines() if ln.strip().startswith("Serial Number:")]
        want = []
        for k in range(count):  # openssl prints the magnitude in hex, a minus sign in front of a negative serial
            v = int.from_bytes(cc.serial_of(b"ossl", pset, k), "big", signed=True)
            want.append(("-" if v < 0 else "") + ("%X" % abs(v)).rjust(2 * ((len("%X" % abs(v)) + 1) // 2), "0").lower())
        assert [s.lstrip("-").lstrip("0") or "0" for s in serials] == [s.lstrip("-").lstrip("0") or "0" for s in want], (pset, count)
        assert [s.startswith("-") for s in serials] == [s.startswith("-") for s in want]
        assert ("Next Update" in run.stdout and "NONE" not in run.stdout.split("Next Update")[1][:12]) == kw.get("next_update", True)
        assert "Version %d" % (2 if kw.get("v2", True) else 1) in run.stdout and "openssl ca" in run.stdout


def test_a_crl_signed_and_verified_with_the_oracle():
    pset = 44
    pk, sk = orc.keygen_from_seed(pset, xc._bytes(b"crl-ca", 0, 32))
    ca = xc.cert(xc.tbs(pset, pset, b"oracle ca", b"oracle ca", orc.pk_into_bytes(pset, pk)), pset, bytes(xc.SIG_LEN[pset]))
    p = cc.parts(pset, b"oracle ca", cc.random_entries(b"orc", 0, 4), bytes(xc.SIG_LEN[pset]))
    sig = orc.sign_internal(pset, sk, cc.tbs_of(p), xc._bytes(b"crl-rnd", 0, 32), ctx=b"", mode=orc.MODE_PURE)
    p["sig_bits"] = b"\x00" + sig
    der = cc.join(p)
    blob, certs, items, cert_fields = cc.lay_out([ca], [0], [(der, len(der))], [0], pad=3)
    f, e, ops, status, _ = cc.expected(blob, items, cert_fields, 8)
    assert status.tolist() == [0] and int(f[0]["count"]) == 4
    raw, op = blob.tobytes(), ops[0]
    cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
    assert cut(op["msg_off"], op["msg_len"]) == cc.tbs_of(p) and cut(op["sig_off"], xc.SIG_LEN[pset]) == sig
    verify = lambda data: bool(orc.verify_internal(pset, orc.pk_try_from_bytes(pset, cut(op["pk_off"], xc.PK_LEN[pset])),  # noqa: E731
                                                   data, cut(op["sig_off"], xc.SIG_LEN[pset]), ctx=b"", mode=orc.MODE_PURE))
    assert verify(cut(op["msg_off"], op["msg_len"]))
    tampered = bytearray(cut(op["msg_off"], op["msg_len"]))
    tampered[int(e[1]["off"]) - 4 + 5] ^= 1  # a serial byte of the second entry (offsets are the CRL's, the TBS begins 4 bytes in)
    assert not verify(bytes(tampered))


# ---- the walks under the sanitizers --------------------------------------------------------------------------------------------------
def test_the_walks_the_hash_and_the_placement_under_asan_and_ubsan(tmp_path):
    cases = []
    for k, pset in enumerate(cc.SETS):
        good = cc.random_parts(pset, b"root", b"san", pset, 5 + k)
        cases.append(cc.join(good))
        for defect in cc.DEFECTS:
            data, n = cc.make_defect(good, defect)
            cases.append((data + b"\xC3")[:n])
    for count, kw in ((0, {}), (1, dict(v2=False)), (65, dict(next_update=False)), (130, {}), (2, dict(ext=None))):
        cases.append(cc.random_crl(44, b"root", b"san2", count, count, **kw))
    long_ext = cc.parts(44, b"root", [cc.entry(b"\x01"), cc.entry(b"\x02\x03", ext=cc.tlv(0x30, bytes(1500))), cc.entry(b"\x80")], bytes(2420))
    cases.append(cc.join(long_ext))
    # single-byte mutants: the first 130 bytes, and one whole entry in the middle of a 65-entry list
    base = cc.random_parts(44, b"root", b"mut", 0, 65)
    der = cc.join(base)
    mid = cc.list_entries(der, cc.walk_crl(der))[32][1]
    for pos in list(range(xc.MUTATION_SPAN)) + list(range(mid, mid + len(base["entries"][32]))):
        for v in xc.MUTATION_VALUES:
            cases.append(der[:pos] + bytes([v]) + der[pos + 1:])
    (tmp_path / "cases.txt").write_text("".join(c.hex() + "\n" for c in cases))
    rows_path = tmp_path / "rows.txt"
    sanitized_program(tmp_path, "crl_plan", ["crl_plan_main.cpp"], "crl_plan OK", env={"CRL_CASES": str(tmp_path / "cases.txt"), "CRL_ROWS": str(rows_path)})
    rows = rows_path.read_text().splitlines()
    assert len(rows) == len(cases)
    seen = set()
    for i, (der, row) in enumerate(zip(cases, rows)):
        w = cc.walk_crl(der)
        found = cc.list_entries(der, w) if w["status"] == cc.OK else []
        status = w["status"] if found is not None else cc.ENTRY
        want = [status] + [w[f] for f in ("tbs_off", "tbs_len", "sig_off", "issuer_off", "issuer_len", "this_off", "next_off", "revoked_off",
                                         "revoked_len", "ext_off", "ext_len", "sig_set")] + [len(found or [])]
        got = row.split()
        assert [int(x) for x in got[:14]] == want, (i, row[:200], want)
        assert got[14:] == ["%s@%d#%08x" % (s.hex(), at, cc.hash_serial(i, s)) for s, at in (found or [])], i
        seen.add(status)
    assert seen == {cc.OK, cc.DER, cc.ALG, cc.SIG, cc.VERSION, cc.ENTRY}
