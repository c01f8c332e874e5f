"""The path-validation library (include/mldsa_path.h, fips204_amd/path/libmldsa_path.so) without a device: its C ABI, how it is linked
against the core, its host helper and argument checks, its kernels' resources, the restatement of tests/path_cases.py against
calendar.timegm, pinned offsets and openssl, and the Time reader, the walk and the climb as a stand-alone program under the sanitizers."""
import calendar
import ctypes as C
import datetime
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import path_cases as pc
import x509_cases as xc
from fips204_amd import _crl_lib, _csr_lib, _lib, _mus_lib, _path_lib, _x509_lib, _x509sign_lib
from layer_checks import (ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program, sources_clean)

PATH_DIR = os.path.join(ROOT, "fips204_amd", "path")
SOURCES = ["Makefile", "path.hip", "path_plan.h"]
KERNELS = ("k_path_times", "k_path_parse", "k_path_crl_times", "k_path_node", "k_path_climb")


@pytest.fixture(scope="module")
def lib():
    return built(_path_lib, PATH_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(lib, tmp_path):
    from fips204_amd import build
    assert build.PATH_LAYERS == {"path": "libmldsa_path.so"}
    assert build.PATH_LIB == _path_lib.LIB_PATH and build.PATH_DIR == PATH_DIR
    # the seven older dicts as they were
    assert len(build.LAYERS) == 8 and build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"} and build.PARSE_LAYERS == {"x509": "libmldsa_x509.so"}
    assert build.ISSUE_LAYERS == {"x509sign": "libmldsa_x509sign.so"} and build.REQUEST_LAYERS == {"csr": "libmldsa_csr.so"}
    assert build.REVOCATION_LAYERS == {"crl": "libmldsa_crl.so"}
    # path_plan.h includes the plan headers of two other layers: the shadow links their directories
    (tmp_path / "fips204_amd").mkdir()
    for d in (build.REC_DIR, build.X509_DIR):
        os.symlink(d, tmp_path / "fips204_amd" / os.path.basename(d))
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS, **build.ISSUE_LAYERS,
                                                         **build.REQUEST_LAYERS, **build.REVOCATION_LAYERS, **build.PATH_LAYERS}.items()]
    assert libs[-1] == _path_lib.LIB_PATH and libs[-2] == _crl_lib.LIB_PATH  # built last, behind the revocation layers
    clean_build("path", _path_lib, SOURCES, libs, tmp_path)
    mk = open(os.path.join(PATH_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../x509/x509_plan.h", "../x509/x509_dev.h", "../rec/rec_plan.h", "path_plan.h", "mldsa_path.h", "mldsa_crl.h", "mldsa_x509.h", "mldsa_rec.h"):
        assert h in mk, h  # a change of a shared header rebuilds this library
    assert not re.search(r"-lmldsa_(rec|recsign|x509|x509sign|csr|crl)\b", mk)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_path_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(lib, tmp_path):
    declared, text = header_and_exports(
        _path_lib, lib,
        "#include <stddef.h>\n"
        "int main(void) { mldsa_path_fields f; mldsa_path_result r; mldsa_x509_cert c; mldsa_crl_fields l;\n"
        "  f.reserved[2] = 0; r.reserved[1] = 0; c.issuer = 0; l.reserved[5] = 0;\n"
        "  return sizeof(f) == 48 && sizeof(r) == 8 && sizeof(c) == 16 && sizeof(l) == 88\n"
        "    && offsetof(mldsa_path_fields, not_after) == 8 && offsetof(mldsa_path_fields, ext_off) == 16\n"
        "    && offsetof(mldsa_path_fields, crit_off) == 24 && offsetof(mldsa_path_fields, ext_len) == 32\n"
        "    && offsetof(mldsa_path_fields, path_len) == 36 && offsetof(mldsa_path_fields, key_usage) == 40\n"
        "    && offsetof(mldsa_path_fields, flags) == 42 && offsetof(mldsa_path_fields, n_ext) == 43 && offsetof(mldsa_path_fields, status) == 44\n"
        "    && offsetof(mldsa_path_result, verdict) == 4 && offsetof(mldsa_path_result, depth) == 5\n"
        "    && mldsa_path_abi_version() == MLDSA_PATH_ABI_VERSION && MLDSA_PATH_CRITICAL == 25 && MLDSA_PATH_VERSION > MLDSA_CRL_SPACE\n"
        "    && MLDSA_PATH_MAX_CERTS == MLDSA_X509_MAX_CERTS && MLDSA_PATH_NO_PATH_LEN > MLDSA_PATH_MAX_CERTS && MLDSA_PATH_DEPTH == 12\n"
        "    && !f.reserved[2] && !r.reserved[1] && !c.issuer && !l.reserved[5] ? 0 : 1; }\n",
        r"\b(mldsa_path_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_path_abi_version", "mldsa_path_last_error", "mldsa_path_scratch_bytes", "mldsa_path_times", "mldsa_path_parse",
                        "mldsa_path_crl_times", "mldsa_path_chain"}
    for h in ("mldsa_rec.h", "mldsa_x509.h", "mldsa_crl.h"):
        assert '#include "%s"' % h in text  # for the types and the codes only
    assert "#define MLDSA_PATH_ABI_VERSION 1" in text and lib.mldsa_path_abi_version() == _path_lib.ABI_VERSION == 1
    assert "#define MLDSA_PATH_MAX_CERTS MLDSA_X509_MAX_CERTS" in text and _path_lib.MAX_CERTS == _x509_lib.MAX_CERTS
    assert "#define MLDSA_PATH_MAX_EXTS 32" in text and _path_lib.MAX_EXTS == pc.MAX_EXTS == 32
    assert "#define MLDSA_PATH_MAX_DEPTH 16" in text and _path_lib.MAX_DEPTH == pc.MAX_DEPTH == 16
    assert "#define MLDSA_PATH_NO_PATH_LEN 0xFFFFFFFFu" in text and _path_lib.NO_PATH_LEN == pc.NO_PATH_LEN == 0xFFFFFFFF
    for name, bit in (("ALLOW_UNKNOWN_CRITICAL", 1), ("REQUIRE_NEXT_UPDATE", 2), ("ALLOW_NO_CRL", 4), ("V3", 1), ("HAS_BC", 2), ("IS_CA", 4), ("HAS_KU", 8)):
        assert re.search(r"#define MLDSA_PATH_%s %du\b" % (name, bit), text), name
        assert getattr(_path_lib, name) == getattr(pc, name) == bit
    codes = (("VERSION", 22), ("TIME", 23), ("EXT", 24), ("CRITICAL", 25))
    for name, code in codes:
        assert re.search(r"#define MLDSA_PATH_%s %d\b" % (name, code), text), name
        assert getattr(_path_lib, name) == getattr(pc, name) == code
    for code, name in enumerate(("TRUSTED", "CERT", "SIG", "POLICY", "NOT_YET", "EXPIRED", "REVOKED", "REVOCATION", "NOT_CA", "KEY_USAGE", "PATH_LEN",
                                 "NO_ANCHOR", "DEPTH")):
        assert re.search(r"#define MLDSA_PATH_%s %d\b" % (name, code), text), name
        assert getattr(_path_lib, name) == getattr(pc, name) == code
    for code, name in enumerate(("CRL_FRESH", "CRL_REFUSED", "CRL_TIME", "CRL_NOT_YET", "CRL_STALE")):
        assert re.search(r"#define MLDSA_PATH_%s %d\b" % (name, code), text), name
        assert getattr(_path_lib, name) == getattr(pc, name) == code
    # codes 0 ... 2 are the certificate library's; the new ones are disjoint from every code of the x509, x509sign, csr and crl headers (0 ... 21)
    for name in ("OK", "RANGE", "DER"):
        assert getattr(_path_lib, name) == getattr(_x509_lib, name) == getattr(pc, name)
    used = set(range(8)) | {_x509sign_lib.ENTRY, _x509sign_lib.KEY, _x509sign_lib.LONG, _x509sign_lib.SPACE} | {
        _csr_lib.VERSION, _csr_lib.KEY, _csr_lib.POP, _csr_lib.ENTRY, _csr_lib.TEMPLATE, _csr_lib.LONG, _csr_lib.SPACE} | {
        _crl_lib.VERSION, _crl_lib.ENTRY, _crl_lib.SPACE}
    assert used == set(range(22)) and not {c for _, c in codes} & used
    assert (pc.REV_GOOD, pc.REV_REVOKED, pc.REV_NO_CRL) == (_crl_lib.GOOD, _crl_lib.REVOKED, _crl_lib.NO_CRL) and pc.NO_ISSUER == _x509_lib.NO_ISSUER
    # the layouts
    assert (_path_lib.FIELDS_DTYPE.itemsize, _path_lib.RESULT_DTYPE.itemsize, _path_lib.NODE_DTYPE.itemsize) == (48, 8, 8)
    names = ("not_before", "not_after", "ext_off", "crit_off", "ext_len", "path_len", "key_usage", "flags", "n_ext", "status", "reserved")
    assert [_path_lib.FIELDS_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 36, 40, 42, 43, 44, 45]
    assert [_path_lib.RESULT_DTYPE.fields[f][1] for f in ("where", "verdict", "depth", "reserved")] == [0, 4, 5, 6]
    assert [_path_lib.NODE_DTYPE.fields[f][1] for f in ("issuer", "own", "as_issuer", "path_len", "anchor")] == [0, 4, 5, 6, 7]
    # what is out of scope is said, each item, and a measurement is stated only where its file exists
    for word in ("NOT IN SCOPE", "self-issued certificates are not exempt from pathLen", "name and policy constraints", "extended key usage", "AKI / SKI",
                 "cRLSign on CRL issuers", "delta and indirect CRLs", "PEM", "before 2050 use UTCTime is not enforced", "host-memory, group and batcher",
                 "C++ / Rust mirrors", "parse_time", "walk_policy", "k_path_node", "k_path_climb", "RANGE, DER, VERSION, TIME, EXT, CRITICAL"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "path_bench.jsonl")):
        assert "not measured" in text and "from counts (an expectation)" in text


def test_layered_on_the_one_core_library(lib):
    layered_on_core(_path_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_sign", "mldsa_verify", "mldsa_verify_pk", "mldsa_keygen", "mldsa_rec_verify", "mldsa_rec_plan", "mldsa_rec_pack",
                           "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops", "mldsa_csr_parse", "mldsa_crl_parse", "mldsa_crl_ops",
                           "mldsa_crl_table", "mldsa_crl_check"))
    links_the_core_and_never_builds_it(PATH_DIR)
    dyn = subprocess.run(["readelf", "-d", _path_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign|x509|x509sign|csr|crl)\.so", dyn)
    no_new_dynamic_symbol(_path_lib.LIB_PATH, "mldsa_path_")


def test_kernels_do_not_spill_and_sources_are_clean(lib):
    kernels = [k for k in kernel_resources(PATH_DIR, lds_zero=True) if "k_path" in k]
    for stem in KERNELS:
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == len(KERNELS)
    read = dict(sources_clean(PATH_DIR, ["../../include/mldsa_path.h", "../_path_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]))
    src, plan = read["path.hip"], read["path_plan.h"]
    certificate_helpers_shared_once("path")
    for h in ("../layer/layer_host.h", "../layer/layer_dev.h", "../x509/x509_dev.h", "../../include/mldsa_path.h", "path_plan.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../x509/x509_plan.h"' in plan and '#include "../rec/rec_plan.h"' in open(os.path.join(PATH_DIR, "..", "x509", "x509_plan.h")).read()
    # no wave waits for another, no host wait, no allocation; the scaffold and the shared readers are included, not copied
    for word in ("__threadfence", "__syncthreads", "__shared__", "atomic", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate",
                 "hipStreamSynchronize", "hipMemcpy", "hipMalloc", "hipDeviceSynchronize", "struct DeviceScope", "thread_local", "int fail(",
                 "mldsa_rec_verify(", "mldsa_x509_parse(", "mldsa_crl_check("):
        assert word not in src and word not in plan, word
    for name in ("read_tlv", "oid_set", "in_range", "wave_or", "wave_max", "walk"):
        defined = r"^[^\n;=/]*\b(void|bool|int|uint32_t|uint64_t|Tlv|Walk)\s+%s\s*\(" % name
        assert not re.search(defined, src + plan, flags=re.M), name
    # the plan has no HIP in it, and the kernels keep no second copy of its rules: they call the plan's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan
    kernel_code = re.sub(r"//[^\n]*", "", src)
    for call in ("parse_time(", "walk_policy(", "own_rule(", "issuer_rule(", "node_of(", "pack_node(", "climb(", "crl_time_status(", "in_range(",
                 "scratch_bytes("):
        assert call in kernel_code and "constexpr" in plan, call
    for word in ("read_tlv", "0x17", "0x18", "0xA3", "0x81", "0x1D", "0x5A", "146097", "86400"):  # the rules live in the plan alone
        assert word in plan and word not in kernel_code, word
    # no table indexed by data: the plan holds no array at all; both loops run to a constant
    assert not re.search(r"\[\s*\w*\s*\]\s*=\s*\{", code) and "k < MAX_EXTS" in code and "k <= MAX_DEPTH" in code


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_never_abort(lib):
    null = None
    buf, p, _ = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    err = lib.mldsa_path_last_error

    def times(ctx=null, blob=p, blob_len=1024, offs=p, n=4, seconds=p, status=p, stream=null):
        return lib.mldsa_path_times(ctx, blob, blob_len, offs, n, seconds, status, stream)

    def parse(ctx=null, blob=p, blob_len=1024, certs=p, n=4, flags=0, fields=p, stream=null):
        return lib.mldsa_path_parse(ctx, blob, blob_len, certs, n, flags, fields, stream)

    def crl_times(ctx=null, blob=p, blob_len=1024, crl_fields=p, crl_status=p, crl_ok=null, n=4, now=0, flags=0, this_s=p, next_s=p, time_status=p,
                  fresh_ok=p, stream=null):
        return lib.mldsa_path_crl_times(ctx, blob, blob_len, crl_fields, crl_status, crl_ok, n, now, flags, this_s, next_s, time_status, fresh_ok, stream)

    def chain(ctx=null, certs=p, policy=p, cert_status=p, cert_ok=p, revocation=null, anchor=p, n=4, now=0, flags=0, results=p, scratch=p,
              scratch_bytes=256, stream=null):
        return lib.mldsa_path_chain(ctx, certs, policy, cert_status, cert_ok, revocation, anchor, n, now, flags, results, scratch, scratch_bytes, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (times, parse, crl_times, chain):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    fake = p  # a fake non-NULL context must still be refused before it is touched
    for call in (times, parse, crl_times):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    for call, pointers, aligned8 in ((times, ("offs", "seconds", "status"), ("offs", "seconds")),
                                     (parse, ("certs", "fields"), ("certs", "fields")),
                                     (crl_times, ("crl_fields", "crl_status", "this_s", "next_s", "time_status", "fresh_ok"), ("crl_fields", "this_s", "next_s")),
                                     (chain, ("certs", "policy", "cert_status", "cert_ok", "anchor", "results"), ("certs", "policy", "results"))):
        for name in pointers:
            assert call(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
        for name in aligned8:
            assert call(ctx=fake, **{name: odd4}) == _lib.ERR_PARAM and b"8-byte aligned" in err(), name
    for call in (times, parse, chain):
        assert call(ctx=fake, n=_path_lib.MAX_CERTS + 1) == _lib.ERR_PARAM and b"MLDSA_PATH_MAX_CERTS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_PATH_MAX_CERTS" in err()
    assert crl_times(ctx=fake, n=_crl_lib.MAX_CRLS + 1) == _lib.ERR_PARAM and b"MLDSA_CRL_MAX_CRLS" in err()
    # each call takes its own flag and refuses the others'
    for call, own in ((parse, pc.ALLOW_UNKNOWN_CRITICAL), (crl_times, pc.REQUIRE_NEXT_UPDATE), (chain, pc.ALLOW_NO_CRL)):
        for flags in (1, 2, 4, 8, 7, 0x80000000):
            if flags != own:
                assert call(ctx=fake, flags=flags) == _lib.ERR_PARAM and b"unknown flag" in err(), flags
    assert chain(ctx=fake, scratch=null) == _lib.ERR_PARAM and b"mldsa_path_scratch_bytes" in err()
    assert chain(ctx=fake, scratch=C.c_void_p(p.value + 128)) == _lib.ERR_PARAM and b"256-byte aligned" in err()
    assert chain(ctx=fake, scratch_bytes=lib.mldsa_path_scratch_bytes(4) - 1) == _lib.ERR_PARAM and b"smaller than" in err()
    assert chain(ctx=fake, n=33, scratch_bytes=256) == _lib.ERR_PARAM and b"smaller than" in err()
    # a NULL blob is an empty blob's, revocation and crl_ok may be NULL: the checks go on to the next one
    assert parse(ctx=fake, blob=null, blob_len=0, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    assert chain(ctx=null, revocation=null) == _lib.ERR_PARAM and b"NULL context" in err()
    # empty calls succeed without a context, and touch nothing
    assert times(n=0, blob=null, offs=null, seconds=null, status=null) == _lib.OK
    assert parse(n=0, blob=null, certs=null, fields=null, flags=99) == _lib.OK
    assert crl_times(n=0, blob=null, crl_fields=null, crl_status=null, this_s=null, next_s=null, time_status=null, fresh_ok=null) == _lib.OK
    assert chain(n=0, certs=null, policy=null, cert_status=null, cert_ok=null, anchor=null, results=null, scratch=null, scratch_bytes=0) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(lib):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert lib.mldsa_path_chain(p, p, p, p, p, null, p, 4, 0, 0, p, p, 255, null) == _lib.ERR_PARAM
    mine = lib.mldsa_path_last_error()
    assert mine == b"mldsa_path_chain: scratch is NULL, not 256-byte aligned or smaller than mldsa_path_scratch_bytes"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert lib.mldsa_path_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _path_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "walk_policy", "parse_time", "k_path", "climb"):
        assert word not in exported, word
    del buf


def test_scratch_bytes(lib):
    last = 0
    for n in (0, 1, 31, 32, 33, 64, 65, 257, 65536, 65537, 1 << 30):
        got = lib.mldsa_path_scratch_bytes(n)
        assert got == (8 * n + 255) // 256 * 256 and got >= last
        last = got
    for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
        assert lib.mldsa_path_scratch_bytes(n) == 0


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_time_restatement_against_timegm_on_every_day_of_a_century():
    day, end, count = datetime.date(1950, 1, 1), datetime.date(2049, 12, 31), 0
    while day <= end:
        for clock in ((0, 0, 0), (23, 59, 59)):
            want = calendar.timegm((day.year, day.month, day.day) + clock)
            for der in (pc.utc(day.year, day.month, day.day, *clock), pc.generalized(day.year, day.month, day.day, *clock)):
                assert pc.parse_time(der, 0, len(der)) == (want, len(der)), day
        day += datetime.timedelta(days=1)
        count += 1
    assert count == 36525  # 100 years, 25 of them leap years
    # the leap-year edges, and the ends of the range a GeneralizedTime can name
    for y in (1, 4, 100, 400, 1600, 1700, 1900, 1970, 2000, 2038, 2100, 2400, 9999):
        leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
        for mo, d in ((1, 1), (2, 28), (3, 1), (12, 31)) + (((2, 29),) if leap else ()):
            der = pc.generalized(y, mo, d, 12, 30, 15)
            assert pc.parse_time(der, 0, len(der))[0] == calendar.timegm((y, mo, d, 12, 30, 15)), (y, mo, d)
        assert (pc.parse_time(pc.generalized(y, 2, 29), 0, 17) is not None) == leap
    assert pc.parse_time(pc.utc(1950), 0, 15)[0] == calendar.timegm((1950, 1, 1, 0, 0, 0)) < 0 < pc.parse_time(pc.utc(2049, 12, 31), 0, 15)[0]
    assert pc.parse_time(pc.generalized(1, 1, 1), 0, 17)[0] == -62135596800 and pc.parse_time(pc.generalized(9999, 12, 31, 23, 59, 59), 0, 17)[0] == 253402300799
    # a Time is bounded by the end it is given
    assert pc.parse_time(pc.utc(2025), 0, 14) is None and pc.parse_time(pc.utc(2025) + b"\x00", 0, 16) == (calendar.timegm((2025, 1, 1, 0, 0, 0)), 15)


def test_valid_certificates_have_the_pinned_fields():
    der = pc.case("ok_ca")
    w = pc.walk_policy(der)
    assert w["status"] == 0 and w["flags"] == pc.V3 | pc.HAS_BC | pc.IS_CA | pc.HAS_KU and w["key_usage"] == 0x60 and w["path_len"] == pc.NO_PATH_LEN
    assert w["not_before"] == calendar.timegm((2025, 1, 1, 0, 0, 0)) and w["not_after"] == calendar.timegm((2035, 1, 1, 0, 0, 0))
    assert (w["n_ext"], w["n_crit"], w["crit_off"]) == (2, 0, 0)
    x = xc.walk(der)
    tail_at = x["tbs_off"] + x["tbs_len"] - len(pc.CA_TAIL)
    assert der[tail_at:tail_at + len(pc.CA_TAIL)] == pc.CA_TAIL and w["ext_off"] == tail_at + 4 and w["ext_len"] == len(pc.CA_TAIL) - 4
    assert der[w["ext_off"]:w["ext_off"] + w["ext_len"]] == pc.basic() + pc.key_usage(b"\x01\x06")
    for name, flags, path_len, usage, n_ext in (("ok_v3_plain", pc.V3, pc.NO_PATH_LEN, 0, 0), ("ok_v1", 0, pc.NO_PATH_LEN, 0, 0),
                                                ("ok_v2_both_uids", 0, pc.NO_PATH_LEN, 0, 0), ("ok_bc_empty", pc.V3 | pc.HAS_BC, pc.NO_PATH_LEN, 0, 1),
                                                ("ok_path_len_0", pc.V3 | pc.HAS_BC | pc.IS_CA, 0, 0, 1), ("ok_path_len_127", 7, 127, 0, 1),
                                                ("ok_path_len_128", 7, 128, 0, 1), ("ok_path_len_max", 7, 2 ** 31 - 1, 0, 1),
                                                ("ok_ku_1_bit", pc.V3 | pc.HAS_KU, pc.NO_PATH_LEN, 1, 1), ("ok_ku_8_bits", 9, pc.NO_PATH_LEN, 0xE0, 1),
                                                ("ok_ku_9_bits", 9, pc.NO_PATH_LEN, 0x160, 1), ("ok_ku_16_bits", 9, pc.NO_PATH_LEN, 0x80A5, 1),
                                                ("ok_32_extensions", 15, pc.NO_PATH_LEN, 0x20, 32)):
        w = pc.walk_policy(pc.case(name))
        assert (w["status"], w["flags"], w["path_len"], w["key_usage"], w["n_ext"]) == (0, flags, path_len, usage, n_ext), name
    # an unknown critical extension: where it is, with and without the flag
    der = pc.case("critical_unknown_twice")
    w, allowed = pc.walk_policy(der), pc.walk_policy(der, pc.ALLOW_UNKNOWN_CRITICAL)
    assert w["status"] == pc.CRITICAL and allowed["status"] == 0 and w["n_crit"] == allowed["n_crit"] == 2
    assert w["crit_off"] == allowed["crit_off"] == w["ext_off"] + len(pc.other(0)) and der[w["crit_off"]:w["crit_off"] + len(pc.other(1, True))] == pc.other(1, True)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_every_case_gives_its_documented_status(name):
    for pset in pc.SETS:
        der = pc.case(name, pset)
        w = pc.walk_policy(der)
        assert w["status"] == pc.CASES[name][0], (name, pset, w)
        # the certificate library's walk sees none of this: DER there only where DER here
        assert (xc.walk(der)["status"] == xc.DER) <= (w["status"] == pc.DER)
        if w["status"] == pc.DER:
            assert not any(w[f] for f in w if f != "status")
        if w["status"] == pc.TIME:
            assert w["not_before"] == w["not_after"] == 0


def test_status_order():
    # one certificate that breaks every class: the first in the header's order is the status as the classes are mended one by one
    bad_tail = pc.extensions([pc.other(0, critical=b"\x01\x01\x00"), pc.other(1, critical=True)])
    bad_dates = pc.validity(pc.utc(2025, 13, 1), pc.utc(2035))
    assert pc.walk_policy(pc.make(version=pc.V2, dates=bad_dates, tail=bad_tail + b"\x05\x00"))["status"] == pc.DER
    assert pc.walk_policy(pc.make(version=pc.V2, dates=bad_dates, tail=bad_tail))["status"] == pc.VERSION
    assert pc.walk_policy(pc.make(dates=bad_dates, tail=bad_tail))["status"] == pc.TIME
    assert pc.walk_policy(pc.make(tail=bad_tail))["status"] == pc.EXT
    assert pc.walk_policy(pc.make(tail=pc.extensions([pc.other(1, critical=True)])))["status"] == pc.CRITICAL
    # RANGE before everything
    blob, certs = xc.lay_out([(pc.case("der_tail_wrong_tag"), 1), (pc.case("ok_ca"), 2 ** 32 - 1)], [0, 0])
    assert pc.expected_parse(blob, certs)["status"].tolist() == [pc.RANGE, pc.RANGE]


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the certificates independently")
def test_builder_and_walk_agree_with_openssl_asn1parse(tmp_path):
    for name in ("ok_ca", "ok_v2_both_uids", "ok_32_extensions", "ok_generalized_dates", "critical_unknown"):
        der = pc.case(name, 65)
        path = tmp_path / "c.der"
        path.write_bytes(der)
        run = subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        lines = [re.match(r"\s*(\d+):d=(\d+)\s+hl=\s*(\d+)\s+l=\s*(\d+)\s+(cons|prim):\s+(.*)", ln) for ln in run.stdout.splitlines()]
        rows = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(6)) for m in lines if m]
        w = pc.walk_policy(der, pc.ALLOW_UNKNOWN_CRITICAL)
        assert w["status"] == 0
        wrapper = [r for r in rows if r[1] == 2 and r[4].startswith("cont [ 3 ]")]
        assert len(wrapper) == (1 if w["ext_off"] else 0)
        if wrapper:
            seq = rows[rows.index(wrapper[0]) + 1]
            assert (seq[0] + seq[2], seq[3]) == (w["ext_off"], w["ext_len"])
            assert len([r for r in rows if r[1] == 4 and w["ext_off"] <= r[0] < w["ext_off"] + w["ext_len"] and "SEQUENCE" in r[4]]) == w["n_ext"]
        dates = [r for r in rows if r[1] == 3 and ("UTCTIME" in r[4] or "GENERALIZEDTIME" in r[4])]
        assert len(dates) == 2
        for r, f in zip(dates, ("not_before", "not_after")):
            text = r[4].split(":")[-1]
            text = text if "GENERALIZED" in r[4] else ("20" if int(text[:2]) < 50 else "19") + text
            want = calendar.timegm(tuple(int(text[a:b]) for a, b in ((0, 4), (4, 6), (6, 8), (8, 10), (10, 12), (12, 14))))
            assert w[f] == want, (name, f)


def test_chain_restatement_on_hand_made_chains():
    now = 1500
    # a line of depth 3, every certificate a CA: everything trusted, the depth is the distance
    issuers, anchor = pc.line(3)
    rows, zero, one = pc.policy_rows(4), np.zeros(4, dtype=np.uint8), np.ones(4, dtype=np.uint8)
    got = pc.expected_chain(issuers, rows, zero, one, None, anchor, now)
    assert got["verdict"].tolist() == [0] * 4 and got["where"].tolist() == [0] * 4 and got["depth"].tolist() == [0, 1, 2, 3]
    # the leaf need not be a CA, the certificate above it must be
    rows = pc.policy_rows(4)
    rows[3] = pc.policy_rows(1, ca=False)[0]
    assert pc.expected_chain(issuers, rows, zero, one, None, anchor, now)["verdict"].tolist() == [0] * 4
    rows[2] = pc.policy_rows(1, ca=False)[0]
    got = pc.expected_chain(issuers, rows, zero, one, None, anchor, now)
    assert got["verdict"].tolist() == [0, 0, 0, pc.NOT_CA] and got[3]["where"] == 2 and got[3]["depth"] == 1
    # pathLen: certificate 1 allows one CA below it; the leaf at distance 2 from it is the last that passes
    issuers, anchor = pc.line(4)
    rows, zero, one = pc.policy_rows(5), np.zeros(5, dtype=np.uint8), np.ones(5, dtype=np.uint8)
    rows[1]["path_len"] = 1
    got = pc.expected_chain(issuers, rows, zero, one, None, anchor, now)
    assert got["verdict"].tolist() == [0, 0, 0, 0, pc.PATH_LEN] and got[4]["where"] == 1 and got[4]["depth"] == 3
    # an anchor is checked for nothing: an expired root that is one does not matter, without the mark it does
    rows = pc.policy_rows(5)
    rows[0]["not_after"] = now - 1
    assert pc.expected_chain(issuers, rows, zero, one, None, anchor, now)["verdict"].tolist() == [0] * 5
    got = pc.expected_chain(issuers, rows, zero, one, None, np.zeros(5, dtype=np.uint8), now)
    assert got["verdict"].tolist() == [pc.EXPIRED] * 5 and got["where"].tolist() == [0] * 5
    # no anchor, a cycle, the depth
    got = pc.expected_chain(issuers, pc.policy_rows(5), zero, one, None, np.zeros(5, dtype=np.uint8), now)
    assert got["verdict"].tolist() == [pc.NO_ANCHOR] * 5 and got["where"].tolist() == [0] * 5
    cycle = np.array([1, 2, 0], dtype=np.uint32)
    got = pc.expected_chain(cycle, pc.policy_rows(3), zero[:3], one[:3], None, zero[:3], now)
    assert got["verdict"].tolist() == [pc.DEPTH] * 3 and got["depth"].tolist() == [16] * 3 and got["where"].tolist() == [1, 2, 0]
    for depth, verdict in ((16, pc.TRUSTED), (17, pc.DEPTH)):
        issuers, anchor = pc.line(depth)
        got = pc.expected_chain(issuers, pc.policy_rows(depth + 1), np.zeros(depth + 1, dtype=np.uint8), np.ones(depth + 1, dtype=np.uint8), None, anchor, now)
        assert got[depth]["verdict"] == verdict and got[depth]["depth"] == 16 and got[depth]["where"] == (0 if verdict == pc.TRUSTED else 1)


# ---- the plan under the sanitizers ---------------------------------------------------------------------------------------------------
def chain_cases():
    """node arrays (as bytes) for the climb: lines of every depth up to the bound and one past it, every rule at every place, cycles"""
    out = []
    for depth in (0, 1, 2, 3, 15, 16, 17, 20):
        for anchored in (True, False):
            issuers, anchor = pc.line(depth, anchored)
            n = depth + 1
            out.append(pc.nodes_of(issuers, pc.policy_rows(n), np.zeros(n, np.uint8), np.ones(n, np.uint8), None, anchor, 1500))
    issuers, anchor = pc.line(4)
    for at in range(5):
        for own in range(8):
            for as_issuer in (0, pc.NOT_CA, pc.KEY_USAGE):
                for path_len in (255, 0, 1, 2):
                    nodes = pc.nodes_of(issuers, pc.policy_rows(5), np.zeros(5, np.uint8), np.ones(5, np.uint8), None, anchor, 1500)
                    nodes[at]["own"], nodes[(at + 1) % 5]["as_issuer"], nodes[(at + 2) % 5]["path_len"] = own, as_issuer, path_len
                    out.append(nodes)
    for issuers in ([0], [1, 0], [1, 2, 0], [5, 0], [pc.NO_ISSUER], [1, pc.NO_ISSUER], [1, 2, 2]):
        n = len(issuers)
        out.append(pc.nodes_of(np.array(issuers, dtype=np.uint32), pc.policy_rows(n), np.zeros(n, np.uint8), np.ones(n, np.uint8), None,
                               np.zeros(n, np.uint8), 1500))
    return out


def test_the_time_reader_the_walk_and_the_climb_under_asan_and_ubsan(tmp_path):
    lines, want = [], []
    # the walk: the first case a valid CA (the program walks its prefixes), every case of every set, both flags for the critical ones
    ders = [(pc.case("ok_ca"), 0)]
    for k, pset in enumerate(pc.SETS):
        for name in pc.CASES:
            ders.append((pc.case(name, pset, k), pc.ALLOW_UNKNOWN_CRITICAL if name.startswith("critical") and k == 1 else 0))
    base = pc.case("ok_32_extensions")
    positions = pc.spans(base)
    for pos in positions[:32 + 40] + positions[-60:]:
        for v in xc.MUTATION_VALUES:
            ders.append((base[:pos] + bytes([v]) + base[pos + 1:], 0))
    base = pc.case("ok_v3_uid_and_ca")
    for pos in pc.spans(base):
        for v in xc.MUTATION_VALUES:
            ders.append((base[:pos] + bytes([v]) + base[pos + 1:], v & 1))
    seen = set()
    for der, flags in ders:
        w = pc.walk_policy(der, flags)
        lines.append("W %d %s" % (flags, der.hex()))
        want.append(" ".join(str(w[f]) for f in ("status", "not_before", "not_after", "ext_off", "ext_len", "crit_off", "path_len", "key_usage", "flags",
                                                  "n_ext", "n_crit")))
        seen.add(w["status"])
    assert seen == {pc.OK, pc.DER, pc.VERSION, pc.TIME, pc.EXT, pc.CRITICAL}
    # the Time reader: the month ends of a few years, every refusal, every single-byte change of both forms, every prefix
    times = [pc.generalized(y, mo, d, 23, 59, 59) for y in (1, 1600, 1900, 1970, 2000, 2038, 2100, 2400, 9999) for mo in range(1, 13) for d in (28, 29, 30, 31, 32)]
    times += [pc.utc(y, mo, d) for y in (1950, 1999, 2000, 2049) for mo in (0, 1, 2, 12, 13) for d in (0, 1, 28, 29, 30)]
    for good in (pc.utc(2024, 2, 29, 23, 59, 59), pc.generalized(2024, 2, 29, 23, 59, 59)):
        times += [good[:pos] + bytes([v]) + good[pos + 1:] for pos in range(len(good)) for v in (0x00, 0x2F, 0x30, 0x39, 0x3A, 0x5A, 0x7A, 0x80, 0xFF)]
        times += [good[:k] for k in range(len(good))] + [good + b"\x17"]
    for t in times:
        got = pc.parse_time(t, 0, len(t))
        lines.append("T " + t.hex())
        want.append("0 0 0" if got is None else "1 %d %d" % got)
    assert sum(w.startswith("1 ") for w in want[-len(times):]) > 300
    # the climb
    for nodes in chain_cases():
        lines.append("C " + nodes.tobytes().hex())
        want.append(" ".join("%d:%d:%d" % pc.climb(nodes, i) for i in range(len(nodes))))
    verdicts = {int(x.split(":")[0]) for w in want[-len(chain_cases()):] for x in w.split()}
    assert verdicts == set(range(13))
    (tmp_path / "cases.txt").write_text("".join(ln + "\n" for ln in lines))
    rows_path = tmp_path / "rows.txt"
    sanitized_program(tmp_path, "path_plan", ["path_plan_main.cpp"], "path_plan OK", env={"PATH_CASES": str(tmp_path / "cases.txt"), "PATH_ROWS": str(rows_path)})
    rows = rows_path.read_text().splitlines()
    assert len(rows) == len(want)
    for i, (got, w) in enumerate(zip(rows, want)):
        assert got == w, (i, lines[i][:120], got, w)
