"""The certificate library (include/mldsa_x509.h, fips204_amd/x509/libmldsa_x509.so) without a device: its C ABI, how it is linked against
the core, its argument checks, its kernels' resources and sources, the builder and the restatement of tests/x509_cases.py against pinned
offsets, an independent parser and the oracle, and the walk as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import x509_cases as xc
from fips204_amd import _lib, _mus_lib, _x509_lib
from layer_checks import (PK_SK, ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, core_params, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, sanitized_program, sources_clean)
from oracle import oracle as orc

X509_DIR = os.path.join(ROOT, "fips204_amd", "x509")
SOURCES = ["Makefile", "x509.hip", "x509_plan.h", "x509_dev.h"]


@pytest.fixture(scope="module")
def x509():
    return built(_x509_lib, X509_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(x509, tmp_path):
    from fips204_amd import build
    assert build.PARSE_LAYERS == {"x509": "libmldsa_x509.so"} and build.X509_LIB == _x509_lib.LIB_PATH and build.X509_DIR == X509_DIR
    assert len(build.LAYERS) == 8 and build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"}  # the two older dicts as they were
    # x509_plan.h includes ../rec/rec_plan.h: the shadow links rec/ too
    (tmp_path / "fips204_amd").mkdir()
    os.symlink(build.REC_DIR, tmp_path / "fips204_amd" / "rec")
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS}.items()]
    clean_build("x509", _x509_lib, SOURCES, libs, tmp_path)  # build() builds it: the library is there after build()
    mk = open(os.path.join(X509_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    assert "../rec/rec_plan.h" in mk and "-lmldsa_rec" not in mk  # a change of the shared plan rebuilds this library
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_x509_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(x509, tmp_path):
    declared, text = header_and_exports(
        _x509_lib, x509,
        "int main(void) { mldsa_x509_cert c; mldsa_x509_fields f; mldsa_rec_op o;\n"
        "  c.issuer = MLDSA_X509_NO_ISSUER; f.status = MLDSA_X509_PARSE_ONLY; f.key_set = MLDSA_87; o.set = 0;\n"
        "  return sizeof(c) == 16 && sizeof(f) == 56 && sizeof(o) == 40 && mldsa_x509_abi_version() == MLDSA_X509_ABI_VERSION\n"
        "    && c.issuer > MLDSA_X509_MAX_CERTS && f.status == 7 && MLDSA_X509_CHECK_NAMES == 1u && !o.set ? 0 : 1; }\n",
        r"\b(mldsa_x509_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_x509_abi_version", "mldsa_x509_last_error", "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops"}
    assert '#include "mldsa_rec.h"' in text  # for the descriptor type only
    # the Python constants and layouts are the header's
    assert "#define MLDSA_X509_ABI_VERSION 1" in text and x509.mldsa_x509_abi_version() == _x509_lib.ABI_VERSION == 1
    assert "#define MLDSA_X509_MAX_CERTS (1u << 30)" in text and _x509_lib.MAX_CERTS == 1 << 30
    assert "#define MLDSA_X509_NO_ISSUER 0xFFFFFFFFu" in text and _x509_lib.NO_ISSUER == xc.NO_ISSUER == 0xFFFFFFFF
    assert "#define MLDSA_X509_CHECK_NAMES 1u" in text and _x509_lib.CHECK_NAMES == xc.CHECK_NAMES == 1
    for code, name in enumerate(("OK", "RANGE", "DER", "ALG", "SIG", "ISSUER", "NAME", "PARSE_ONLY")):
        assert re.search(r"#define MLDSA_X509_%s %d\b" % (name, code), text), name
        assert getattr(_x509_lib, name) == getattr(xc, name) == code
    assert _x509_lib.CERT_DTYPE.itemsize == 16 and _x509_lib.FIELDS_DTYPE.itemsize == 56
    assert [_x509_lib.CERT_DTYPE.fields[f][1] for f in ("off", "len", "issuer")] == [0, 8, 12]
    names = ("tbs_off", "sig_off", "key_off", "issuer_off", "subject_off", "tbs_len", "issuer_len", "subject_len", "sig_set", "key_set",
             "status", "reserved")
    assert [_x509_lib.FIELDS_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 53, 54, 55]
    # the lengths the restatement and the plan use are the core's
    params = core_params()
    plan = open(os.path.join(ROOT, "fips204_amd", "rec", "rec_plan.h")).read()
    for pset in (44, 65, 87):
        assert (params[pset].pk_len, params[pset].sig_len) == (xc.PK_LEN[pset], xc.SIG_LEN[pset]) and xc.PK_LEN[pset] == PK_SK[pset][0]
        assert str(xc.PK_LEN[pset]) in plan and str(xc.SIG_LEN[pset]) in plan
    # what is out of scope is said, and a measurement is stated only where its file exists
    for word in ("NOT IN SCOPE", "Validity dates".lower(), "extensions", "revocation", "PEM"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "x509_bench.jsonl")):
        assert "not measured" in text


def test_layered_on_the_one_core_library(x509):
    # The library's one core call is mldsa_ctx_device.  (It makes no core call that can fail with a message of the core's, so it does
    # not take mldsa_last_error either: its messages are its own.)
    layered_on_core(_x509_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_verify_pk", "mldsa_verify", "mldsa_sign", "mldsa_keygen", "mldsa_verify_mu", "mldsa_rec_verify",
                           "mldsa_rec_plan", "mldsa_rec_pack"))
    links_the_core_and_never_builds_it(X509_DIR)
    dyn = subprocess.run(["readelf", "-d", _x509_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign)\.so", dyn)


def test_argument_errors_never_abort(x509):
    null = None
    buf, p, _ = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    err = x509.mldsa_x509_last_error

    def parse(ctx=null, blob=p, blob_len=4096, certs=p, n=4, fields=p, stream=null):
        return x509.mldsa_x509_parse(ctx, blob, blob_len, certs, n, fields, stream)

    def link(ctx=null, blob=p, blob_len=4096, certs=p, fields=p, n=4, flags=1, ops=p, status=p, stream=null):
        return x509.mldsa_x509_link(ctx, blob, blob_len, certs, fields, n, flags, ops, status, stream)

    def ops(ctx=null, blob=p, blob_len=4096, certs=p, n=4, flags=1, fields=p, ops=p, status=p, stream=null):
        return x509.mldsa_x509_ops(ctx, blob, blob_len, certs, n, flags, fields, ops, status, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (parse, link, ops):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    # a fake non-NULL context must still be refused before it is touched
    fake = p
    for call in (parse, link, ops):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, certs=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, certs=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, fields=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n=_x509_lib.MAX_CERTS + 1) == _lib.ERR_PARAM and b"MLDSA_X509_MAX_CERTS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_X509_MAX_CERTS" in err()
    for call in (link, ops):
        assert call(ctx=fake, ops=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, status=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, ops=odd4) == _lib.ERR_PARAM and b"ops must be 8-byte aligned" in err()
        for flags in (2, 3, 0x80000000):
            assert call(ctx=fake, flags=flags) == _lib.ERR_PARAM and b"unknown flag" in err(), flags
    # a NULL blob is an empty blob's: only with blob_len > 0 is it an error (the checks go on to the next one)
    assert parse(ctx=fake, blob=null, blob_len=0, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
    # empty calls succeed without a context, and touch nothing
    assert parse(n=0, blob=null, certs=null, fields=null) == _lib.OK
    assert link(n=0, blob=null, certs=null, fields=null, ops=null, status=null, flags=99) == _lib.OK
    assert ops(n=0, blob=null, certs=null, fields=null, ops=null, status=null) == _lib.OK
    del buf


def test_the_error_slot_is_this_librarys_own(x509):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert x509.mldsa_x509_link(p, p, 16, p, p, 4, 6, p, p, null) == _lib.ERR_PARAM
    mine = x509.mldsa_x509_last_error()
    assert mine == b"mldsa_x509_link: unknown flag"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert x509.mldsa_x509_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _x509_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "k_x509"):
        assert word not in exported, word
    del buf


def test_kernels_do_not_spill_and_sources_are_clean(x509):
    kernels = kernel_resources(X509_DIR)
    for stem in ("k_x509_parse", "k_x509_link"):
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == 2
    read = dict(sources_clean(X509_DIR, ["../../include/mldsa_x509.h", "../_x509_lib.py", "../layer/layer_host.h", "../layer/layer_dev.h"]))
    src, plan, dev = read["x509.hip"], read["x509_plan.h"], read["x509_dev.h"]
    certificate_helpers_shared_once("x509")
    for h in ("../layer/layer_host.h", "../layer/layer_dev.h", "../../include/mldsa_x509.h", "x509_plan.h", "x509_dev.h"):
        assert f'#include "{h}"' in src, h
    assert '#include "../rec/rec_plan.h"' in plan
    # the kernel boundary does the ordering: no atomics, no flag another workgroup waits for, no host wait; the scaffold is shared, not copied
    for word in ("atomic", "__threadfence", "while (true)", "for (;;)", "s_sleep", "hipGraph", "hipStreamCreate", "hipStreamSynchronize",
                 "hipMemcpy", "hipMalloc", "struct DeviceScope", "thread_local", "int fail(", "mldsa_rec_verify(", "mldsa_verify"):
        assert word not in src and word not in plan, word
    # the plan has no HIP in it, and the kernels keep no second copy of its rules: they call the plan's functions
    code = re.sub(r"//[^\n]*", "", plan)
    assert "hip" not in code.lower() and "__device__" not in plan and "__global__" not in plan
    kernel_code = re.sub(r"//[^\n]*", "", src + dev)  # (the link step's comparison is x509_dev.h's, which k_crl_link shares)
    for call in ("walk(", "link_status(", "name_byte_diff(", "in_range(", "wave_or("):
        assert call in kernel_code and "constexpr" in plan, call
    for word in ("read_tlv", "0x1F", "0x80", "0x84", "0x30", "0x03", "0xA0", "0x0365014886600906"):  # the rules live in the plan alone
        assert word in plan and word not in kernel_code, word


# ---- the builder and the restatement ------------------------------------------------------------------------------------------------
def plain(pset, i=0):
    return xc.cert(xc.tbs(pset, pset, b"root", b"leaf", xc._bytes(b"pk", i, xc.PK_LEN[pset])), pset, xc._bytes(b"sig", i, xc.SIG_LEN[pset]))


def one(der, length=None, flags=xc.CHECK_NAMES):
    """fields row and status of one certificate that is its own issuer"""
    blob, certs = xc.lay_out([(der, len(der) if length is None else length)], [0], pad=5)
    fields, ops, status = xc.expected(blob, certs, flags)
    return fields[0], ops[0], int(status[0]), int(certs[0]["off"])


@pytest.mark.parametrize("pset,sig_at,total", [(44, 1448, 3868), (65, 2088, 5397), (87, 2728, 7355)])
def test_valid_certificates_have_the_pinned_offsets(pset, sig_at, total):
    der = plain(pset)
    assert len(der) == total
    w = xc.walk(der)
    assert (w["status"], w["tbs_off"], w["key_off"], w["sig_off"], w["sig_set"], w["key_set"]) == (0, 4, 118, sig_at, pset, pset)
    assert der[w["issuer_off"]:w["issuer_off"] + w["issuer_len"]] == xc.name(b"root")
    assert der[w["subject_off"]:w["subject_off"] + w["subject_len"]] == xc.name(b"leaf")
    assert der[w["tbs_off"]:w["tbs_off"] + w["tbs_len"]] == xc.tbs(pset, pset, b"root", b"leaf", xc._bytes(b"pk", 0, xc.PK_LEN[pset]))
    # as its own issuer it is accepted without the flag; with it, "root" did not issue "leaf"
    f, op, st, off = one(der, flags=0)
    assert st == xc.OK and (int(f["tbs_off"]), int(f["key_off"]), int(f["sig_off"])) == (off + 4, off + 118, off + sig_at)
    assert (int(op["pk_off"]), int(op["sig_off"]), int(op["msg_off"]), int(op["msg_len"])) == (off + 118, off + sig_at, off + 4, w["tbs_len"])
    assert (int(op["ctx_off"]), int(op["ctx_len"]), int(op["set"]), int(op["reserved"])) == (0, 0, pset, 0)
    f, op, st, _ = one(der)
    assert st == xc.NAME and op.tobytes() == bytes(40) and int(f["status"]) == xc.OK


def test_builder_options_and_name_length_forms():
    for v3 in (True, False):
        for tail in (b"", xc.extensions(40), xc.tlv(0x81, b"\x00\x01") + xc.tlv(0x82, b"\x00\x02") + xc.extensions(300)):
            for cn in (b"x", b"y" * 100, b"z" * 116, b"w" * 117, b"v" * 300):
                der = xc.random_cert(65, 44, cn, cn, b"opt", len(cn), v3=v3, tail=tail)
                w = xc.walk(der)
                assert (w["status"], w["sig_set"], w["key_set"]) == (0, 65, 44)
                assert w["issuer_len"] == w["subject_len"] == len(xc.name(cn))
                assert der[w["subject_off"]:w["subject_off"] + w["subject_len"]] == xc.name(cn)
                assert w["key_off"] == 118 - (0 if v3 else 5) + 2 * (len(xc.name(cn)) - 17)
    # the three forms of a Name's length: short below 128, 0x81 up to 255, 0x82 above
    forms = [xc.name(b"n" * k)[1] for k in range(1, 301)]
    assert forms[0] == 12 and forms == sorted(forms) and max(f for f in forms if f < 0x80) == 127 and set(f for f in forms if f >= 0x80) == {0x81, 0x82}
    assert all(xc.take(xc.name(b"n" * k), 0, 400)[2] == len(xc.name(b"n" * k)) for k in range(1, 301))


@pytest.mark.parametrize("defect", list(xc.DEFECTS))
def test_every_defect_gives_its_documented_status(defect):
    for pset in xc.SETS:
        good = xc.random_cert(pset, pset, b"self", b"self", b"defect", pset)
        data, length = xc.make_defect(good, defect)
        blob, certs = xc.lay_out([(good, len(good)), (data, length), (good, len(good))], [0, 0, 2], pad=[2, 9, 4], front=1)
        fields, ops, status = xc.expected(blob, certs)
        assert status.tolist() == [0, xc.DEFECTS[defect], 0], (defect, pset)
        assert int(fields[1]["status"]) == xc.DEFECTS[defect] and (int(fields[1]["key_set"]) == 0) == (defect in xc.KEY_SET_ZERO or status[1] == xc.DER)
        assert (ops[1].tobytes() == bytes(40)) == (status[1] != 0)
        if status[1] == xc.DER:
            assert fields[1].tobytes() == bytes(54) + bytes([xc.DER, 0])
        if defect in xc.KEY_SET_ZERO:  # fine as a leaf, useless as an issuer
            certs[2]["issuer"] = 1
            assert xc.expected(blob, certs)[2].tolist() == [0, 0, xc.ISSUER]


def test_len_one_short_reads_nothing_behind_the_declared_range():
    good = plain(44)
    blob, certs = xc.lay_out([xc.make_defect(good, "len_one_short")], [0])
    assert blob[int(certs[0]["off"]):][:len(good)].tobytes() == good  # the missing byte is there, behind the range
    assert xc.expected(blob, certs)[2].tolist() == [xc.DER]
    # and the range rule: len below 2, a range that ends behind the blob, an offset behind it
    for off, length in ((0, 0), (0, 1), (blob.size, 2), (blob.size - 1, 2), (2 ** 64 - 1, 2), (0, blob.size + 1)):
        certs[0]["off"], certs[0]["len"] = off, min(length, 2 ** 32 - 1)
        fields, ops, status = xc.expected(blob, certs)
        assert status.tolist() == [xc.RANGE] and fields[0].tobytes() == bytes(54) + bytes([xc.RANGE, 0])


def test_precedence_the_earlier_rule_is_reported():
    good = xc.random_cert(44, 44, b"self", b"self", b"prec", 0)

    def status_of(*defects, issuer=0, length=None):
        data, n = good, len(good)
        for d in defects:
            data, n = xc.make_defect(data, d)
        blob, certs = xc.lay_out([(data, n if length is None else length), (good, len(good))], [issuer, 1])
        return int(xc.expected(blob, certs)[2][0])

    assert status_of("sig_one_short", "outer_alg_null_params") == xc.ALG            # ALG before SIG
    assert status_of("sig_unused_bits", "alg_sets_differ") == xc.ALG
    assert status_of("outer_alg_null_params", "wrong_tag_validity") == xc.DER       # DER before ALG, wherever on the path it lies
    assert status_of("sig_one_short", "spki_trailing") == xc.DER                    # ... and before SIG
    assert status_of("wrong_tag_spki", length=1) == xc.RANGE                         # RANGE before DER
    assert status_of("sig_one_short", issuer=7) == xc.SIG                            # SIG before ISSUER
    assert status_of("alg_sets_differ", issuer=xc.NO_ISSUER) == xc.ALG              # ... and before PARSE_ONLY
    assert status_of(issuer=7) == xc.ISSUER and status_of(issuer=xc.NO_ISSUER) == xc.PARSE_ONLY and status_of() == xc.OK


def test_link_rules_of_the_restatement():
    root44 = xc.random_cert(44, 44, b"root", b"root", b"link", 0)
    root65 = xc.random_cert(65, 65, b"root", b"root", b"link", 1)
    leaf = xc.random_cert(44, 65, b"root", b"leaf", b"link", 2)            # signed by an ML-DSA-44 issuer called root
    other = xc.random_cert(44, 0, b"rooT", b"leaf2", b"link", 3)           # the last byte of its issuer Name differs; an RSA key
    longer = xc.random_cert(44, 44, b"root1", b"leaf3", b"link", 4)        # the issuer Name is one byte longer
    broken = xc.make_defect(root44, "wrong_tag_subject")
    badsig = xc.make_defect(root44, "sig_unused_bits")
    entries = [(c, len(c)) for c in (root44, root65, leaf, other, longer)] + [broken, badsig]
    n = len(entries)

    def run(issuers, flags=xc.CHECK_NAMES):
        blob, certs = xc.lay_out(entries, issuers, pad=[1, 6])
        return xc.expected(blob, certs, flags)

    base = [0, 1, 0, 0, 0, 5, 6]
    fields, ops, status = run(base)
    assert status.tolist() == [0, 0, 0, xc.NAME, xc.NAME, xc.DER, xc.SIG]
    assert int(ops[2]["pk_off"]) == int(fields[0]["key_off"]) and int(ops[2]["sig_off"]) == int(fields[2]["sig_off"]) and int(ops[2]["set"]) == 44
    assert run(base, flags=0)[2].tolist() == [0, 0, 0, 0, 0, xc.DER, xc.SIG]       # without the flag no Name is compared
    assert run([0, 1, n, 0, 0, 5, 6])[2][2] == xc.ISSUER                            # issuer out of range
    assert run([0, 1, 2 ** 32 - 2, 0, 0, 5, 6])[2][2] == xc.ISSUER
    assert run([0, 1, 5, 0, 0, 5, 6])[2][2] == xc.ISSUER                            # the issuer is malformed
    assert run([0, 1, 1, 0, 0, 5, 6])[2][2] == xc.ISSUER                            # cross-set: a 65 key under a 44 signature
    assert run([0, 1, 3, 0, 0, 5, 6])[2][2] == xc.ISSUER                            # the issuer's key is not ML-DSA
    assert run([0, 1, 6, 0, 0, 5, 6])[2][2] == xc.OK                                # an issuer with a SIG status still lends its key
    f, o, s = run([0, 1, xc.NO_ISSUER, 0, 0, 5, 6])
    assert s[2] == xc.PARSE_ONLY and o[2].tobytes() == bytes(40) and int(f[2]["key_set"]) == 65 and int(f[2]["sig_off"]) != 0
    assert run([0, 1, 2, 0, 0, 5, 6])[2][2] == xc.ISSUER                            # itself: its own key is of another set
    assert run([0, 0, 0, 0, 0, 5, 6])[2][1] == xc.ISSUER and run(base)[2][1] == xc.OK  # a self-signed root names itself


# ---- an independent parser ------------------------------------------------------------------------------------------------------------
def asn1parse(der, tmp_path):
    """the (offset, depth, header length, length, type) lines of `openssl asn1parse`, or None where it refuses the file"""
    path = tmp_path / "c.der"
    path.write_bytes(der)
    run = subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(path)], capture_output=True, text=True)
    if run.returncode != 0:
        return None
    rows = []
    for ln in run.stdout.splitlines():
        m = re.match(r"\s*(\d+):d=(\d+)\s+hl=(\d+)\s+l=\s*(\d+)\s+(?:prim|cons):\s+(.+?)\s*(?::.*)?$", ln)
        assert m, ln
        rows.append((int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5]))
    return rows


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the certificates independently")
def test_builder_and_restatement_agree_with_openssl_asn1parse(tmp_path):
    cases = [(pset, True, b"", b"root") for pset in xc.SETS] + [(44, False, xc.extensions(33), b"q" * 200), (87, True, xc.extensions(7), b"r" * 290)]
    for pset, v3, tail, cn in cases:
        der = xc.random_cert(pset, pset, cn, b"leaf", b"ossl", pset, v3=v3, tail=tail)
        rows, w = asn1parse(der, tmp_path), xc.walk(der)
        assert rows is not None and w["status"] == 0
        d1 = [r for r in rows if r[1] == 1]
        assert [r[4] for r in d1] == ["SEQUENCE", "SEQUENCE", "BIT STRING"]
        assert (d1[0][0], d1[0][2] + d1[0][3]) == (w["tbs_off"], w["tbs_len"])
        assert d1[2][0] + d1[2][2] + 1 == w["sig_off"] and d1[2][3] == 1 + xc.SIG_LEN[pset]
        d2 = [r for r in rows if r[1] == 2 and r[0] < d1[1][0] and r[4] == "SEQUENCE"]  # inner algorithm, issuer, validity, subject, SPKI
        assert len(d2) == 5
        assert (d2[1][0], d2[1][2] + d2[1][3]) == (w["issuer_off"], w["issuer_len"])
        assert (d2[3][0], d2[3][2] + d2[3][3]) == (w["subject_off"], w["subject_len"])
        key = [r for r in rows if r[1] == 3 and r[4] == "BIT STRING" and r[0] > d2[4][0]]
        assert len(key) == 1 and key[0][0] + key[0][2] + 1 == w["key_off"] and key[0][3] == 1 + xc.PK_LEN[pset]
        assert key[0][0] + key[0][2] + key[0][3] == d2[4][0] + d2[4][2] + d2[4][3]  # the key ends the SPKI
        oids = [ln for ln in subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(tmp_path / "c.der")], capture_output=True,
                                            text=True).stdout.splitlines() if "2.16.840.1.101.3.4.3." in ln or "ML-DSA" in ln.upper()]
        assert len(oids) == 3  # inner, SPKI and outer algorithm
    # asn1parse reads BER, so an indefinite, a non-minimal or a five-byte length passes it; what no reader can follow fails there as well
    good = plain(44)
    for defect in ("len_one_short", "tbs_overruns"):
        data, length = xc.make_defect(good, defect)
        assert xc.walk(data[:length])["status"] == xc.DER and asn1parse(data[:length], tmp_path) is None, defect


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------------
def oracle_verdicts(blob, ops, status):
    raw = blob.tobytes()
    out = []
    for op, st in zip(ops, status):
        if st != 0:
            out.append(False)
            continue
        pset = int(op["set"])
        pk = raw[int(op["pk_off"]):int(op["pk_off"]) + xc.PK_LEN[pset]]
        sig = raw[int(op["sig_off"]):int(op["sig_off"]) + xc.SIG_LEN[pset]]
        msg = raw[int(op["msg_off"]):int(op["msg_off"]) + int(op["msg_len"])]
        assert (int(op["ctx_off"]), int(op["ctx_len"]), int(op["reserved"])) == (0, 0, 0)
        out.append(bool(orc.verify_internal(pset, orc.pk_try_from_bytes(pset, pk), msg, sig, ctx=b"", mode=orc.MODE_PURE)))
    return out


def test_restated_ops_of_signed_chains_verify_under_the_oracle():
    ders, issuers = [], []
    for psets, tag in (((44, 44, 44), b"c44"), ((65, 65, 65), b"c65"), ((87, 87, 87), b"c87"), ((87, 65, 44), b"cross")):
        d, iss = xc.signed_chain(psets, tag)
        issuers += [len(ders) + j for j in iss]
        ders += d
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], issuers, pad=list(range(16)), front=3)
    fields, ops, status = xc.expected(blob, certs)
    assert status.tolist() == [0] * 12 and [int(o["set"]) for o in ops] == [44] * 3 + [65] * 3 + [87] * 3 + [87, 87, 65]
    assert oracle_verdicts(blob, ops, status) == [True] * 12
    # one flipped byte each: in a TBS (not in its key), in a signature, in an issuer's key
    bad = blob.copy()
    bad[int(fields[1]["tbs_off"]) + 12] ^= 1      # the serial of the 44 intermediate: its own verdict
    bad[int(fields[5]["sig_off"]) + 100] ^= 0x40  # the signature of the 65 leaf
    bad[int(fields[6]["key_off"]) + 500] ^= 2     # the key of the 87 root: itself and its child, and not its grandchild
    f2, o2, s2 = xc.expected(bad, certs)
    assert s2.tolist() == [0] * 12 and np.array_equal(o2, ops)
    assert [i for i, v in enumerate(oracle_verdicts(bad, o2, s2)) if not v] == [1, 5, 6, 7]
    # a key flip fails every child of that issuer (and the issuer, whose TBS holds the key): a fan of leaves under the 44 intermediate
    fan = np.concatenate([certs, np.repeat(certs[2:3], 3)])
    bad = blob.copy()
    bad[int(fields[1]["key_off"])] ^= 0x80
    f3, o3, s3 = xc.expected(bad, fan)
    assert [i for i, v in enumerate(oracle_verdicts(bad, o3, s3)) if not v] == [1, 2, 12, 13, 14]


# ---- the walk under the sanitizers ------------------------------------------------------------------------------------------------------
def test_the_walk_and_link_rule_under_asan_and_ubsan(tmp_path):
    sanitized_program(tmp_path, "x509_plan", ["x509_plan_main.cpp"], "x509_plan OK")
