"""The certification-request library (include/mldsa_csr.h, fips204_amd/csr/libmldsa_csr.so) without a device: its C ABI, how it is linked
against the core, its host helpers and argument checks, its kernels' resources, the restatement of tests/csr_cases.py against pinned
offsets, openssl, the issuing and the verifying side's restatements and the oracle, and the walk, the rules and the TBSCertificate's
bytes as a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import csr_cases as cs
import x509_cases as xc
import x509sign_cases as xs
from fips204_amd import _csr_lib, _lib, _mus_lib, _x509_lib, _x509sign_lib
from layer_checks import (ROOT, certificate_helpers_shared_once, aligned_buffer, built, clean_build, header_and_exports, kernel_resources, layered_on_core,
                          links_the_core_and_never_builds_it, no_new_dynamic_symbol, sanitized_program)
from oracle import oracle as orc

CSR_DIR = os.path.join(ROOT, "fips204_amd", "csr")
SOURCES = ["Makefile", "csr.hip", "csr_plan.h"]
KERNELS = ("k_csr_parse", "k_csr_check", "k_csr_offsets", "k_csr_apply", "k_csr_tbs_write")


@pytest.fixture(scope="module")
def lib():
    return built(_csr_lib, CSR_DIR)


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_clean_build_in_a_shadow_tree(lib, tmp_path):
    from fips204_amd import build
    assert build.REQUEST_LAYERS == {"csr": "libmldsa_csr.so"}
    assert build.CSR_LIB == _csr_lib.LIB_PATH and build.CSR_DIR == CSR_DIR
    # the four older dicts as they were
    assert len(build.LAYERS) == 8 and build.FRONT_LAYERS == {"recsign": "libmldsa_recsign.so"} and build.PARSE_LAYERS == {"x509": "libmldsa_x509.so"}
    assert build.ISSUE_LAYERS == {"x509sign": "libmldsa_x509sign.so"}
    # csr_plan.h includes the plan headers of three other layers: the shadow links their directories
    (tmp_path / "fips204_amd").mkdir()
    for d in (build.REC_DIR, build.X509_DIR, build.X509SIGN_DIR):
        os.symlink(d, tmp_path / "fips204_amd" / os.path.basename(d))
    libs = [os.path.join(build._HERE, d, f) for d, f in {**build.LAYERS, **build.FRONT_LAYERS, **build.PARSE_LAYERS, **build.ISSUE_LAYERS,
                                                         **build.REQUEST_LAYERS}.items()]
    assert libs[-1] == _csr_lib.LIB_PATH and libs[-2] == _x509sign_lib.LIB_PATH  # built last, behind the issue layers
    clean_build("csr", _csr_lib, SOURCES, libs, tmp_path)
    mk = open(os.path.join(CSR_DIR, "Makefile")).read()
    assert "include ../layer/layer.mk" in mk and "$(HIPCC)" not in mk and "clean" not in mk  # LIB, OBJS, HDRS and the shared recipe
    for h in ("../x509/x509_plan.h", "../x509/x509_dev.h", "../x509sign/x509sign_plan.h", "../rec/rec_plan.h", "../rec/rec_wave.h", "../rec/rec_place.h",
              "csr_plan.h", "mldsa_csr.h"):
        assert h in mk, h  # a change of a shared header rebuilds this library
    assert not re.search(r"-lmldsa_(rec|recsign|x509|x509sign)\b", mk)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_csr_lib.load()" in entry  # build() loads the library it built


def test_header_is_strict_c99_and_declares_exactly_the_exported_symbols(lib, tmp_path):
    declared, text = header_and_exports(
        _csr_lib, lib,
        "#include <stddef.h>\n"
        "int main(void) { mldsa_csr_item c; mldsa_csr_fields f; mldsa_csr_issue e; mldsa_csr_totals t; mldsa_rec_op o; mldsa_x509sign_req q;\n"
        "  c.reserved = 0; f.reserved[1] = 0; e.flags = MLDSA_CSR_RND; e.set = MLDSA_87; t.out_bytes = 0; o.reserved = 0; q.reserved = 0;\n"
        "  return sizeof(c) == 16 && sizeof(f) == 56 && sizeof(e) == 64 && sizeof(t) == 24 && sizeof(o) == 40 && sizeof(q) == 32\n"
        "    && offsetof(mldsa_csr_fields, cri_len) == 40 && offsetof(mldsa_csr_fields, set) == 52 && offsetof(mldsa_csr_fields, status) == 53\n"
        "    && offsetof(mldsa_csr_issue, issuer_len) == 40 && offsetof(mldsa_csr_issue, issuer) == 56 && offsetof(mldsa_csr_issue, serial_len) == 60\n"
        "    && offsetof(mldsa_csr_issue, reserved) == 63 && offsetof(mldsa_csr_item, len) == 8\n"
        "    && mldsa_csr_abi_version() == MLDSA_CSR_ABI_VERSION && MLDSA_CSR_SPACE == 18 && MLDSA_CSR_RND == MLDSA_X509SIGN_RND\n"
        "    && !c.reserved && !f.reserved[1] && !t.out_bytes && !o.reserved && !q.reserved ? 0 : 1; }\n",
        r"\b(mldsa_csr_[a-z0-9_]+)\s*\(", tmp_path)
    assert declared == {"mldsa_csr_abi_version", "mldsa_csr_last_error", "mldsa_csr_tbs_len", "mldsa_csr_plan_bytes", "mldsa_csr_parse",
                        "mldsa_csr_tbs_plan", "mldsa_csr_tbs_write", "mldsa_csr_tbs"}
    for h in ("mldsa_rec.h", "mldsa_x509.h", "mldsa_x509sign.h"):
        assert '#include "%s"' % h in text  # for the types and the codes only
    assert "#define MLDSA_CSR_ABI_VERSION 1" in text and lib.mldsa_csr_abi_version() == _csr_lib.ABI_VERSION == 1
    assert "#define MLDSA_CSR_MAX_REQUESTS (1u << 30)" in text and _csr_lib.MAX_REQUESTS == 1 << 30
    assert "#define MLDSA_CSR_SCAN_BLOCK 256" in text and _csr_lib.SCAN_BLOCK == 256
    assert "#define MLDSA_CSR_RND 1" in text and _csr_lib.FLAG_RND == cs.FLAG_RND == _x509sign_lib.FLAG_RND == 1
    assert "#define MLDSA_CSR_SERIAL_MAX 20" in text and _csr_lib.SERIAL_MAX == cs.SERIAL_MAX == 20
    codes = (("VERSION", 12), ("KEY", 13), ("POP", 14), ("ENTRY", 15), ("TEMPLATE", 16), ("LONG", 17), ("SPACE", 18))
    for name, code in codes:
        assert re.search(r"#define MLDSA_CSR_%s %d\b" % (name, code), text), name
        assert getattr(_csr_lib, name) == getattr(cs, name) == code
    # codes 0 ... 4 are the certificate library's; the new ones are disjoint from its 4 ... 7 and from the issuing library's 8 ... 11
    assert (_csr_lib.OK, _csr_lib.RANGE, _csr_lib.DER, _csr_lib.ALG, _csr_lib.SIG) == (_x509_lib.OK, _x509_lib.RANGE, _x509_lib.DER, _x509_lib.ALG,
                                                                                      _x509_lib.SIG) == (0, 1, 2, 3, 4)
    assert not {c for _, c in codes} & (set(range(8)) | {_x509sign_lib.ENTRY, _x509sign_lib.KEY, _x509sign_lib.LONG, _x509sign_lib.SPACE})
    # the layouts
    assert (_csr_lib.ITEM_DTYPE.itemsize, _csr_lib.FIELDS_DTYPE.itemsize, _csr_lib.ISSUE_DTYPE.itemsize, _csr_lib.TOTALS_DTYPE.itemsize) == (16, 56, 64, 24)
    assert [_csr_lib.ITEM_DTYPE.fields[f][1] for f in ("off", "len", "reserved")] == [0, 8, 12]
    names = ("cri_off", "sig_off", "key_off", "subject_off", "spki_off", "cri_len", "subject_len", "spki_len", "set", "status", "reserved")
    assert [_csr_lib.FIELDS_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 53, 54]
    names = ("serial_off", "issuer_off", "validity_off", "ext_off", "rnd_off", "issuer_len", "validity_len", "ext_len", "key", "issuer",
             "serial_len", "set", "flags", "reserved")
    assert [_csr_lib.ISSUE_DTYPE.fields[f][1] for f in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 61, 62, 63]
    assert [_csr_lib.TOTALS_DTYPE.fields[f][1] for f in ("accepted", "refused", "out_bytes")] == [0, 8, 16]
    # the contract, what is out of scope, and a measurement only where its file exists
    for word in ("THE CONTRACT", "mldsa_x509sign_plan", "walk_tbs", "mldsa_x509_parse", "NOT IN SCOPE", "extensionRequest", "name policy",
                 "validity dates", "PEM", "CRLs", "HashML-DSA", "external-mu", "batcher", "Rust", "proof of possession", "A0 00"):
        assert word in text, word
    if not os.path.exists(os.path.join(ROOT, "profiles", "csr_bench.jsonl")):
        assert "not measured" in text


def test_layered_on_the_one_core_library(lib):
    layered_on_core(_csr_lib.LIB_PATH, needs=("mldsa_ctx_device",),
                    never=("mldsa_sign", "mldsa_verify", "mldsa_verify_pk", "mldsa_keygen", "mldsa_memset", "mldsa_rec_verify", "mldsa_rec_plan",
                           "mldsa_rec_pack", "mldsa_recsign_sign", "mldsa_recsign_plan", "mldsa_x509_parse", "mldsa_x509_link", "mldsa_x509_ops",
                           "mldsa_x509sign_plan", "mldsa_x509sign_frame", "mldsa_x509sign_issue_ops"))
    links_the_core_and_never_builds_it(CSR_DIR)
    dyn = subprocess.run(["readelf", "-d", _csr_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"NEEDED.*libmldsa_(mu|mus|ph|keys|seed|keycheck|vfy|rec|recsign|x509|x509sign)\.so", dyn)
    no_new_dynamic_symbol(_csr_lib.LIB_PATH, "mldsa_csr_")


def test_host_helpers_against_the_restatement(lib):
    for pset in cs.SETS:
        rest = (40, 32, 45, 22 + cs.PK_LEN[pset])
        edge = cs.MAX_TBS[pset] - 24 - 5 - sum(rest)
        for sl, ext in ((1, 0), (20, 0), (5, 100), (5, edge - 1), (5, edge), (5, edge + 1), (0, 0), (21, 0), (5, 2 ** 32), (5, 2 ** 64 - 1), (2 ** 64 - 1, 0)):
            assert lib.mldsa_csr_tbs_len(pset, sl, *rest, ext) == cs.tbs_len(pset, sl, *rest, ext), (pset, sl, ext)
        assert lib.mldsa_csr_tbs_len(pset, 5, *rest, edge) == cs.MAX_TBS[pset] and lib.mldsa_csr_tbs_len(pset, 5, *rest, edge + 1) == 0
        assert lib.mldsa_csr_tbs_len(pset, 5, 2 ** 64 - 30, 32, 45, 1334, 0) == 0  # a sum that would wrap
    for bad in (0, 43, 66, -1, 128, 2 ** 31 - 1):
        assert lib.mldsa_csr_tbs_len(bad, 5, 40, 32, 45, 1334, 0) == 0
    # the plan's working memory: the header's formula, never decreasing, 0 past the cap
    last = 0
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 192, 255, 256, 257, 264, 1000, 65536, 65537, 1 << 30):
        got = lib.mldsa_csr_plan_bytes(n)
        assert got == cs.plan_bytes(n) == xs.plan_bytes(n) and got >= last and got % 256 == 0, n
        last = got
    for n in ((1 << 30) + 1, 2 ** 63, 2 ** 64 - 1):
        assert lib.mldsa_csr_plan_bytes(n) == 0
    text = open(_csr_lib.HEADER_PATH).read()
    assert "R(16 B) + R(4 n)" in text and "4 + 20 + serial_len + issuer_len + validity_len + subject_len + spki_len + ext_len" in text


def test_argument_errors_never_abort(lib):
    null = None
    buf, p, _ = aligned_buffer()
    odd4 = C.c_void_p(p.value + 4)
    other = (C.c_uint8 * 8192)()
    q = C.c_void_p((C.addressof(other) + 255) // 256 * 256)  # a second buffer: apart from the first
    err = lib.mldsa_csr_last_error

    def parse(ctx=null, blob=p, blob_len=1024, items=p, n=4, fields=p, ops=p, status=p, stream=null):
        return lib.mldsa_csr_parse(ctx, blob, blob_len, items, n, fields, ops, status, stream)

    def plan(ctx=null, blob=p, blob_len=1024, fields=p, entries=p, ok=p, n=4, out_len=4096, reqs_out=p, status=p, totals=p, mem=p, mem_bytes=3840,
             stream=null):
        return lib.mldsa_csr_tbs_plan(ctx, blob, blob_len, fields, entries, ok, n, out_len, reqs_out, status, totals, mem, mem_bytes, stream)

    def write(ctx=null, blob=p, blob_len=1024, fields=p, entries=p, n=4, out=q, out_len=4096, reqs_out=p, status=p, stream=null):
        return lib.mldsa_csr_tbs_write(ctx, blob, blob_len, fields, entries, n, out, out_len, reqs_out, status, stream)

    def both(ctx=null, blob=p, blob_len=1024, fields=p, entries=p, ok=p, n=4, out=q, out_len=4096, reqs_out=p, status=p, totals=p, mem=p,
             mem_bytes=3840, stream=null):
        return lib.mldsa_csr_tbs(ctx, blob, blob_len, fields, entries, ok, n, out, out_len, reqs_out, status, totals, mem, mem_bytes, stream)

    # there is no context in this process, so a call that got past its checks would have to use a NULL one: every line below stops earlier
    for call in (parse, plan, write, both):
        assert call() == _lib.ERR_PARAM and b"NULL context" in err()
    fake = p  # a fake non-NULL context must still be refused before it is touched
    for call in (parse, plan, write, both):
        assert call(ctx=fake, blob=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, fields=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, status=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        assert call(ctx=fake, fields=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, n=_csr_lib.MAX_REQUESTS + 1) == _lib.ERR_PARAM and b"MLDSA_CSR_MAX_REQUESTS" in err()
        assert call(ctx=fake, n=2 ** 64 - 1) == _lib.ERR_PARAM and b"MLDSA_CSR_MAX_REQUESTS" in err()
    for name in ("items", "ops"):
        assert parse(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
        assert parse(ctx=fake, **{name: odd4}) == _lib.ERR_PARAM and b"8-byte aligned" in err(), name
    for call in (plan, write, both):
        for name in ("entries", "reqs_out"):
            assert call(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
            assert call(ctx=fake, **{name: odd4}) == _lib.ERR_PARAM and b"8-byte aligned" in err(), name
    for call in (plan, both):
        for name in ("ok", "totals"):
            assert call(ctx=fake, **{name: null}) == _lib.ERR_PARAM and b"NULL pointer" in err(), name
        assert call(ctx=fake, totals=odd4) == _lib.ERR_PARAM and b"8-byte aligned" in err()
        assert call(ctx=fake, mem=null) == _lib.ERR_PARAM and b"mldsa_csr_plan_bytes" in err()
        assert call(ctx=fake, mem=C.c_void_p(p.value + 128)) == _lib.ERR_PARAM and b"256-byte aligned" in err()
        assert call(ctx=fake, mem_bytes=lib.mldsa_csr_plan_bytes(4) - 1) == _lib.ERR_PARAM and b"smaller than" in err()
    # out must not overlap the blob: decided from the two pointer ranges
    for call in (write, both):
        assert call(ctx=fake, out=null) == _lib.ERR_PARAM and b"NULL pointer" in err()
        for out, out_len in ((p, 4096), (C.c_void_p(p.value + 1023), 16), (C.c_void_p(p.value - 15), 16), (C.c_void_p(p.value - 100), 4096)):
            assert call(ctx=fake, out=out, out_len=out_len) == _lib.ERR_PARAM and b": out overlaps the blob" in err(), (out, out_len)
    # flush against the blob on either side is apart: the next check is reached
    assert write(ctx=null, out=C.c_void_p(p.value + 1024), out_len=16) == _lib.ERR_PARAM and b"NULL context" in err()
    # empty calls succeed without a context, and touch nothing
    assert parse(n=0, blob=null, items=null, fields=null, ops=null, status=null) == _lib.OK
    assert plan(n=0, blob=null, fields=null, entries=null, ok=null, reqs_out=null, status=null, totals=null, mem=null, mem_bytes=0) == _lib.OK
    assert write(n=0, blob=null, fields=null, entries=null, out=null, reqs_out=null, status=null) == _lib.OK
    assert both(n=0, blob=null, fields=null, entries=null, ok=null, out=null, reqs_out=null, status=null, totals=null, mem=null, mem_bytes=0) == _lib.OK
    del buf, other


def test_the_error_slot_is_this_librarys_own(lib):
    buf, p, _ = aligned_buffer()
    null, big = None, 1 << 50
    mus = _mus_lib.load()
    assert lib.mldsa_csr_tbs_write(p, p, 64, p, p, 4, p, 64, p, p, null) == _lib.ERR_PARAM
    mine = lib.mldsa_csr_last_error()
    assert mine == b"mldsa_csr_tbs_write: out overlaps the blob"
    assert mus.mldsa_mus_final(p, p, big, null, null, 4, null) == _lib.ERR_PARAM and mus.mldsa_mus_last_error() != mine
    assert lib.mldsa_csr_last_error() == mine
    exported = subprocess.run(["nm", "-D", "--defined-only", _csr_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for word in ("g_err", "DeviceScope", "mldsa_layer", "read_tlv", "walk_tbs", "k_csr", "copy_field"):
        assert word not in exported, word
    del buf


def test_kernels_do_not_spill(lib):
    kernels = kernel_resources(CSR_DIR)
    for stem in KERNELS:
        assert sum(stem in nm for nm in kernels) == 1, stem
    assert len(kernels) == len(KERNELS)  # rec_wave.h and rec_place.h bring no kernel along: nothing is compiled that is not launched
    certificate_helpers_shared_once("csr")
    # LDS in the scan alone: the walk and the write use none
    res = open(os.path.join(CSR_DIR, "csr.res")).read()
    lds = dict(zip(re.findall(r"Function Name: (\S+)", res), (int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", res))))
    assert {stem: [v for nm, v in lds.items() if stem in nm][0] for stem in KERNELS} == \
        {"k_csr_parse": 0, "k_csr_check": 64, "k_csr_offsets": 0, "k_csr_apply": 64, "k_csr_tbs_write": 0}


# ---- the restatement against pinned offsets, openssl, the neighbouring restatements and the oracle ------------------------------------
def one(der, template, length=None, ok=1, out_len=10 ** 6, pad=5):
    """(stage 1's fields row, stage 2's expectation, blob) of one request"""
    blob, items, entries = cs.lay_out([(der, len(der) if length is None else length, template)], pad=pad)
    fields, ops, status = cs.expected_parse(blob, items)
    return fields[0], ops[0], cs.expected_tbs(blob, fields, entries, [ok], out_len), blob, entries


def test_one_fixed_request_gives_the_pinned_rows():
    der = cs.join(cs.parts(44, b"leaf", xc._bytes(b"pk", 0, 1312), xc._bytes(b"sig", 0, 2420)))
    t = (65, 3, b"\x01\x02\x03", xc.name(b"root"), xc.VALIDITY, b"", None, 7)
    row, op, want, blob, entries = one(der, t)
    # 30 82 LLLL | 30 82 LLLL | 02 01 00 | Name (17) | SPKI 30 82 0532 (30 0B oid, 03 82 0521 00 key) | A0 00 | 30 0B oid | 03 82 0975 00 sig
    assert len(der) == 3802 and (int(row["status"]), int(row["set"])) == (0, 44)
    assert (int(row["cri_off"]), int(row["cri_len"])) == (5 + 4, 4 + 3 + 17 + 1334 + 2)
    assert (int(row["subject_off"]), int(row["subject_len"]), int(row["spki_off"]), int(row["spki_len"])) == (5 + 11, 17, 5 + 28, 1334)
    assert int(row["key_off"]) == 5 + 28 + 4 + 13 + 5 and int(row["sig_off"]) == 5 + 8 + 1356 + 13 + 5 == 5 + len(der) - 2420
    assert (int(op["pk_off"]), int(op["sig_off"]), int(op["msg_off"]), int(op["msg_len"])) == (55, 1387, 9, 1360)
    assert (int(op["ctx_off"]), int(op["ctx_len"]), int(op["set"]), int(op["reserved"])) == (0, 0, 44, 0)
    tbs, q = want["tbs"][0], want["reqs"][0]
    assert want["status"].tolist() == [0] and want["totals"] == (1, 0, len(tbs)) and len(tbs) == 24 + 3 + 17 + 32 + 17 + 1334
    assert tuple(int(x) for x in q) == (0, 0, len(tbs), 3, 7, 65, 0, 0)
    assert tbs[:27] == bytes.fromhex("3082") + (len(tbs) - 4).to_bytes(2, "big") + bytes.fromhex("a003020102" "0203010203" "300b0609608648016503040312")
    assert tbs[27:44] == xc.name(b"root") and tbs[76:93] == xc.name(b"leaf") and tbs[93:] == der[28:28 + 1334]
    out = cs.written(np.full(len(tbs) + 3, cs.FILL, dtype=np.uint8), want)
    assert out[:len(tbs)].tobytes() == tbs and (out[len(tbs):] == cs.FILL).all()


def test_every_defect_gives_its_documented_status_and_neighbours_are_untouched():
    batch, at = cs.defect_batch()
    fields, ops, status = batch["parse"]
    want = cs.expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 10 ** 7)
    assert set(at) == set(cs.DEFECTS) and len(status) == 9 * len(cs.DEFECTS)
    for name, i in ((name, i) for name, three in at.items() for i in three):
        assert status[i] == cs.PARSE_STATUS[name] and want["status"][i] == cs.DEFECTS[name], name
        assert status[i - 1] == status[i + 1] == want["status"][i - 1] == want["status"][i + 1] == 0, name
        assert want["reqs"][i].tobytes() == bytes(32) and i not in want["tbs"], name
        if status[i] != cs.OK:
            assert ops[i].tobytes() == bytes(40) and int(fields[i]["sig_off"]) == int(fields[i]["key_off"]) == int(fields[i]["set"]) == 0, name
        if status[i] in (cs.RANGE, cs.DER):
            assert fields[i].tobytes() == bytes(53) + bytes([status[i]]) + bytes(2), name
        elif status[i] != cs.OK:
            assert int(fields[i]["cri_len"]) > 1000 and int(fields[i]["spki_len"]) > 1000, name
        # a refused request takes no room
        assert int(want["reqs"][i + 1]["off"]) == int(want["reqs"][i - 1]["off"]) + int(want["reqs"][i - 1]["len"]), name
    assert want["totals"] == (6 * len(cs.DEFECTS), 3 * len(cs.DEFECTS), sum(len(t) for t in want["tbs"].values()))
    # once per parameter set: where stage 1 accepts, the three requests of a defect are of the three sets
    assert all([int(fields[i]["set"]) for i in three] == list(cs.SETS) for name, three in at.items() if cs.PARSE_STATUS[name] == cs.OK)
    # one byte short with the missing byte in the blob behind it; serials that are fine
    i = at["len_one_short"][0]
    off, n = int(batch["items"][i]["off"]), int(batch["items"][i]["len"])
    assert cs.walk(batch["blob"][off:off + n + 1].tobytes())["status"] == cs.OK
    der = cs.join(cs.random_parts(44, b"ser", 0))
    for s, st in ((b"\x00", cs.OK), (b"\x7f", cs.OK), (b"\x00\x80", cs.OK), (b"\x00\x7f", cs.TEMPLATE), (b"\x80", cs.TEMPLATE), (b"\x01" * 20, cs.OK)):
        assert one(der, (44, 0, s, cs.ISSUER, cs.VALIDITY, b"", None, 0))[2]["status"].tolist() == [st], s


def test_precedence_the_earlier_rule_is_reported():
    p = cs.random_parts(44, b"prec", 0)
    good = cs.template(44, 1)
    assert one(cs.join(p), good)[2]["status"].tolist() == [cs.OK]
    both = dict(p, version=xc.tlv(0x02, b"\x01"), alg=xc.alg_id(0), kalg=xc.alg_id(65), sig=xc.tlv(0x03, b"\x01"))
    steps = [("version", cs.VERSION), ("alg", cs.ALG), ("kalg", cs.KEY), ("sig", cs.SIG)]
    for k, (part, st) in enumerate(steps):  # VERSION before ALG before KEY before SIG; DER before all of them
        assert cs.walk(cs.join(both))["status"] == st, part
        assert cs.walk(cs.join(dict(both, attrs=b"")))["status"] == cs.DER
        both[part] = p[part]
    assert cs.walk(cs.join(both))["status"] == cs.OK
    # stage 2: stage 1's status, RANGE, POP, ENTRY, TEMPLATE, LONG, SPACE
    der = cs.join(p)
    bad_entry = cs.template_defect(cs.template_defect(good, "serial_len_21", 0), "issuer_wrong_tag", 0)
    long_t = cs.template(44, 1, ext=cs.ext_of_len(cs.MAX_TBS[44]))
    assert one(cs.byte_defect(p, 44, "version_01")[0], bad_entry, ok=0)[2]["status"].tolist() == [cs.VERSION]
    assert one(der, bad_entry, ok=0)[2]["status"].tolist() == [cs.POP]
    assert one(der, bad_entry)[2]["status"].tolist() == [cs.ENTRY]
    assert one(der, cs.template_defect(long_t, "issuer_wrong_tag", 0))[2]["status"].tolist() == [cs.TEMPLATE]
    assert one(der, long_t, out_len=0)[2]["status"].tolist() == [cs.LONG]
    assert one(der, good, out_len=0)[2]["status"].tolist() == [cs.SPACE] and one(der, good, out_len=0)[2]["totals"][2] > 1400


def test_edges_space_mixes_and_the_sweep_of_the_restatement():
    batch, status = cs.edge_batch()
    want = cs.expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 10 ** 7)
    assert want["status"].tolist() == status and status.count(cs.LONG) == 3 and status[-3:] == [cs.OK, cs.OK, cs.ENTRY]
    assert sorted(int(q["len"]) for q in want["reqs"])[-3:] == sorted(cs.MAX_TBS.values())
    # SPACE: the need, one byte less, nothing
    b = cs.seam_case(65, "tenth_defect", seed=3)
    free = cs.expected_tbs(b["blob"], b["fields"], b["entries"], b["ok"], 2 ** 62)
    need, last = free["totals"][2], max(free["tbs"])
    assert cs.expected_tbs(b["blob"], b["fields"], b["entries"], b["ok"], need)["status"].tolist() == free["status"].tolist()
    short = cs.expected_tbs(b["blob"], b["fields"], b["entries"], b["ok"], need - 1)
    assert [i for i in range(65) if short["status"][i] != free["status"][i]] == [last] and short["status"][last] == cs.SPACE
    assert short["totals"] == (free["totals"][0] - 1, free["totals"][1] + 1, need)
    none = cs.expected_tbs(b["blob"], b["fields"], b["entries"], b["ok"], 0)
    assert none["totals"] == (0, 65, need) and (none["status"] == cs.SPACE).sum() == len(free["tbs"])
    for mix in cs.MIXES:
        b = cs.seam_case(65, mix, seed=2)
        want = cs.expected_tbs(b["blob"], b["fields"], b["entries"], b["ok"], 10 ** 7)
        hist = np.bincount(want["status"], minlength=19)
        if mix in ("mod3", "only44", "only87"):
            assert hist[0] == 65
        elif mix == "all_defect":
            assert hist[0] == 0 and all(hist[c] > 0 for c in (cs.RANGE, cs.DER, cs.ALG, cs.SIG, cs.VERSION, cs.KEY, cs.POP, cs.ENTRY, cs.TEMPLATE))
        else:
            assert hist[0] == 65 - 6
        for i, tbs in want["tbs"].items():  # the contract: the issuing side's walk accepts every TBSCertificate for the entry's set
            assert xs.walk_tbs(tbs, int(b["entries"][i]["set"])) == xs.OK, (mix, i)
    hist = np.bincount(cs.mutation_batch()["parse"][2], minlength=14)
    assert hist.sum() == 170 * 7 and hist[cs.RANGE] == 0 and hist[cs.ALG] == 77 and hist[cs.VERSION] == 6  # (the OID's 11 bytes; the version's one, seven values but 00)
    for front in (0, 5):
        assert len(cs.alignment_batch(front)["items"]) == 256


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl on this machine to parse the DER independently")
def test_request_and_assembled_certificate_parse_with_openssl_asn1parse(tmp_path):
    for pset in cs.SETS:
        der = cs.join(cs.random_parts(pset, b"ossl", pset, cn=b"openssl", attrs=cs.ATTRS))
        row, _, want, _, _ = one(der, cs.template(pset, 4, ext=xc.extensions(33)))
        assert int(row["status"]) == 0 and want["status"].tolist() == [0]
        cert = xc.cert(want["tbs"][0], pset, xc._bytes(b"osig", pset, cs.SIG_LEN[pset]))
        for name, data, d1_want in (("r", der, 3), ("c", cert, 3)):
            path = tmp_path / ("%s%d.der" % (name, pset))
            path.write_bytes(data)
            run = subprocess.run(["openssl", "asn1parse", "-inform", "DER", "-in", str(path)], capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            d1 = [ln for ln in run.stdout.splitlines() if ":d=1 " in ln]
            assert len(d1) == d1_want and "SEQUENCE" in d1[0] and "SEQUENCE" in d1[1] and "BIT STRING" in d1[2]
            if name == "r":  # the CertificationRequestInfo openssl sees is the row's
                assert re.match(r"\s*4:d=1\s+hl=4\s+l=\s*%d\s" % (int(row["cri_len"]) - 4), d1[0])
            else:
                assert re.match(r"\s*4:d=1\s+hl=4\s+l=\s*%d\s" % (len(want["tbs"][0]) - 4), d1[0]) and "cont [ 3 ]" in run.stdout


def test_signed_requests_on_the_oracle_and_the_finished_certificate_on_the_verifying_side():
    for pset in cs.SETS:
        s = cs.signed_case(pset)
        blob, items, entries = cs.lay_out([(d, len(d), t) for d, t in zip(s["ders"], s["templates"])], pad=3)
        fields, ops, status = cs.expected_parse(blob, items)
        assert status.tolist() == [0, 0]
        raw = blob.tobytes()
        cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
        verdicts = []
        for j, op in enumerate(ops):  # the op is the proof of possession: the request's own key over its CertificationRequestInfo
            rs = int(op["set"])
            assert rs == s["req_set"] and cut(op["msg_off"], op["msg_len"]) == s["cris"][j] and cut(op["pk_off"], cs.PK_LEN[rs]) == s["pks"][j]
            verdicts.append(orc.verify_internal(rs, orc.pk_try_from_bytes(rs, s["pks"][j]), s["cris"][j], cut(op["sig_off"], cs.SIG_LEN[rs]),
                                                ctx=b"", mode=orc.MODE_PURE))
        assert verdicts == [True, False]
        want = cs.expected_tbs(blob, fields, entries, np.array(verdicts, dtype=np.uint8), 10 ** 6)
        assert want["status"].tolist() == [0, cs.POP] and list(want["tbs"]) == [0]
        tbs = want["tbs"][0]
        assert xs.walk_tbs(tbs, pset) == xs.OK
        der = xc.cert(tbs, pset, orc.sign_internal(pset, s["ca_sk"], tbs, bytes(32), ctx=b"", mode=orc.MODE_PURE))
        w = xc.walk(der)
        assert w["status"] == xc.OK and w["key_set"] == s["req_set"] and der[w["key_off"]:w["key_off"] + cs.PK_LEN[s["req_set"]]] == s["pks"][0]
        assert der[w["subject_off"]:w["subject_off"] + w["subject_len"]] == cut(fields[0]["subject_off"], fields[0]["subject_len"])
        assert der[w["issuer_off"]:w["issuer_off"] + w["issuer_len"]] == s["ca_name"]
        # under the CA certificate the verifying side's restatement accepts it, names checked
        vblob, certs = xc.lay_out([(der, len(der)), (s["ca_der"], len(s["ca_der"]))], [1, 1], pad=1)
        assert xc.expected(vblob, certs)[2].tolist() == [0, 0]


# ---- the walk, the rules and the bytes under the sanitizers -----------------------------------------------------------------------------
def _t_lines(batch, want):
    lines = ["B " + batch["blob"].tobytes().hex()]
    for i, (r, e) in enumerate(zip(batch["fields"], batch["entries"])):
        st = int(want["status"][i])
        row = [int(r[f]) for f in ("status", "subject_off", "subject_len", "spki_off", "spki_len", "key_off", "set")]
        ent = [int(e[f]) for f in ("serial_off", "issuer_off", "validity_off", "ext_off", "issuer_len", "validity_len", "ext_len", "serial_len", "set",
                                   "flags", "reserved")]
        lines.append("T %d %d %s %s %s" % (st, int(batch["ok"][i]), " ".join(map(str, row)), " ".join(map(str, ent)), want["tbs"][i].hex() if st == 0 else "-"))
    return lines


def test_the_walk_the_rules_and_the_bytes_under_asan_and_ubsan(tmp_path):
    lines = []

    def w_line(der):
        w = cs.walk(der)
        lines.append("W %d %s %s" % (w["status"], " ".join(str(w[f]) for f in ("cri_off", "cri_len", "subject_off", "subject_len", "spki_off", "spki_len",
                                                                                 "sig_off", "key_off", "set")), der.hex()))

    for pset in cs.SETS:
        p = cs.random_parts(pset, b"san", pset, attrs=cs.ATTRS)
        w_line(cs.join(p))
        w_line(cs.join(cs.random_parts(pset, b"san1", pset, cn=bytes(300))))
        for name in cs.BYTE_DEFECTS:
            data, n = cs.byte_defect(p, pset, name)
            data = (data + b"\xc3")[:n]  # (len_one_long: the byte behind the request)
            assert cs.walk(data)["status"] == cs.BYTE_DEFECTS[name], name
            w_line(data)
    m = cs.mutation_batch()  # the single-byte sweep over both windows; the expected rows are the restatement's
    for c in m["items"]:
        w_line(m["blob"][int(c["off"]):int(c["off"]) + int(c["len"])].tobytes())
    # stage 2: the defect batch (SPACE aside: every rule up to LONG) and the length edges
    batch, _ = cs.defect_batch()
    lines += _t_lines(batch, cs.expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 2 ** 62))
    batch, _ = cs.edge_batch()
    lines += _t_lines(batch, cs.expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 2 ** 62))
    kinds = {int(ln.split()[1]) for ln in lines if ln[0] == "T"}
    assert kinds == {cs.OK, cs.RANGE, cs.DER, cs.ALG, cs.SIG, cs.VERSION, cs.KEY, cs.POP, cs.ENTRY, cs.TEMPLATE, cs.LONG}
    table = tmp_path / "csr_table.txt"
    table.write_text("\n".join(lines) + "\n")
    sanitized_program(tmp_path, "csr_plan", ["csr_plan_main.cpp"], "csr_plan OK", env={"CSR_TABLE": str(table)})
