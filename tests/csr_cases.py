"""Cases for the certification-request library (include/mldsa_csr.h) and a Python restatement of what both of its stages must produce
-- the walk, the fields rows, the ops, the status of every request, the mldsa_x509sign_req rows, the totals and every byte of the output
buffer --, written from the rules the header states and not from the kernels: the TLV reader and the DER builder are
tests/x509_cases.py's (take / expect / tlv / name / alg_id), imported and not copied.  Loads no library.  Not a test file:
test_csr_cpu.py and test_gpu_csr.py import it by name."""
import functools

import numpy as np

import x509_cases as xc
import x509sign_cases as xs
from fips204_amd import _csr_lib, _rec_lib, _x509sign_lib
from fips204_amd.ml_dsa import csr_blob

SIG_LEN, PK_LEN, SETS = xc.SIG_LEN, xc.PK_LEN, xc.SETS
OK, RANGE, DER, ALG, SIG = xc.OK, xc.RANGE, xc.DER, xc.ALG, xc.SIG
VERSION, KEY, POP, ENTRY, TEMPLATE, LONG, SPACE = 12, 13, 14, 15, 16, 17, 18
FLAG_RND = 1
SERIAL_MAX = 20
MAX_TBS = xs.MAX_TBS                                   # x509sign's own LONG limit
FILL = 0x5A                                            # what the tests fill the output buffer with
SEAM_SIZES, MIXES = xc.SEAM_SIZES, xc.MIXES
_bytes = xc._bytes


# ------------------------------------------------------------------------------------------------------------------- the builder
def parts(pset, cn, pk, sig, attrs=b""):
    """the pieces of a CertificationRequest of `pset`, each a whole TLV, for join()"""
    return dict(version=xc.tlv(0x02, b"\x00"), subject=xc.name(cn), kalg=xc.alg_id(pset), key=xc.tlv(0x03, b"\x00" + bytes(pk)),
                attrs=xc.tlv(0xA0, attrs), alg=xc.alg_id(pset), sig=xc.tlv(0x03, b"\x00" + bytes(sig)), spki_extra=b"", cri_extra=b"",
                outer_tag=0x30, cri_tag=0x30, spki_tag=0x30)


def join(p):
    spki = xc.tlv(p["spki_tag"], p["kalg"] + p["key"] + p["spki_extra"])
    cri = xc.tlv(p["cri_tag"], p["version"] + p["subject"] + spki + p["attrs"] + p["cri_extra"])
    return xc.tlv(p["outer_tag"], cri + p["alg"] + p["sig"])


def cri_of(pset, cn, pk, attrs=b""):
    """the CertificationRequestInfo TLV alone: what the requester signs"""
    p = parts(pset, cn, pk, b"", attrs)
    return xc.tlv(0x30, p["version"] + p["subject"] + xc.tlv(0x30, p["kalg"] + p["key"]) + p["attrs"])


ATTRS = xc.tlv(0x30, bytes.fromhex("06092a864886f70d01090e") + xc.tlv(0x31, xc.tlv(0x30, b"")))  # an empty extensionRequest


def random_parts(pset, tag, i, cn=None, attrs=b""):
    """a request of the right shape around random key and signature bytes: what the seam needs, which verifies nothing"""
    cn = _bytes(tag + b"cn", i, (4, 1, 130, 300, 17)[i % 5]) if cn is None else cn
    return parts(pset, cn, _bytes(tag + b"pk", i, PK_LEN[pset]), _bytes(tag + b"sig", i, SIG_LEN[pset]), attrs)


# ------------------------------------------------------------------------------------------------------------------- stage 1 restated
def walk(der):
    """dict of the request's fields relative to its first byte, status among OK / DER / VERSION / ALG / KEY / SIG"""
    out = dict(cri_off=0, cri_len=0, sig_off=0, key_off=0, subject_off=0, subject_len=0, spki_off=0, spki_len=0, set=0, status=DER)
    n = len(der)
    try:
        at, behind = xc.expect(der, 0, n, 0x30)
        if behind != n:
            raise xc.Malformed("bytes behind the request")
        cri_at, cri_end = xc.expect(der, at, n, 0x30)
        alg_at, alg_end = xc.expect(der, cri_end, n, 0x30)
        sig_at, sig_end = xc.expect(der, alg_end, n, 0x03)
        if sig_end != n:
            raise xc.Malformed("bytes behind the signature")
        ver_at, ver_end = xc.expect(der, cri_at, cri_end, 0x02)
        sub_end = xc.expect(der, ver_end, cri_end, 0x30)[1]
        spki_at, spki_end = xc.expect(der, sub_end, cri_end, 0x30)
        kalg_at, kalg_end = xc.expect(der, spki_at, spki_end, 0x30)
        key_at, key_end = xc.expect(der, kalg_end, spki_end, 0x03)
        if key_end != spki_end:
            raise xc.Malformed("bytes behind the key")
        if xc.expect(der, spki_end, cri_end, 0xA0)[1] != cri_end:
            raise xc.Malformed("bytes behind the attributes")
    except xc.Malformed:
        return out
    out.update(cri_off=at, cri_len=cri_end - at, subject_off=ver_end, subject_len=sub_end - ver_end, spki_off=sub_end, spki_len=spki_end - sub_end)
    if bytes(der[ver_at:ver_end]) != b"\x00":
        out["status"] = VERSION
        return out
    pset = xc.set_of_oid(der[alg_at:alg_end])
    if not pset:
        out["status"] = ALG
        return out
    if der[kalg_at:kalg_end] != der[alg_at:alg_end] or key_end - key_at != 1 + PK_LEN[pset] or der[key_at] != 0:
        out["status"] = KEY
        return out
    if sig_end - sig_at != 1 + SIG_LEN[pset] or der[sig_at] != 0:
        out["status"] = SIG
        return out
    out.update(status=OK, set=pset, sig_off=sig_at + 1, key_off=key_at + 1)
    return out


def expected_parse(blob, items):
    """(fields [n] of _csr_lib.FIELDS_DTYPE, ops [n] of _rec_lib.OP_DTYPE, status uint8 [n]) for a blob (uint8 array) and its items"""
    raw = blob.tobytes()
    n = len(items)
    fields = np.zeros(n, dtype=_csr_lib.FIELDS_DTYPE)
    ops = np.zeros(n, dtype=_rec_lib.OP_DTYPE)
    for i, c in enumerate(items):
        off, length = int(c["off"]), int(c["len"])
        if not xc.inside(off, length, len(raw)) or length < 2:
            fields[i]["status"] = RANGE
            continue
        w = walk(raw[off:off + length])
        fields[i]["status"] = w["status"]
        if w["status"] == DER:
            continue
        for f in ("cri_len", "subject_len", "spki_len"):
            fields[i][f] = w[f]
        for f in ("cri_off", "subject_off", "spki_off"):
            fields[i][f] = off + w[f]
        if w["status"] == OK:
            fields[i]["set"], fields[i]["sig_off"], fields[i]["key_off"] = w["set"], off + w["sig_off"], off + w["key_off"]
            ops[i]["pk_off"], ops[i]["sig_off"], ops[i]["set"] = fields[i]["key_off"], fields[i]["sig_off"], w["set"]
            ops[i]["msg_off"], ops[i]["msg_len"] = fields[i]["cri_off"], w["cri_len"]
    return fields, ops, fields["status"].copy()


# ------------------------------------------------------------------------------------------------------------------- stage 2 restated
def _one_tlv(raw, off, length, tag):
    try:
        return xc.expect(raw, off, off + length, tag)[1] == off + length
    except xc.Malformed:
        return False


def pieces_len(row, e):
    return 24 + int(e["serial_len"]) + int(e["issuer_len"]) + int(e["validity_len"]) + int(row["subject_len"]) + int(row["spki_len"]) + int(e["ext_len"])


def status_before_space(raw, row, e, ok):
    """the first rule of stage 2 a request breaks, up to LONG: Python integers, so nothing wraps"""
    if int(row["status"]) != OK:
        return int(row["status"])
    n = len(raw)
    if not xc.inside(int(row["subject_off"]), int(row["subject_len"]), n) or not xc.inside(int(row["spki_off"]), int(row["spki_len"]), n):
        return RANGE
    if int(ok) != 1:
        return POP
    pset, sl = int(e["set"]), int(e["serial_len"])
    if pset not in SETS or int(e["flags"]) & ~FLAG_RND or int(e["reserved"]) != 0 or not 1 <= sl <= SERIAL_MAX:
        return ENTRY
    so, io, il, vo, vl, eo, el = (int(e[f]) for f in ("serial_off", "issuer_off", "issuer_len", "validity_off", "validity_len", "ext_off", "ext_len"))
    if not xc.inside(so, sl, n) or not xc.inside(io, il, n) or not xc.inside(vo, vl, n) or (el > 0 and not xc.inside(eo, el, n)):
        return TEMPLATE
    if not _one_tlv(raw, io, il, 0x30) or not _one_tlv(raw, vo, vl, 0x30) or (el > 0 and not _one_tlv(raw, eo, el, 0xA3)):
        return TEMPLATE
    if raw[so] >= 0x80 or (sl > 1 and raw[so] == 0 and raw[so + 1] < 0x80):
        return TEMPLATE
    if pieces_len(row, e) > MAX_TBS[pset]:
        return LONG
    return OK


def tbs_bytes(raw, row, e):
    """the TBSCertificate of a request that passed status_before_space, by the header's picture"""
    cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
    body = (xc.VERSION + xc.tlv(0x02, cut(e["serial_off"], e["serial_len"])) + xc.alg_id(int(e["set"])) + cut(e["issuer_off"], e["issuer_len"]) +
            cut(e["validity_off"], e["validity_len"]) + cut(row["subject_off"], row["subject_len"]) + cut(row["spki_off"], row["spki_len"]) +
            (cut(e["ext_off"], e["ext_len"]) if int(e["ext_len"]) else b""))
    out = b"\x30\x82" + len(body).to_bytes(2, "big") + body
    assert len(out) == pieces_len(row, e) and (len(body) < 256 or out == xc.tlv(0x30, body))
    return out


def expected_tbs(blob, fields, entries, ok, out_len):
    """dict(status uint8 [n], reqs [n] of _x509sign_lib.REQ_DTYPE, totals (accepted, refused, out_bytes), tbs {i: the TBSCertificate})"""
    raw = blob.tobytes()
    n = len(entries)
    status = np.zeros(n, dtype=np.uint8)
    reqs = np.zeros(n, dtype=_x509sign_lib.REQ_DTYPE)
    tbs, at = {}, 0
    for i in range(n):
        status[i] = status_before_space(raw, fields[i], entries[i], ok[i])
        if status[i] != OK:
            continue
        need = pieces_len(fields[i], entries[i])
        if at + need > out_len:
            status[i] = SPACE
        else:
            tbs[i] = tbs_bytes(raw, fields[i], entries[i])
            e = entries[i]
            reqs[i] = (at, e["rnd_off"], need, e["key"], e["issuer"], e["set"], e["flags"], 0)
        at += need  # the need counts every request that passes every rule but SPACE
    accepted = int((status == OK).sum())
    return dict(status=status, reqs=reqs, totals=(accepted, n - accepted, at), tbs=tbs)


def written(before, want):
    """`before` (uint8 array, the output buffer) with every accepted request's TBSCertificate written"""
    out = np.array(before, dtype=np.uint8, copy=True)
    for i, t in want["tbs"].items():
        at = int(want["reqs"][i]["off"])
        out[at:at + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return out


def tbs_len(pset, serial_len, issuer_len, validity_len, subject_len, spki_len, ext_len):
    """mldsa_csr_tbs_len as the header spells it"""
    total = 4 + 20 + serial_len + issuer_len + validity_len + subject_len + spki_len + ext_len
    return total if pset in SETS and 1 <= serial_len <= SERIAL_MAX and total <= MAX_TBS[pset] else 0


def plan_bytes(n):
    """mldsa_csr_plan_bytes as the header spells it"""
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r(16 * ((n + 255) // 256)) + r(4 * n)


# ------------------------------------------------------------------------------------------------------------------- templates
ISSUER = xc.name(b"csr test CA")
VALIDITY = xc.VALIDITY


def serial(i, n=None):
    """a valid serial number content of n bytes (1 ... 20; by default cycling with i): positive and minimal"""
    n = 1 + i % SERIAL_MAX if n is None else n
    return bytes([0x1A + i % 0x60]) + _bytes(b"serial", i, n - 1)


def template(pset, i, ext=None, rnd=False, issuer=None):
    """(pset, key_row, serial, issuer Name, Validity, extensions, rnd, issuer) of request i: a template every rule accepts"""
    ext = (xc.extensions(3 + i % 40) if i % 3 else b"") if ext is None else ext
    return (pset, i % 4, serial(i), ISSUER, VALIDITY, ext, _bytes(b"trnd", i, 32) if rnd else None, i if issuer is None else issuer)


def ext_of_len(target):
    """an [3] extensions TLV of exactly `target` bytes (tens of kilobytes: every nested length is of the 0x82 form)"""
    ext = xc.extensions(40000 + target - len(xc.extensions(40000)))
    assert len(ext) == target
    return ext


# ------------------------------------------------------------------------------------------------------------------- defects
# stage 1, of the request's bytes: name -> status (which stage 2 hands on)
POSITIONS = ("outer", "cri", "alg", "sig", "version", "subject", "spki", "kalg", "key", "attrs")
BYTE_DEFECTS = {
    **{"wrong_tag_" + part: DER for part in POSITIONS},
    "indefinite_length": DER, "nonminimal_81_7f": DER, "nonminimal_82_00": DER, "length_85": DER, "high_tag_number": DER, "cri_overruns": DER,
    "trailing_byte": DER, "len_one_short": DER, "len_one_long": DER, "spki_trailing": DER, "attrs_missing": DER, "attrs_not_last": DER,
    "version_01": VERSION, "version_two_bytes": VERSION, "outer_null_params": ALG, "outer_rsa": ALG, "outer_other_set": KEY,
    "spki_other_set": KEY, "spki_null_params": KEY, "spki_rsa": KEY, "key_one_short": KEY, "key_unused_bits": KEY, "sig_one_short": SIG,
    "sig_unused_bits": SIG,
}
# stage 1, of the item: name -> status
ITEM_DEFECTS = {"off_wraps": RANGE, "len_zero": RANGE, "len_one": RANGE, "ends_one_past_blob": RANGE, "off_behind_blob": RANGE}
# stage 2, of the template's bytes: name -> status (the request itself is accepted by stage 1)
TEMPLATE_DEFECTS = {"issuer_wrong_tag": TEMPLATE, "issuer_nonminimal": TEMPLATE, "validity_wrong_tag": TEMPLATE, "ext_wrong_tag": TEMPLATE,
                    "serial_negative": TEMPLATE, "serial_ff": TEMPLATE, "serial_not_minimal": TEMPLATE, "serial_00_00": TEMPLATE,
                    "serial_len_21": ENTRY, "serial_len_0": ENTRY}
# stage 2, of the entry, the verdict and the row, applied once the blob is laid out: name -> status
ENTRY_DEFECTS = {"pop_0": POP, "pop_2": POP, "pop_ff": POP, "unknown_set": ENTRY, "flag_bit_1": ENTRY, "reserved": ENTRY,
                 "serial_off_wraps": TEMPLATE, "serial_ends_past_blob": TEMPLATE, "issuer_off_wraps": TEMPLATE, "issuer_one_short": TEMPLATE,
                 "issuer_one_long": TEMPLATE, "issuer_len_1": TEMPLATE, "validity_behind_blob": TEMPLATE, "validity_one_short": TEMPLATE,
                 "ext_off_wraps": TEMPLATE, "ext_one_long": TEMPLATE, "row_subject_wraps": RANGE, "row_spki_past_blob": RANGE,
                 "row_status_der": DER}
DEFECTS = {**BYTE_DEFECTS, **ITEM_DEFECTS, **TEMPLATE_DEFECTS, **ENTRY_DEFECTS}
# what stage 1 says of each: its own defects' status, OK for stage 2's
PARSE_STATUS = {**BYTE_DEFECTS, **ITEM_DEFECTS, **{name: OK for name in {**TEMPLATE_DEFECTS, **ENTRY_DEFECTS}}}


def _retag(part, tag):
    return bytes([tag]) + part[1:]


def byte_defect(p, pset, name):
    """(bytes to lay into the blob, the len to declare for them) of the request join(p) with one of BYTE_DEFECTS.  For len_one_long the
    caller sees to it that one more byte lies behind the request in the blob."""
    p = dict(p)
    der = join(p)
    n = len(der)
    other = SETS[(SETS.index(pset) + 1) % 3]
    if name.startswith("wrong_tag_"):
        part = name[len("wrong_tag_"):]
        if part in ("outer", "cri", "spki"):
            p[part + "_tag"] = 0x31
        else:
            p[part] = _retag(p[part], {"version": 0x04, "key": 0x04, "sig": 0x04, "attrs": 0xA1}.get(part, 0x31))
    elif name == "indefinite_length":
        return der[:1] + b"\x80" + der[2:], n
    elif name == "nonminimal_81_7f":      # attributes of 127 bytes behind 81 7F
        p["attrs"] = b"\xa0\x81\x7f" + xc.tlv(0x30, bytes(125))
    elif name == "nonminimal_82_00":      # the subject Name behind 82 00 xx
        body = p["subject"][xc.take(p["subject"], 0, len(p["subject"]))[1]:]
        p["subject"] = (b"\x30\x82\x00" + bytes([len(body)]) if len(body) < 256 else b"\x30\x83\x00" + len(body).to_bytes(2, "big")) + body
    elif name == "length_85":
        p["version"] = b"\x02\x85\x00\x00\x00\x00\x01\x00"
    elif name == "high_tag_number":
        p["subject"] = _retag(p["subject"], 0x3F)
    elif name == "cri_overruns":          # the CertificationRequestInfo claims the whole rest of the request and one byte more
        at = xc.take(der, 0, n)[1]
        assert der[at + 1] == 0x82
        return der[:at + 2] + (n - at - 4 + 1).to_bytes(2, "big") + der[at + 4:], n
    elif name == "trailing_byte":
        return der + b"\x00", n + 1
    elif name == "len_one_short":
        return der, n - 1
    elif name == "len_one_long":
        return der, n + 1
    elif name == "spki_trailing":
        p["spki_extra"] = b"\x05\x00"
    elif name == "attrs_missing":
        p["attrs"] = b""
    elif name == "attrs_not_last":
        p["cri_extra"] = b"\x05\x00"
    elif name == "version_01":
        p["version"] = xc.tlv(0x02, b"\x01")
    elif name == "version_two_bytes":
        p["version"] = xc.tlv(0x02, b"\x00\x00")
    elif name == "outer_null_params":
        p["alg"] = xc.tlv(0x30, xc.OID[pset] + b"\x05\x00")
    elif name == "outer_rsa":
        p["alg"] = xc.alg_id(0)
    elif name == "outer_other_set":
        p["alg"] = xc.alg_id(other)
    elif name == "spki_other_set":
        p["kalg"] = xc.alg_id(other)
    elif name == "spki_null_params":
        p["kalg"] = xc.tlv(0x30, xc.OID[pset] + b"\x05\x00")
    elif name == "spki_rsa":
        p["kalg"] = xc.alg_id(0)
    elif name == "key_one_short":
        p["key"] = xc.tlv(0x03, p["key"][4:-1])
    elif name == "key_unused_bits":
        p["key"] = p["key"][:4] + b"\x01" + p["key"][5:]
    elif name == "sig_one_short":
        p["sig"] = xc.tlv(0x03, p["sig"][4:-1])
    elif name == "sig_unused_bits":
        p["sig"] = p["sig"][:4] + b"\x01" + p["sig"][5:]
    else:
        raise KeyError(name)
    out = join(p)
    return out, len(out)


def item_defect(items, i, name, blob_len):
    c = items[i]
    if name == "off_wraps":
        c["off"] = 2 ** 64 - 8
    elif name == "len_zero":
        c["len"] = 0
    elif name == "len_one":
        c["len"] = 1
    elif name == "ends_one_past_blob":
        c["off"] = blob_len + 1 - int(c["len"])
    elif name == "off_behind_blob":
        c["off"], c["len"] = blob_len + 1, 2
    else:
        raise KeyError(name)


def template_defect(t, name, i):
    """the template t with one of TEMPLATE_DEFECTS"""
    t = list(t)
    if name == "issuer_wrong_tag":
        t[3] = _retag(t[3], 0x31)
    elif name == "issuer_nonminimal":
        t[3] = b"\x30\x81" + t[3][1:]
    elif name == "validity_wrong_tag":
        t[4] = _retag(t[4], 0x31)
    elif name == "ext_wrong_tag":
        t[5] = _retag(xc.extensions(7 + i % 9), 0x30)
    elif name == "serial_negative":
        t[2] = b"\x80" + _bytes(b"sneg", i, i % 5)
    elif name == "serial_ff":
        t[2] = b"\xff"
    elif name == "serial_not_minimal":
        t[2] = b"\x00\x7f" + _bytes(b"smin", i, i % 3)
    elif name == "serial_00_00":
        t[2] = b"\x00\x00\x80"
    elif name == "serial_len_21":
        t[2] = serial(i, 1) + bytes(20)
    elif name == "serial_len_0":
        t[2] = b""
    else:
        raise KeyError(name)
    return tuple(t)


def entry_defect(entries, fields, ok, i, name, blob_len):
    """damages entry i, its verdict or its row with one of ENTRY_DEFECTS"""
    e, r = entries[i], fields[i]
    if name.startswith("pop_"):
        ok[i] = {"pop_0": 0, "pop_2": 2, "pop_ff": 0xFF}[name]
    elif name == "unknown_set":
        e["set"] = (43, 0, 66, 255)[i % 4]
    elif name == "flag_bit_1":
        e["flags"] = int(e["flags"]) | (2, 0x80)[i % 2]
    elif name == "reserved":
        e["reserved"] = 1 + i % 255
    elif name == "serial_off_wraps":
        e["serial_off"] = 2 ** 64 - 4
    elif name == "serial_ends_past_blob":
        e["serial_off"] = blob_len + 1 - int(e["serial_len"])
    elif name == "issuer_off_wraps":
        e["issuer_off"] = 2 ** 64 - 8
    elif name == "issuer_one_short":
        e["issuer_len"] = int(e["issuer_len"]) - 1
    elif name == "issuer_one_long":
        e["issuer_len"] = int(e["issuer_len"]) + 1
    elif name == "issuer_len_1":
        e["issuer_len"] = 1
    elif name == "validity_behind_blob":
        e["validity_off"] = blob_len + 1
    elif name == "validity_one_short":
        e["validity_len"] = int(e["validity_len"]) - 1
    elif name == "ext_off_wraps":
        e["ext_off"], e["ext_len"] = 2 ** 64 - 16, 32
    elif name == "ext_one_long":
        e["ext_off"], e["ext_len"] = e["issuer_off"], int(e["issuer_len"]) + 1
    elif name == "row_subject_wraps":
        r["subject_off"] = 2 ** 64 - 2
    elif name == "row_spki_past_blob":
        r["spki_off"] = blob_len + 1 - int(r["spki_len"])
    elif name == "row_status_der":
        r["status"] = DER
    else:
        raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------- batches
def lay_out(cases, pad=0, front=0):
    """(blob, items, entries) for cases (request bytes, declared len, template), with 40 spare bytes behind the last piece"""
    blob, items, entries = csr_blob([c[0] for c in cases], [c[2] for c in cases], pad=pad, front=front)
    for i, c in enumerate(cases):
        items[i]["len"] = c[1]
    return np.concatenate([blob, np.full(40, 0xC3, dtype=np.uint8)]), items, entries


def _case(pset, tag, i, defect=None, rnd=False):
    """one case and the name of a defect to apply once the blob is laid out (or None)"""
    p = random_parts(pset, tag, i, attrs=ATTRS if i % 2 else b"")
    der, length = byte_defect(p, pset, defect) if defect in BYTE_DEFECTS else (join(p), None)
    t = template(SETS[(SETS.index(pset) + i) % 3], i, rnd=rnd)
    if defect in TEMPLATE_DEFECTS:
        t = template_defect(t, defect, i)
    return (der, len(der) if length is None else length, t), defect if defect in ITEM_DEFECTS or defect in ENTRY_DEFECTS else None


def finish(cases, late, pad, front):
    """dict(blob, items, entries, ok, fields, parse): the batch laid out and the item defects applied; parse = what stage 1 must give
    (fields, ops, status); ok = 1 wherever stage 1 accepts; then the entry defects applied to the entries, to ok and to `fields`, a copy of
    stage 1's rows: what stage 2 is given"""
    blob, items, entries = lay_out(cases, pad=pad, front=front)
    for i, name in late:
        if name in ITEM_DEFECTS:
            item_defect(items, i, name, blob.size)
    parse = expected_parse(blob, items)
    fields, ok = parse[0].copy(), (parse[2] == OK).astype(np.uint8)
    for i, name in late:
        if name in ENTRY_DEFECTS:
            entry_defect(entries, fields, ok, i, name, blob.size)
    return dict(blob=blob, items=items, entries=entries, ok=ok, fields=fields, parse=parse)


def defect_batch():
    """(batch, {defect: its three indices}): every defect once per parameter set, each time between two valid neighbours.
    batch["fields"] holds stage 1's rows with the row defects applied; batch["parse"] what stage 1 must give."""
    cases, at, late = [], {name: [] for name in DEFECTS}, []
    for k, name in enumerate(DEFECTS):
        for pset in SETS:
            for j in range(3):
                case, after = _case(pset, b"def", len(cases), name if j == 1 else None, rnd=bool(k % 2))
                cases.append(case)
                if after:
                    late.append((len(cases) - 1, after))
            at[name].append(len(cases) - 2)
    return finish(cases, late, [0, 3, 8, 13, 5], 2), at


def seam_case(n, mix, seed=0, front=0):
    """a batch of n requests, the gaps cycling 0 ... 15, every third template hedged, Names and extensions of varying length; with
    all_defect / tenth_defect every / every tenth request carries one of DEFECTS in turn"""
    names = list(DEFECTS)
    cases, late = [], []
    for i in range(n):
        pset = {"only44": 44, "only87": 87}.get(mix, SETS[i % 3])
        defect = names[(i + seed) % len(names)] if mix == "all_defect" or (mix == "tenth_defect" and i % 10 == 9) else None
        case, after = _case(pset, b"seam%d" % seed, i, defect, rnd=i % 3 == 0)
        cases.append(case)
        if after:
            late.append((i, after))
    return finish(cases, late, list(range(16)), front)


@functools.lru_cache(maxsize=None)
def mutation_batch():
    """a batch: one ML-DSA-44 request with each byte of two windows -- its first xc.MUTATION_SPAN bytes, and the 40 bytes that begin at
    the SPKI's end: the attributes, the outer algorithm and the BIT STRING's header -- set to each of xc.MUTATION_VALUES.  Every status of
    stage 1 but RANGE occurs."""
    der = join(random_parts(44, b"mut", 0, cn=b"mut", attrs=b""))
    w = walk(der)
    second = w["spki_off"] + w["spki_len"]
    cases = []
    for pos in list(range(xc.MUTATION_SPAN)) + list(range(second, second + 40)):
        for v in xc.MUTATION_VALUES:
            cases.append((der[:pos] + bytes([v]) + der[pos + 1:], len(der), template(44, len(cases))))
    batch = finish(cases, [], [3, 0, 7], 0)
    assert set(batch["parse"][2].tolist()) == {OK, DER, VERSION, ALG, KEY, SIG}
    return batch


@functools.lru_cache(maxsize=None)
def alignment_batch(front=0):
    """an ML-DSA-44 batch in which each of the 256 pairs (the SPKI's blob offset mod 16, its offset in the output buffer mod 16) occurs:
    request i's gap in the blob gives the first, its serial_len the second; subject lengths vary, and every serial_len 1 ... 20 occurs"""
    cases, pads, at, pairs, lens = [], [], 0, set(), set()
    blob_at = front
    for i in range(256):
        src, dst = i % 16, i // 16
        p = random_parts(44, b"align", i, cn=_bytes(b"acn", i, 1 + i % 23))
        der = join(p)
        w = walk(der)
        gap = (src - (blob_at + w["spki_off"])) % 16
        fixed = at + 24 + len(ISSUER) + len(VALIDITY) + w["subject_len"]
        sl = (dst - fixed) % 16 or 16
        if sl <= 4 and i % 2:
            sl += 16
        t = template(44, i, ext=xc.extensions(i % 9) if i % 4 == 1 else b"")
        t = t[:2] + (serial(i, sl),) + t[3:]
        cases.append((der, len(der), t))
        pads.append(gap)
        pairs.add(((blob_at + gap + w["spki_off"]) % 16, (fixed + sl) % 16))
        lens.add(sl)
        blob_at += gap + len(der)
        at += 24 + sl + len(ISSUER) + len(VALIDITY) + w["subject_len"] + w["spki_len"] + len(t[5])
    batch = finish(cases, [], pads + [0] * 64, front)
    assert len(pairs) == 256 and lens == set(range(1, 21))
    want = expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 2 ** 62)
    got = {(int(r["spki_off"]) % 16, (int(q["off"]) + 24 + int(e["serial_len"]) + int(e["issuer_len"]) + int(e["validity_len"]) +
                                     int(r["subject_len"])) % 16) for r, q, e in zip(batch["fields"], want["reqs"], batch["entries"])}
    assert not want["status"].any() and got == pairs
    return batch


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(batch, want status): per set a TBSCertificate of exactly x509sign's MAX_TBS and one of a byte more, driven by ext_len, small ones
    between them; then serial_len 1, 20 and 21"""
    cases, status = [], []
    for pset in SETS:
        p = random_parts(44, b"edge", pset, cn=b"edge")
        w = walk(join(p))
        rest = 24 + 1 + len(ISSUER) + len(VALIDITY) + w["subject_len"] + w["spki_len"]
        for extra in (0, 1):
            t = template(pset, 0, ext=ext_of_len(MAX_TBS[pset] - rest + extra))
            cases.append((join(p), len(join(p)), t[:2] + (b"\x05",) + t[3:]))
            cases.append(_case(pset, b"edge-s", len(cases))[0])
            status += [LONG if extra else OK, OK]
    for sl, st in ((1, OK), (20, OK), (21, ENTRY)):
        c = _case(44, b"edge-sl", sl)[0]
        cases.append(c[:2] + (c[2][:2] + (serial(sl, 1) + bytes(sl - 1),) + c[2][3:],))
        status.append(st)
    return finish(cases, [], [5, 0, 11], 0), status


# ------------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def signed_case(pset):
    """dict for the end-to-end test of one set: a CA key and its self-signed certificate, two requests signed by the oracle under their
    own keys -- the second with a damaged signature --, the templates (deterministic, issuer Name = the CA certificate's subject) and
    the oracle's signature over the TBSCertificate the restatement assembles for the first"""
    from oracle import oracle as orc
    ca_pk, ca_sk = orc.keygen_from_seed(pset, _bytes(b"csr-ca", pset, 32))
    ca_name = b"csr CA %d" % pset
    ca_tbs = xc.tbs(pset, pset, ca_name, ca_name, orc.pk_into_bytes(pset, ca_pk))
    ca_der = xc.cert(ca_tbs, pset, orc.sign_internal(pset, ca_sk, ca_tbs, bytes(32), ctx=b"", mode=orc.MODE_PURE))
    req_set = SETS[(SETS.index(pset) + 1) % 3]  # the requester's key is of another set than the CA's
    ders, cris, pks = [], [], []
    for j in range(2):
        pk, sk = orc.keygen_from_seed(req_set, _bytes(b"csr-req%d" % pset, j, 32))
        pkb = orc.pk_into_bytes(req_set, pk)
        cri = cri_of(req_set, b"requester %d" % j, pkb, ATTRS)
        sig = orc.sign_internal(req_set, sk, cri, _bytes(b"csr-rnd", j, 32), ctx=b"", mode=orc.MODE_PURE)
        assert orc.verify_internal(req_set, pk, cri, sig, ctx=b"", mode=orc.MODE_PURE)
        if j == 1:
            sig = sig[:100] + bytes([sig[100] ^ 0x10]) + sig[101:]
        ders.append(join(parts(req_set, b"requester %d" % j, pkb, sig, ATTRS)))
        cris.append(cri)
        pks.append(pkb)
    templates = [(pset, 0, serial(40 + j, 9), xc.name(ca_name), xc.VALIDITY, xc.extensions(11), None, 2) for j in range(2)]
    return dict(ca_der=ca_der, ca_sk=ca_sk, ca_pk=ca_pk, ca_seed=_bytes(b"csr-ca", pset, 32), ders=ders, cris=cris, pks=pks, req_set=req_set,
                templates=templates, ca_name=xc.name(ca_name))
