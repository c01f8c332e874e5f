"""Cases for the revocation-list library (include/mldsa_crl.h): a minimal DER builder for CertificateLists on the certificate cases'
tlv / name / alg_id, the list of defects the header names, and a Python restatement of what the library must produce -- walk_crl,
walk_entry, the placement, the link rule, the hash and the lookup --, written from the rules the header states and not from the kernels.
Loads no library.  Not a test file: test_crl_cpu.py and test_gpu_crl.py import it by name."""
import numpy as np

import x509_cases as xc
from fips204_amd import _crl_lib, _rec_lib, _x509_lib
from fips204_amd.ml_dsa import certificates_blob
from x509_cases import DER, Malformed, OK, RANGE, ALG, SIG, ISSUER, NAME, SETS, SIG_LEN, _bytes, alg_id, expect, name, take, tlv

VERSION, ENTRY, SPACE = 19, 20, 21
GOOD, REVOKED, NO_CRL, CRL_INDEX, CRL_REFUSED, CERT, SCOPE = range(7)
CHECK_NAMES = 1
NONE = 0xFFFFFFFF
SERIAL_MAX = 20
ENTRY_MIN = 20
TIME_MIN = 13
TIMES = (0x17, 0x18)
UTC = tlv(0x17, b"250101000000Z")
GENERALIZED = tlv(0x18, b"20500101000000Z")
V2 = tlv(0x02, b"\x01")
ENTRY_COUNTS = (0, 1, 63, 64, 65, 130)
SEAM_SIZES = xc.SEAM_SIZES


# ----------------------------------------------------------------------------------------------------------------------- the builder
def entry(serial, date=UTC, ext=None):
    """one revoked entry: userCertificate (the INTEGER's content bytes as given), revocationDate, crlEntryExtensions with `ext` as content"""
    return tlv(0x30, tlv(0x02, serial) + date + (b"" if ext is None else tlv(0x30, ext)))


def reason(code=1):
    """the content of a crlEntryExtensions: one reasonCode extension"""
    return tlv(0x30, bytes.fromhex("0603551d15") + tlv(0x04, tlv(0x0A, bytes([code]))))


def crl_number(n=7):
    """the content of crlExtensions: one cRLNumber extension"""
    return tlv(0x30, bytes.fromhex("0603551d14") + tlv(0x04, tlv(0x02, bytes([n]))))


def parts(sig_set, issuer_cn, entries, sig, v2=True, next_update=True, ext=b"default"):
    """the pieces of a CRL, each a bytes object (whole TLVs; `entries` a list of them, None: revokedCertificates absent): what join()
    concatenates and the defect makers change"""
    if ext == b"default":
        ext = crl_number() if v2 else None
    return dict(version=V2 if v2 else b"", inner=alg_id(sig_set), issuer=name(issuer_cn), this=UTC, next=GENERALIZED if next_update else b"",
                entries=None if entries is None else list(entries), ext=b"" if ext is None else tlv(0xA0, tlv(0x30, ext)),
                outer=alg_id(sig_set), sig_bits=b"\x00" + bytes(sig), tbs_extra=b"", list_extra=b"", revoked_extra=b"", revoked_tag=0x30)


def tbs_of(p):
    revoked = b"" if p["entries"] is None else bytes([p["revoked_tag"]]) + tlv(0x30, b"".join(p["entries"]) + p["revoked_extra"])[1:]
    return tlv(0x30, p["version"] + p["inner"] + p["issuer"] + p["this"] + p["next"] + revoked + p["ext"] + p["tbs_extra"])


def join(p):
    return tlv(0x30, p.get("tbs_raw", tbs_of(p)) + p["outer"] + p.get("sig_raw", tlv(0x03, p["sig_bits"])) + p["list_extra"])


def serial_of(tag, i, k):
    """a minimally encoded serial of 1 ... 20 bytes, the k-th of CRL i: lengths cycle, positive and negative ones alternate"""
    n = 1 + (k * 7 + i) % SERIAL_MAX
    raw = bytearray(_bytes(tag + b"serial%d" % i, k, n))
    if n >= 2 and ((raw[0] == 0x00 and raw[1] < 0x80) or (raw[0] == 0xFF and raw[1] >= 0x80)):
        raw[0] = 0x17
    return bytes(raw)


def random_entries(tag, i, count):
    """`count` entries with serials of every length, UTCTime and GeneralizedTime dates, every third with a reason code"""
    return [entry(serial_of(tag, i, k), UTC if k % 2 else GENERALIZED, reason(k % 9) if k % 3 == 0 else None) for k in range(count)]


def random_parts(sig_set, issuer_cn, tag, i, count, **kw):
    """a CRL of the right shape around random signature bytes: what the seam needs, which verifies nothing.  count = 0: no list."""
    return parts(sig_set, issuer_cn, random_entries(tag, i, count) if count else None, _bytes(tag + b"sig", i, SIG_LEN[sig_set]), **kw)


def random_crl(sig_set, issuer_cn, tag, i, count, **kw):
    return join(random_parts(sig_set, issuer_cn, tag, i, count, **kw))


def cert_with_serial(sig_set, key_set, issuer_cn, subject_cn, serial, tag, i, v3=True):
    """xc.random_cert with a serial of the caller's"""
    pk = _bytes(tag + b"pk", i, xc.PK_LEN.get(key_set, 270))
    spki = tlv(0x30, alg_id(key_set) + tlv(0x03, b"\x00" + pk))
    body = tlv(0x30, (xc.VERSION if v3 else b"") + tlv(0x02, serial) + alg_id(sig_set) + name(issuer_cn) + xc.VALIDITY + name(subject_cn) + spki)
    return xc.cert(body, sig_set, _bytes(tag + b"sig", i, SIG_LEN[sig_set]))


# ------------------------------------------------------------------------------------------------------------------- the restatement
def serial_ok(content):
    if not 1 <= len(content) <= SERIAL_MAX:
        return False
    if len(content) >= 2 and ((content[0] == 0x00 and content[1] < 0x80) or (content[0] == 0xFF and content[1] >= 0x80)):
        return False
    return True


def walk_crl(der):
    """dict of the CRL's fields relative to its first byte, status among OK / DER / ALG / SIG / VERSION / ENTRY"""
    out = dict(tbs_off=0, tbs_len=0, sig_off=0, issuer_off=0, issuer_len=0, this_off=0, next_off=0, revoked_off=0, revoked_len=0, ext_off=0,
               ext_len=0, sig_set=0, status=DER)
    n = len(der)
    try:
        at, behind = expect(der, 0, n, 0x30)
        if behind != n:
            raise Malformed("bytes behind the list")
        tbs_at, tbs_end = expect(der, at, n, 0x30)
        alg_at, alg_end = expect(der, tbs_end, n, 0x30)
        sig_at, sig_end = expect(der, alg_end, n, 0x03)
        if sig_end != n:
            raise Malformed("bytes behind the signature")
        pos, version = tbs_at, None
        tag, a, b = take(der, pos, tbs_end)
        if tag == 0x02:
            version, pos = der[a:b], b
        inner = (pos, expect(der, pos, tbs_end, 0x30)[1])
        issuer = (inner[1], expect(der, inner[1], tbs_end, 0x30)[1])
        this_off = issuer[1]
        tag, a, pos = take(der, this_off, tbs_end)
        if tag not in TIMES:
            raise Malformed("thisUpdate is no Time")
        next_off, revoked, ext = 0, None, None
        if pos < tbs_end and take(der, pos, tbs_end)[0] in TIMES:
            next_off, pos = pos, take(der, pos, tbs_end)[2]
        if pos < tbs_end and take(der, pos, tbs_end)[0] == 0x30:
            _, a, b = take(der, pos, tbs_end)
            revoked, pos = (a, b), b
        if pos < tbs_end and take(der, pos, tbs_end)[0] == 0xA0:
            _, a, b = take(der, pos, tbs_end)
            ea, eb = expect(der, a, b, 0x30)
            if eb != b:
                raise Malformed("bytes behind the extensions")
            ext, pos = (ea, eb), b
        if pos != tbs_end:
            raise Malformed("a field that belongs nowhere")
    except Malformed:
        return out
    out.update(tbs_off=at, tbs_len=tbs_end - at, issuer_off=issuer[0], issuer_len=issuer[1] - issuer[0], this_off=this_off, next_off=next_off)
    if revoked:
        out.update(revoked_off=revoked[0], revoked_len=revoked[1] - revoked[0])
    if ext:
        out.update(ext_off=ext[0], ext_len=ext[1] - ext[0])
    sset = xc.set_of_oid(der[alg_at:alg_end])
    if not sset or der[inner[0]:inner[1]] != der[tbs_end:alg_end]:
        out["status"] = ALG
    elif sig_end - sig_at != 1 + SIG_LEN[sset] or der[sig_at] != 0:
        out["status"] = SIG
    elif (version is not None and version != b"\x01") or (ext and version is None):
        out["status"] = VERSION
    elif revoked and revoked[0] == revoked[1]:
        out["status"] = ENTRY
    else:
        out.update(status=OK, sig_set=sset, sig_off=sig_at + 1)
    return out


def walk_entry(der, pos, end):
    """(position behind the entry, the serial's content bytes) or None where the entry at pos breaks a rule"""
    try:
        at, eend = expect(der, pos, end, 0x30)
        sa, sb = expect(der, at, eend, 0x02)
        if not serial_ok(der[sa:sb]):
            return None
        tag, ta, tb = take(der, sb, eend)
        if tag not in TIMES or tb - ta < TIME_MIN:
            return None
        if tb < eend:
            tb = expect(der, tb, eend, 0x30)[1]
        if tb != eend:
            return None
    except Malformed:
        return None
    return eend, bytes(der[sa:sb])


def list_entries(der, w):
    """[(serial, offset in the CRL)] of a CRL whose walk `w` was accepted, or None where the list breaks a rule: an entry refused, bytes
    that are no entry, more entries than revoked_len / 20"""
    pos, end, rows = w["revoked_off"], w["revoked_off"] + w["revoked_len"], []
    while pos < end and len(rows) < w["revoked_len"] // ENTRY_MIN:
        e = walk_entry(der, pos, end)
        if e is None:
            return None
        rows.append((e[1], pos))
        pos = e[0]
    return rows if pos == end else None


def expected_parse(blob, items):
    """the rows mldsa_crl_parse writes"""
    raw = blob.tobytes()
    fields = np.zeros(len(items), dtype=_crl_lib.FIELDS_DTYPE)
    for i, c in enumerate(items):
        off, length = int(c["off"]), int(c["len"])
        if not xc.inside(off, length, len(raw)) or length < 2:
            fields[i]["status"] = RANGE
            continue
        w = walk_crl(raw[off:off + length])
        fields[i]["status"] = w["status"]
        if w["status"] == DER:
            continue
        for f in ("tbs_len", "issuer_len", "revoked_len", "ext_len", "sig_set"):
            fields[i][f] = w[f]
        for f in ("tbs_off", "issuer_off", "this_off"):
            fields[i][f] = off + w[f]
        for f, has in (("sig_off", w["sig_set"]), ("next_off", w["next_off"]), ("revoked_off", w["revoked_off"]), ("ext_off", w["ext_off"])):
            fields[i][f] = off + w[f] if has else 0
    return fields


def expected(blob, items, cert_fields, max_entries, flags=CHECK_NAMES):
    """(crl_fields, entries [max_entries] of _crl_lib.ENTRY_DTYPE, ops, status, totals) as mldsa_crl_ops leaves them"""
    raw = blob.tobytes()
    n = len(items)
    fields = expected_parse(blob, items)
    entries = np.zeros(max_entries, dtype=_crl_lib.ENTRY_DTYPE)
    ops = np.zeros(n, dtype=_rec_lib.OP_DTYPE)
    status = np.zeros(n, dtype=np.uint8)
    totals = np.zeros(1, dtype=_crl_lib.TOTALS_DTYPE)
    first = 0
    for i in range(n):  # the placement: an exclusive scan of the bounds over the CRLs whose walk was accepted
        if fields[i]["status"] != OK:
            continue
        bound = int(fields[i]["revoked_len"]) // ENTRY_MIN
        if first + bound > max_entries:
            fields[i]["status"] = SPACE
        else:
            fields[i]["first"] = first
            totals[0]["slots"] += bound
        first += bound
    for i, c in enumerate(items):  # the entries
        if fields[i]["status"] != OK:
            continue
        off = int(c["off"])
        der = raw[off:off + int(c["len"])]
        w = dict(revoked_off=int(fields[i]["revoked_off"]) - off if fields[i]["revoked_len"] else 0, revoked_len=int(fields[i]["revoked_len"]))
        rows = list_entries(der, w)
        if rows is None:
            fields[i]["status"] = ENTRY
            continue
        fields[i]["count"] = len(rows)
        for k, (serial, at) in enumerate(rows):
            e = entries[int(fields[i]["first"]) + k]
            e["serial"][:len(serial)] = np.frombuffer(serial, dtype=np.uint8)
            e["serial_len"], e["crl"], e["off"] = len(serial), i, at
    for i, c in enumerate(items):  # the link
        st = link_rule(raw, fields[i], int(c["issuer"]), cert_fields, flags)
        status[i] = st
        if st == OK:
            ops[i]["pk_off"], ops[i]["sig_off"], ops[i]["set"] = cert_fields[int(c["issuer"])]["key_off"], fields[i]["sig_off"], fields[i]["sig_set"]
            ops[i]["msg_off"], ops[i]["msg_len"] = fields[i]["tbs_off"], fields[i]["tbs_len"]
            totals[0]["accepted"] += 1
            totals[0]["entries"] += int(fields[i]["count"])
        else:
            totals[0]["refused"] += 1
            if fields[i]["status"] == OK:  # refused by the link: its slots are emptied again
                entries[int(fields[i]["first"]):int(fields[i]["first"]) + int(fields[i]["revoked_len"]) // ENTRY_MIN] = 0
            fields[i]["count"] = 0
    return fields, entries, ops, status, totals


def link_rule(raw, own, issuer, cert_fields, flags):
    if own["status"] != OK:
        return int(own["status"])
    if issuer >= len(cert_fields):
        return ISSUER
    iss = cert_fields[issuer]
    if iss["status"] in (RANGE, DER) or iss["key_set"] == 0 or iss["key_set"] != own["sig_set"]:
        return ISSUER
    if flags & CHECK_NAMES:
        a, a_len, b, b_len = int(own["issuer_off"]), int(own["issuer_len"]), int(iss["subject_off"]), int(iss["subject_len"])
        if a_len != b_len or not xc.inside(a, a_len, len(raw)) or not xc.inside(b, b_len, len(raw)) or raw[a:a + a_len] != raw[b:b + b_len]:
            return NAME
    return OK


# ---- the hash and the table ----
def hash_serial(crl, serial):
    """the constexpr mix of crl_plan.h on (crl, serial_len, the serial zero-padded to 20 bytes as five little-endian words)"""
    m = 0xFFFFFFFF
    words = [crl, len(serial)] + [int.from_bytes(bytes(serial).ljust(20, b"\x00")[4 * k:4 * k + 4], "little") for k in range(5)]
    h = 0x811C9DC5
    for v in words:
        h = ((h ^ v) * 0x9E3779B1) & m
        h ^= h >> 15
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def table_slots(max_entries):
    if max_entries > 1 << 30:
        return 0
    t = 64
    while t < 2 * max_entries:
        t *= 2
    return t


def table_is_sound(table, entries):
    """every full entry row is in the table exactly once, in the probe chain that begins at its home slot; nothing else is in it"""
    slots, mask = len(table), len(table) - 1
    full = {k for k in range(len(entries)) if entries[k]["serial_len"]}
    held = [int(v) - 1 for v in table if v]
    if sorted(held) != sorted(full):
        return False
    where = {int(v) - 1: s for s, v in enumerate(table) if v}
    for k in full:
        e = entries[k]
        home = hash_serial(int(e["crl"]), e["serial"][:int(e["serial_len"])].tobytes()) & mask
        s = home
        while s != where[k]:  # no empty slot between the home slot and the row's
            if table[s] == 0:
                return False
            s = (s + 1) & mask
    return slots == table_slots(len(entries))


def cert_serial(tbs):
    """the serial's content bytes of a TBSCertificate TLV, or None where the rule refuses it"""
    try:
        at, end = expect(tbs, 0, len(tbs), 0x30)
        tag, a, b = take(tbs, at, end)
        if tag == 0xA0:
            tag, a, b = take(tbs, b, end)
        if tag != 0x02 or not serial_ok(tbs[a:b]):
            return None
    except Malformed:
        return None
    return bytes(tbs[a:b])


def expected_check(blob, certs, cert_fields, cert_crl, items, crl_fields, crl_status, crl_ok, entries):
    """revocation uint8 [n_certs]: the rules of the header in their order, the lookup through a Python set"""
    raw = blob.tobytes()
    listed = {(int(e["crl"]), e["serial"][:int(e["serial_len"])].tobytes()) for e in entries if e["serial_len"]}
    out = np.zeros(len(certs), dtype=np.uint8)
    for i, c in enumerate(cert_crl):
        c = int(c)
        if c == NONE:
            out[i] = NO_CRL
        elif c >= len(items):
            out[i] = CRL_INDEX
        elif crl_status[c] != OK or crl_fields[c]["status"] != OK or (crl_ok is not None and not crl_ok[c]):
            out[i] = CRL_REFUSED
        else:
            r = cert_fields[i]
            serial = None
            if r["status"] not in (RANGE, DER) and xc.inside(int(r["tbs_off"]), int(r["tbs_len"]), len(raw)):
                serial = cert_serial(raw[int(r["tbs_off"]):int(r["tbs_off"]) + int(r["tbs_len"])])
            if serial is None:
                out[i] = CERT
            elif certs[i]["issuer"] != items[c]["issuer"]:
                out[i] = SCOPE
            else:
                out[i] = REVOKED if (c, serial) in listed else GOOD
    return out


# ----------------------------------------------------------------------------------------------------------------------- the defects
HEADER_TAGS = ("list", "tbs", "outer", "sig", "version", "inner", "issuer", "this", "next", "revoked", "ext", "ext_inner")
# name -> the status the header documents (of a v2 CRL with nextUpdate, at least three entries and extensions, whose issuer is valid)
DEFECTS = {
    **{"wrong_tag_" + part: DER for part in HEADER_TAGS},
    "trailing_list": DER, "trailing_in_list": DER, "trailing_in_tbs": DER, "trailing_in_ext": DER, "trailing_in_revoked": ENTRY,
    "trailing_in_entry": ENTRY, "len_one_short": DER, "len_one_long": DER, "indefinite_length": DER,
    "outer_alg_null_params": ALG, "alg_sets_differ": ALG, "sig_unused_bits": SIG, "sig_one_short": SIG,
    "version_v1": VERSION, "ext_without_version": VERSION, "empty_revoked": ENTRY, "serial_len_0": ENTRY, "serial_len_21": ENTRY,
    "nonminimal_00": ENTRY, "nonminimal_ff": ENTRY, "entry_one_short": ENTRY, "entry_one_long": ENTRY, "wrong_time_tag": ENTRY,
    "time_too_short": ENTRY, "wrong_tag_entry": ENTRY, "wrong_tag_serial": ENTRY, "wrong_tag_entry_ext": ENTRY,
}


def _retag(part, tag):
    return bytes([tag]) + part[1:]


def _relen(part, delta):
    """the TLV with its (short-form) length byte changed by delta: the bytes stay"""
    assert part[1] < 0x80 and 0 <= part[1] + delta < 0x80
    return part[:1] + bytes([part[1] + delta]) + part[2:]


def make_defect(p, defect):
    """(bytes to lay into the blob, the len to declare for them) of the CRL of parts `p` with one defect.  For len_one_long the
    caller sees to it that one more byte lies behind the CRL in the blob."""
    p = dict(p, entries=None if p["entries"] is None else list(p["entries"]))
    good = join(p)
    n = len(good)
    mid = len(p["entries"]) // 2 if p["entries"] else 0
    if defect == "trailing_list":
        return good + b"\x00", n + 1
    if defect == "len_one_short":
        return good, n - 1
    if defect == "len_one_long":
        return good, n + 1
    if defect == "indefinite_length":
        return good[:1] + b"\x80" + good[2:], n
    if defect == "wrong_tag_list":
        return _retag(good, 0x31), n
    if defect == "wrong_tag_tbs":
        p["tbs_raw"] = _retag(tbs_of(p), 0x31)
    elif defect == "wrong_tag_sig":
        p["sig_raw"] = tlv(0x04, p["sig_bits"])
    elif defect == "wrong_tag_revoked":
        p["revoked_tag"] = 0x31
    elif defect == "wrong_tag_ext_inner":
        p["ext"] = tlv(0xA0, _retag(p["ext"][take(p["ext"], 0, len(p["ext"]))[1]:], 0x31))
    elif defect.startswith("wrong_tag_") and defect[10:] in HEADER_TAGS:
        part = defect[10:]
        assert p[part], "a CRL with every optional field expected"
        p[part] = _retag(p[part], {"version": 0x04, "this": 0x19, "next": 0x19, "ext": 0xA1}.get(part, 0x31))
    elif defect == "trailing_in_list":
        p["list_extra"] = b"\x05\x00"
    elif defect == "trailing_in_tbs":
        p["tbs_extra"] = b"\x05\x00"
    elif defect == "trailing_in_ext":
        p["ext"] = tlv(0xA0, p["ext"][take(p["ext"], 0, len(p["ext"]))[1]:] + b"\x05\x00")
    elif defect == "trailing_in_revoked":
        p["revoked_extra"] = b"\x05\x00"
    elif defect == "trailing_in_entry":
        p["entries"][mid] = tlv(0x30, p["entries"][mid][2:] + b"\x05\x00")
    elif defect == "outer_alg_null_params":
        p["outer"] = tlv(0x30, p["outer"][2:] + b"\x05\x00")
    elif defect == "alg_sets_differ":
        p["outer"] = p["outer"][:-1] + bytes([0x12 if p["outer"][-1] != 0x12 else 0x13])
    elif defect == "sig_unused_bits":
        p["sig_bits"] = b"\x01" + p["sig_bits"][1:]
    elif defect == "sig_one_short":
        p["sig_bits"] = p["sig_bits"][:-1]
    elif defect == "version_v1":
        p["version"] = tlv(0x02, b"\x00")
    elif defect == "ext_without_version":
        p["version"] = b""
    elif defect == "empty_revoked":
        p["entries"] = []
    elif defect == "serial_len_0":
        p["entries"][mid] = entry(b"")
    elif defect == "serial_len_21":
        p["entries"][mid] = entry(b"\x11" * 21)
    elif defect == "nonminimal_00":
        p["entries"][mid] = entry(b"\x00\x7f")
    elif defect == "nonminimal_ff":
        p["entries"][mid] = entry(b"\xff\x80\x01")
    elif defect == "entry_one_short":
        p["entries"][mid] = _relen(p["entries"][mid], -1)
    elif defect == "entry_one_long":
        p["entries"][mid] = _relen(p["entries"][mid], +1)
    elif defect == "wrong_time_tag":
        p["entries"][mid] = entry(b"\x05", date=_retag(UTC, 0x16))
    elif defect == "time_too_short":
        p["entries"][mid] = entry(b"\x05", date=tlv(0x17, b"2501010000Z"))
    elif defect == "wrong_tag_entry":
        p["entries"][mid] = _retag(p["entries"][mid], 0x31)
    elif defect == "wrong_tag_serial":
        p["entries"][mid] = tlv(0x30, tlv(0x04, b"\x05") + UTC)
    elif defect == "wrong_tag_entry_ext":
        p["entries"][mid] = tlv(0x30, tlv(0x02, b"\x05") + UTC + tlv(0x31, reason()))
    else:
        raise KeyError(defect)
    out = join(p)
    return out, len(out)


# ----------------------------------------------------------------------------------------------------------------------- seam cases
CA_CN = {44: b"ca forty-four", 65: b"c" * 130, 87: b"ca-87"}


def ca_certs(tag=b"ca"):
    """three self-signed CA certificates of random bytes, one per parameter set, Names of two length forms"""
    return [xc.random_cert(s, s, CA_CN[s], CA_CN[s], tag, k) for k, s in enumerate(SETS)]


def lay_out(cert_ders, cert_issuers, crl_entries, crl_issuers, pad=0, front=0):
    """(blob, certs, items, cert_fields): the certificates, then the CRLs ((bytes, declared len) each), in one blob with one spare byte
    behind the last; cert_fields is the certificate restatement's rows"""
    blob, rows = certificates_blob(list(cert_ders) + [e[0] for e in crl_entries], list(cert_issuers) + list(crl_issuers), pad=pad, front=front)
    blob = np.concatenate([blob, np.full(1, 0xC3, dtype=np.uint8)])
    nc = len(cert_ders)
    certs = rows[:nc].copy()
    items = np.zeros(len(crl_entries), dtype=_crl_lib.ITEM_DTYPE)
    for f in ("off", "len", "issuer"):
        items[f] = rows[nc:][f]
    for i, e in enumerate(crl_entries):
        items[i]["len"] = e[1]
    return blob, certs, items, xc.expected(blob, certs, 0)[0]


def max_entries_of(items):
    return int(sum(int(c["len"]) // ENTRY_MIN for c in items))


def seam_case(n, seed=0, defect_every=0, front=0):
    """(blob, certs, items, cert_fields) of n random-bytes CRLs under the three CAs, the sets and the entry counts of ENTRY_COUNTS dealt
    in turn, the gaps cycling 0 ... 15; with defect_every every such CRL carries one of the defects in turn"""
    names = list(DEFECTS)
    cas = ca_certs()
    crls, issuers = [], []
    for i in range(n):
        k = (i + seed) % 3
        count = ENTRY_COUNTS[(i + seed) % len(ENTRY_COUNTS)] if n <= 65 else (0, 1, 3, 5)[i % 4]
        p = random_parts(SETS[k], CA_CN[SETS[k]], b"seam%d" % seed, i, count, v2=i % 5 != 4, next_update=i % 3 != 2)
        if defect_every and i % defect_every == defect_every - 1:
            full = random_parts(SETS[k], CA_CN[SETS[k]], b"seam%d" % seed, i, 3 + i % 4)
            crls.append(make_defect(full, names[(i // defect_every + seed) % len(names)]))
        else:
            der = join(p)
            crls.append((der, len(der)))
        issuers.append(k)
    return lay_out(cas, [0, 1, 2], crls, issuers, pad=list(range(16)), front=front)


def mutation_batch(der, positions, issuer_cert):
    """(blob, certs, items, cert_fields): the CRL with each byte of `positions` set to each of xc.MUTATION_VALUES, every copy under the
    one CA certificate"""
    crls = []
    for pos in positions:
        for v in xc.MUTATION_VALUES:
            crls.append((der[:pos] + bytes([v]) + der[pos + 1:], len(der)))
    return lay_out([issuer_cert], [0], crls, [0] * len(crls), pad=[3, 0, 7])
