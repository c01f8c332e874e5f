"""Cases for the path-validation library (include/mldsa_path.h): certificates made with the builder of tests/x509_cases.py (its tail=
argument carries the unique IDs and the extensions), the list of every defect class the header names, and a Python restatement of what
the library must produce -- parse_time, walk_policy, the node rules, the climb and the freshness rule of a CRL --, written from the rules
the header states and not from the kernels.  Loads no library.  Not a test file: test_path_cpu.py and test_gpu_path.py import it by
name."""
import numpy as np

import x509_cases as xc
from fips204_amd import _path_lib
from x509_cases import DER, Malformed, OK, RANGE, SETS, expect, take, tlv

VERSION, TIME, EXT, CRITICAL = 22, 23, 24, 25
ALLOW_UNKNOWN_CRITICAL, REQUIRE_NEXT_UPDATE, ALLOW_NO_CRL = 1, 2, 4
V3, HAS_BC, IS_CA, HAS_KU = 1, 2, 4, 8
MAX_EXTS, MAX_DEPTH, NO_PATH_LEN, NO_ISSUER = 32, 16, 0xFFFFFFFF, 0xFFFFFFFF
TRUSTED, CERT, SIG, POLICY, NOT_YET, EXPIRED, REVOKED, REVOCATION, NOT_CA, KEY_USAGE, PATH_LEN, NO_ANCHOR, DEPTH = range(13)
CRL_FRESH, CRL_REFUSED, CRL_TIME, CRL_NOT_YET, CRL_STALE = range(5)
REV_GOOD, REV_REVOKED, REV_NO_CRL = 0, 1, 2
BC_OID, KU_OID = bytes.fromhex("551d13"), bytes.fromhex("551d0f")
OTHER_OID = bytes.fromhex("551d25")  # extKeyUsage: an extension this library does not read
SEAM_SIZES = (1, 63, 64, 65, 257)
MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


# ----------------------------------------------------------------------------------------------------------------------- the builder
def utc(y, mo=1, d=1, h=0, mi=0, s=0):
    return tlv(0x17, b"%02d%02d%02d%02d%02d%02dZ" % (y % 100, mo, d, h, mi, s))


def generalized(y, mo=1, d=1, h=0, mi=0, s=0):
    return tlv(0x18, b"%04d%02d%02d%02d%02d%02dZ" % (y, mo, d, h, mi, s))


def validity(not_before, not_after):
    return tlv(0x30, not_before + not_after)


def ext(oid, value, critical=None):
    """one Extension: the OID's content bytes, the extnValue's content, critical None (absent), True (01 01 FF) or the BOOLEAN TLV's bytes"""
    flag = b"" if critical is None else b"\x01\x01\xff" if critical is True else bytes(critical)
    return tlv(0x30, tlv(0x06, oid) + flag + tlv(0x04, value))


def basic(ca=True, path_len=None, critical=True):
    """basicConstraints; path_len: None or the INTEGER's content bytes"""
    return ext(BC_OID, tlv(0x30, (b"\x01\x01\xff" if ca else b"") + (b"" if path_len is None else tlv(0x02, path_len))), critical)


def key_usage(content, critical=True):
    """keyUsage; content: the BIT STRING's content bytes, the unused-bits byte first"""
    return ext(KU_OID, tlv(0x03, content), critical)


def other(k=0, critical=None):
    return ext(OTHER_OID, tlv(0x30, bytes([0x05, 0x00]) * (k % 3)), critical)


def extensions(exts):
    """the [3] tail around a list of Extension TLVs"""
    return tlv(0xA3, tlv(0x30, b"".join(exts)))


CA_TAIL = extensions([basic(), key_usage(b"\x01\x06")])  # cA, keyCertSign and cRLSign
V1, V2, V3_VERSION = b"", tlv(0xA0, b"\x02\x01\x01"), xc.VERSION


def make(pset=44, version=None, dates=None, tail=b"", tag=b"path", i=0, issuer_cn=b"root", subject_cn=b"leaf"):
    """a certificate of random key and signature bytes with the given tail; version / dates (whole TLVs) replace the builder's"""
    der = xc.random_cert(pset, pset, issuer_cn, subject_cn, tag, i, tail=tail)
    if version is None and dates is None:
        return der
    p = xc.split(der)
    if version is not None:
        p["version"] = version
    if dates is not None:
        p["validity"] = dates
    return xc.join(p)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def days_before_year(y):
    """days of the proleptic Gregorian calendar in the years 1 ... y - 1"""
    return 365 * (y - 1) + (y - 1) // 4 - (y - 1) // 100 + (y - 1) // 400


def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def parse_time(buf, pos, end):
    """(seconds, position behind the TLV) of the Time TLV at buf[pos:end], or None where the header's rules refuse it"""
    try:
        tag, a, b = take(buf, pos, end)
    except Malformed:
        return None
    c = bytes(buf[a:b])
    if tag == 0x17 and len(c) == 13:
        digits = c[:12]
    elif tag == 0x18 and len(c) == 15:
        digits = c[:14]
    else:
        return None
    if c[-1:] != b"Z" or not all(0x30 <= x <= 0x39 for x in digits):
        return None
    text = digits.decode()
    if tag == 0x17:
        yy = int(text[:2])
        year, rest = (2000 + yy if yy < 50 else 1900 + yy), text[2:]
    else:
        year, rest = int(text[:4]), text[4:]
    month, day, hour, minute, second = (int(rest[k:k + 2]) for k in range(0, 10, 2))
    if year < 1 or not 1 <= month <= 12:
        return None
    month_end = 29 if month == 2 and is_leap(year) else MONTH_DAYS[month - 1]
    if not 1 <= day <= month_end or hour > 23 or minute > 59 or second > 59:
        return None
    days = days_before_year(year) + sum(MONTH_DAYS[:month - 1]) + (1 if month > 2 and is_leap(year) else 0) + day - 1 - days_before_year(1970)
    return days * 86400 + hour * 3600 + minute * 60 + second, b


def basic_rule(value):
    """(ca, path_len) of a basicConstraints extnValue's content, or None where it is refused"""
    try:
        a, b = expect(value, 0, len(value), 0x30)
        if b != len(value):
            return None
        ca, path_len, pos = False, NO_PATH_LEN, a
        if pos < b and take(value, pos, b)[0] == 0x01:
            _, x, y = take(value, pos, b)
            if value[x:y] != b"\xff":
                return None
            ca, pos = True, y
        if pos < b:
            x, y = expect(value, pos, b, 0x02)
            digits = value[x:y]
            if not 1 <= len(digits) <= 4 or not ca:
                return None
            n = int.from_bytes(digits, "big", signed=True)
            if n < 0 or len(digits) != n.bit_length() // 8 + 1:  # non-negative, and no byte more than the value needs
                return None
            path_len, pos = n, y
        if pos != b:
            return None
    except Malformed:
        return None
    return ca, path_len


def key_usage_rule(value):
    """the uint16 of a keyUsage extnValue's content (bit i = KeyUsage bit i), or None where it is refused"""
    try:
        a, b = expect(value, 0, len(value), 0x03)
    except Malformed:
        return None
    c = value[a:b]
    if b != len(value) or not 2 <= len(c) <= 3 or c[0] > 7:
        return None
    bits = "".join("{:08b}".format(x) for x in c[1:])
    used, unused = bits[:len(bits) - c[0]], bits[len(bits) - c[0]:]
    if "1" in unused or not used.endswith("1"):  # the named-bit-list rule: no trailing zero bit
        return None
    return sum(1 << i for i, bit in enumerate(used) if bit == "1")


def walk_policy(der, flags=0):
    """dict of the certificate's policy fields relative to its first byte, status among OK / DER / VERSION / TIME / EXT / CRITICAL"""
    out = dict(not_before=0, not_after=0, ext_off=0, ext_len=0, crit_off=0, path_len=0, key_usage=0, flags=0, n_ext=0, n_crit=0, status=DER)
    n, broken = len(der), set()
    found = dict(out, path_len=NO_PATH_LEN)
    try:
        at, behind = expect(der, 0, n, 0x30)
        if behind != n:
            raise Malformed("bytes behind the certificate")
        tbs_at, tbs_end = expect(der, at, n, 0x30)
        alg_end = expect(der, tbs_end, n, 0x30)[1]
        if expect(der, alg_end, n, 0x03)[1] != n:
            raise Malformed("bytes behind the signature")
        pos, version = tbs_at, 1
        tag, a, b = take(der, pos, tbs_end)
        if tag == 0xA0:
            if der[a:b] in (b"\x02\x01\x01", b"\x02\x01\x02"):
                version = der[b - 1] + 1
            else:
                broken.add(VERSION)
            pos = b
        pos = expect(der, pos, tbs_end, 0x02)[1]
        pos = expect(der, pos, tbs_end, 0x30)[1]
        pos = expect(der, pos, tbs_end, 0x30)[1]
        val_at, val_end = expect(der, pos, tbs_end, 0x30)
        pos = expect(der, val_end, tbs_end, 0x30)[1]
        spki_at, spki_end = expect(der, pos, tbs_end, 0x30)
        kalg_end = expect(der, spki_at, spki_end, 0x30)[1]
        if expect(der, kalg_end, spki_end, 0x03)[1] != spki_end:
            raise Malformed("bytes behind the key")
        pos, has_uid, exts = spki_end, False, None
        for uid in (0x81, 0x82):
            if pos < tbs_end and take(der, pos, tbs_end)[0] == uid:
                has_uid, pos = True, take(der, pos, tbs_end)[2]
        if pos < tbs_end:
            a, b = expect(der, pos, tbs_end, 0xA3)
            exts = expect(der, a, b, 0x30)
            if exts[1] != b:
                raise Malformed("bytes behind the extensions")
            pos = b
        if pos != tbs_end:
            raise Malformed("a field that belongs nowhere")
        if (has_uid and version < 2) or (exts is not None and version < 3):
            broken.add(VERSION)
        values = {}
        if exts is not None:
            q, eend = exts
            found.update(ext_off=q, ext_len=eend - q)
            if q == eend:
                broken.add(EXT)
            while q < eend and found["n_ext"] < MAX_EXTS:
                xa, xb = expect(der, q, eend, 0x30)
                oa, ob = expect(der, xa, xb, 0x06)
                tag, a, b = take(der, ob, xb)
                critical = False
                if tag == 0x01:
                    if der[a:b] == b"\xff":
                        critical = True
                    else:
                        broken.add(EXT)
                    tag, a, b = take(der, b, xb)
                if tag != 0x04 or b != xb:
                    raise Malformed("no extnValue, or bytes behind it")
                oid = bytes(der[oa:ob])
                if oid in (BC_OID, KU_OID):
                    if oid in values:
                        broken.add(EXT)  # twice
                    else:
                        values[oid] = bytes(der[a:b])
                elif critical:
                    if found["n_crit"] == 0:
                        found["crit_off"] = q
                    found["n_crit"] += 1
                found["n_ext"] += 1
                q = xb
            if q != eend:
                broken.add(EXT)  # more than MAX_EXTS
    except Malformed:
        return out
    if BC_OID in values:
        rule = basic_rule(values[BC_OID])
        if rule is None:
            broken.add(EXT)
        else:
            found["flags"] |= HAS_BC | (IS_CA if rule[0] else 0)
            found["path_len"] = rule[1]
    if KU_OID in values:
        bits = key_usage_rule(values[KU_OID])
        if bits is None:
            broken.add(EXT)
        else:
            found["flags"] |= HAS_KU
            found["key_usage"] = bits
    first = parse_time(der, val_at, val_end)
    second = parse_time(der, first[1], val_end) if first else None
    if first and second and second[1] == val_end:
        found.update(not_before=first[0], not_after=second[0])
    else:
        broken.add(TIME)
    if VERSION not in broken and version == 3:
        found["flags"] |= V3
    if found["n_crit"] and not flags & ALLOW_UNKNOWN_CRITICAL:
        broken.add(CRITICAL)
    found["status"] = min(broken) if broken else OK  # the codes rise in the order of the header: VERSION, TIME, EXT, CRITICAL
    return found


def expected_parse(blob, certs, flags=0):
    """the mldsa_path_fields rows for a blob (uint8 array) and its certificate entries"""
    raw = blob.tobytes()
    fields = np.zeros(len(certs), dtype=_path_lib.FIELDS_DTYPE)
    for i, c in enumerate(certs):
        off, length = int(c["off"]), int(c["len"])
        if not xc.inside(off, length, len(raw)) or length < 2:
            fields[i]["status"] = RANGE
            continue
        w = walk_policy(raw[off:off + length], flags)
        fields[i]["status"] = w["status"]
        if w["status"] == DER:
            continue
        for f in ("not_before", "not_after", "ext_len", "path_len", "key_usage", "flags", "n_ext"):
            fields[i][f] = w[f]
        for f in ("ext_off", "crit_off"):
            fields[i][f] = off + w[f] if w[f] else 0
    return fields


def expected_times(blob, offs):
    """(seconds int64, status uint8) of mldsa_path_times"""
    raw = blob.tobytes()
    seconds, status = np.zeros(len(offs), dtype=np.int64), np.zeros(len(offs), dtype=np.uint8)
    for i, off in enumerate(int(x) for x in offs):
        if off + 2 > len(raw):
            status[i] = RANGE
            continue
        got = parse_time(raw, off, len(raw))
        if got is None:
            status[i] = TIME
        else:
            seconds[i] = got[0]
    return seconds, status


def own_rule(cert_status, cert_ok, policy, revocation, now, flags):
    """the first rule a certificate breaks for itself, or 0; revocation None: not checked"""
    if cert_status != 0:
        return CERT
    if not cert_ok:
        return SIG
    if policy["status"] != OK:
        return POLICY
    if now < int(policy["not_before"]):
        return NOT_YET
    if now > int(policy["not_after"]):
        return EXPIRED
    if revocation is None or revocation == REV_GOOD:
        return 0
    if revocation == REV_REVOKED:
        return REVOKED
    if revocation == REV_NO_CRL and flags & ALLOW_NO_CRL:
        return 0
    return REVOCATION


def issuer_rule(policy):
    f = int(policy["flags"])
    if not (f & V3 and f & HAS_BC and f & IS_CA):
        return NOT_CA
    if f & HAS_KU and not int(policy["key_usage"]) & (1 << 5):
        return KEY_USAGE
    return 0


def nodes_of(issuers, policy, cert_status, cert_ok, revocation, anchor, now, flags=0):
    """the node array of mldsa_path_chain's scratch"""
    nodes = np.zeros(len(issuers), dtype=_path_lib.NODE_DTYPE)
    for i in range(len(issuers)):
        path_len = int(policy[i]["path_len"])
        nodes[i] = (int(issuers[i]), own_rule(int(cert_status[i]), bool(cert_ok[i]), policy[i], None if revocation is None else int(revocation[i]),
                                              now, flags),
                    issuer_rule(policy[i]), 255 if path_len == NO_PATH_LEN else min(path_len, 254), 1 if anchor[i] else 0)
    return nodes


def climb(nodes, i):
    """(verdict, where, depth) of certificate i"""
    n, a = len(nodes), i
    for k in range(MAX_DEPTH + 1):
        nd = nodes[a]
        if nd["anchor"]:
            return TRUSTED, a, k
        if nd["own"]:
            return int(nd["own"]), a, k
        if k >= 1 and nd["as_issuer"]:
            return int(nd["as_issuer"]), a, k
        if k >= 1 and nd["path_len"] != 255 and k - 1 > int(nd["path_len"]):
            return PATH_LEN, a, k
        issuer = int(nd["issuer"])
        if issuer == NO_ISSUER or issuer >= n or issuer == a:
            return NO_ANCHOR, a, k
        if k + 1 > MAX_DEPTH:
            return DEPTH, a, k
        a = issuer
    raise AssertionError("the climb ends inside its loop")


def expected_chain(issuers, policy, cert_status, cert_ok, revocation, anchor, now, flags=0):
    """the mldsa_path_result rows"""
    nodes = nodes_of(issuers, policy, cert_status, cert_ok, revocation, anchor, now, flags)
    out = np.zeros(len(issuers), dtype=_path_lib.RESULT_DTYPE)
    for i in range(len(issuers)):
        out[i]["verdict"], out[i]["where"], out[i]["depth"] = climb(nodes, i)
    return out


def expected_crl_times(blob, crl_fields, crl_status, crl_ok, now, flags=0):
    """(this_s, next_s, time_status, fresh_ok) of mldsa_path_crl_times"""
    raw = blob.tobytes()
    n = len(crl_fields)
    this_s, next_s = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    status, fresh = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for c in range(n):
        row = crl_fields[c]
        if int(crl_status[c]) != OK or int(row["status"]) != OK:
            status[c] = CRL_REFUSED
            continue
        this_off, next_off = int(row["this_off"]), int(row["next_off"])
        first = parse_time(raw, this_off, len(raw)) if this_off + 2 <= len(raw) else None
        second = parse_time(raw, next_off, len(raw)) if next_off and next_off + 2 <= len(raw) else None
        this_s[c], next_s[c] = first[0] if first else 0, second[0] if second else 0
        if first is None or (next_off and second is None):
            status[c] = CRL_TIME
        elif now < first[0]:
            status[c] = CRL_NOT_YET
        elif (now > second[0]) if next_off else bool(flags & REQUIRE_NEXT_UPDATE):
            status[c] = CRL_STALE
        else:
            status[c] = CRL_FRESH
            fresh[c] = 1 if crl_ok is None or crl_ok[c] else 0
    return this_s, next_s, status, fresh


# ----------------------------------------------------------------------------------------------------------------------- the defects
DATES = validity(utc(2025), utc(2035))
_INT = lambda content: tlv(0x30, b"\x01\x01\xff" + tlv(0x02, content))  # noqa: E731  (a basicConstraints value with cA and a pathLen)
_ONE = tlv(0x30, tlv(0x06, OTHER_OID) + tlv(0x04, b""))  # one well-formed extension, for the frames around it

# name -> (the status the header documents, keyword arguments of make()).  Every class of the header: the version rule, every refusal
# of parse_time, the fields behind the SPKI, an extension's frame, the critical BOOLEAN, both values, the counts, and what is accepted.
CASES = {
    # accepted
    "ok_v3_plain": (OK, dict()),
    "ok_v1": (OK, dict(version=V1)),
    "ok_v2_both_uids": (OK, dict(version=V2, tail=tlv(0x81, b"\x00\x55") + tlv(0x82, b"\x00\x66"))),
    "ok_v3_uid_and_ca": (OK, dict(tail=tlv(0x82, b"\x00\x66") + CA_TAIL)),
    "ok_ca": (OK, dict(tail=CA_TAIL)),
    "ok_bc_empty": (OK, dict(tail=extensions([basic(ca=False, critical=None)]))),
    "ok_generalized_dates": (OK, dict(dates=validity(generalized(1999, 12, 31, 23, 59, 59), generalized(2400, 2, 29)))),
    "ok_unknown_not_critical": (OK, dict(tail=extensions([other(1), basic(), other(2)]))),
    "ok_32_extensions": (OK, dict(tail=extensions([other(k) for k in range(30)] + [basic(), key_usage(b"\x02\x04")]))),
    "ok_path_len_0": (OK, dict(tail=extensions([basic(path_len=b"\x00")]))),
    "ok_path_len_127": (OK, dict(tail=extensions([basic(path_len=b"\x7f")]))),
    "ok_path_len_128": (OK, dict(tail=extensions([basic(path_len=b"\x00\x80")]))),
    "ok_path_len_max": (OK, dict(tail=extensions([basic(path_len=b"\x7f\xff\xff\xff")]))),
    "ok_ku_1_bit": (OK, dict(tail=extensions([key_usage(b"\x07\x80")]))),
    "ok_ku_8_bits": (OK, dict(tail=extensions([key_usage(b"\x00\x07")]))),
    "ok_ku_9_bits": (OK, dict(tail=extensions([key_usage(b"\x07\x06\x80")]))),
    "ok_ku_16_bits": (OK, dict(tail=extensions([key_usage(b"\x00\xa5\x01", critical=None)]))),
    # VERSION
    "version_explicit_v1": (VERSION, dict(version=tlv(0xA0, b"\x02\x01\x00"))),
    "version_v4": (VERSION, dict(version=tlv(0xA0, b"\x02\x01\x03"))),
    "version_two_bytes": (VERSION, dict(version=tlv(0xA0, b"\x02\x02\x00\x02"))),
    "version_no_integer": (VERSION, dict(version=tlv(0xA0, b"\x04\x01\x02"))),
    "version_empty": (VERSION, dict(version=tlv(0xA0, b""))),
    "version_uid_in_v1": (VERSION, dict(version=V1, tail=tlv(0x81, b"\x00\x55"))),
    "version_ext_in_v1": (VERSION, dict(version=V1, tail=CA_TAIL)),
    "version_ext_in_v2": (VERSION, dict(version=V2, tail=CA_TAIL)),
    # TIME
    "time_utc_12_bytes": (TIME, dict(dates=validity(tlv(0x17, b"25010100000Z"), utc(2035)))),
    "time_utc_14_bytes": (TIME, dict(dates=validity(utc(2025), tlv(0x17, b"3501010000000Z")))),
    "time_generalized_14_bytes": (TIME, dict(dates=validity(tlv(0x18, b"2025010100000Z"), utc(2035)))),
    "time_generalized_16_bytes": (TIME, dict(dates=validity(utc(2025), tlv(0x18, b"20350101000000.Z")))),
    "time_wrong_tag": (TIME, dict(dates=validity(tlv(0x16, b"250101000000Z"), utc(2035)))),
    "time_non_digit": (TIME, dict(dates=validity(tlv(0x17, b"25010100000/Z"), utc(2035)))),
    "time_colon": (TIME, dict(dates=validity(tlv(0x17, b"2501010000:0Z"), utc(2035)))),
    "time_month_0": (TIME, dict(dates=validity(utc(2025, 0, 1), utc(2035)))),
    "time_month_13": (TIME, dict(dates=validity(utc(2025, 13, 1), utc(2035)))),
    "time_day_0": (TIME, dict(dates=validity(utc(2025, 1, 0), utc(2035)))),
    "time_april_31": (TIME, dict(dates=validity(utc(2025, 4, 31), utc(2035)))),
    "time_february_29_2025": (TIME, dict(dates=validity(utc(2025, 2, 29), utc(2035)))),
    "time_february_29_1900": (TIME, dict(dates=validity(generalized(1900, 2, 29), utc(2035)))),
    "time_february_29_2100": (TIME, dict(dates=validity(utc(2025), generalized(2100, 2, 29)))),
    "time_february_30_2000": (TIME, dict(dates=validity(generalized(2000, 2, 30), utc(2035)))),
    "time_hour_24": (TIME, dict(dates=validity(utc(2025, 1, 1, 24), utc(2035)))),
    "time_minute_60": (TIME, dict(dates=validity(utc(2025, 1, 1, 0, 60), utc(2035)))),
    "time_second_60": (TIME, dict(dates=validity(utc(2025), utc(2035, 12, 31, 23, 59, 60)))),
    "time_lower_case_z": (TIME, dict(dates=validity(tlv(0x17, b"250101000000z"), utc(2035)))),
    "time_year_0000": (TIME, dict(dates=validity(generalized(0), utc(2035)))),
    "time_one_only": (TIME, dict(dates=tlv(0x30, utc(2025)))),
    "time_three": (TIME, dict(dates=tlv(0x30, utc(2025) + utc(2035) + utc(2036)))),
    "time_none": (TIME, dict(dates=tlv(0x30, b""))),
    "time_trailing_byte": (TIME, dict(dates=tlv(0x30, utc(2025) + utc(2035) + b"\x00"))),
    # DER: the fields behind the SPKI and the frame of an extension
    "der_tail_wrong_tag": (DER, dict(tail=b"\x05\x00")),
    "der_tail_trailing": (DER, dict(tail=CA_TAIL + b"\x05\x00")),
    "der_uids_swapped": (DER, dict(tail=tlv(0x82, b"\x00\x66") + tlv(0x81, b"\x00\x55"))),
    "der_uid_twice": (DER, dict(tail=tlv(0x81, b"\x00\x55") + tlv(0x81, b"\x00\x55"))),
    "der_uid_behind_extensions": (DER, dict(tail=CA_TAIL + tlv(0x81, b"\x00\x55"))),
    "der_tail_header_alone": (DER, dict(tail=b"\xa3")),
    "der_wrapper_empty": (DER, dict(tail=tlv(0xA3, b""))),
    "der_wrapper_no_sequence": (DER, dict(tail=tlv(0xA3, tlv(0x31, _ONE)))),
    "der_wrapper_trailing": (DER, dict(tail=tlv(0xA3, tlv(0x30, _ONE) + b"\x05\x00"))),
    "der_extension_no_sequence": (DER, dict(tail=extensions([b"\x31" + _ONE[1:]]))),
    "der_extension_overruns": (DER, dict(tail=extensions([_ONE[:1] + bytes([_ONE[1] + 1]) + _ONE[2:]]))),
    "der_extension_no_oid": (DER, dict(tail=extensions([tlv(0x30, tlv(0x04, b""))]))),
    "der_extension_oid_alone": (DER, dict(tail=extensions([tlv(0x30, tlv(0x06, OTHER_OID))]))),
    "der_extension_flag_alone": (DER, dict(tail=extensions([tlv(0x30, tlv(0x06, OTHER_OID) + b"\x01\x01\xff")]))),
    "der_extension_value_no_octets": (DER, dict(tail=extensions([tlv(0x30, tlv(0x06, OTHER_OID) + tlv(0x03, b"\x00"))]))),
    "der_extension_trailing": (DER, dict(tail=extensions([tlv(0x30, tlv(0x06, OTHER_OID) + tlv(0x04, b"") + b"\x05\x00")]))),
    "der_extension_two_flags": (DER, dict(tail=extensions([tlv(0x30, tlv(0x06, OTHER_OID) + b"\x01\x01\xff" * 2 + tlv(0x04, b""))]))),
    "der_second_extension_indefinite": (DER, dict(tail=extensions([basic(), b"\x30\x80" + _ONE[2:]]))),
    # EXT
    "ext_empty_list": (EXT, dict(tail=extensions([]))),
    "ext_33_extensions": (EXT, dict(tail=extensions([other(k) for k in range(33)]))),
    "ext_critical_false": (EXT, dict(tail=extensions([other(0, critical=b"\x01\x01\x00")]))),
    "ext_critical_01": (EXT, dict(tail=extensions([basic(critical=b"\x01\x01\x01")]))),
    "ext_critical_two_bytes": (EXT, dict(tail=extensions([other(0, critical=b"\x01\x02\xff\xff")]))),
    "ext_critical_empty": (EXT, dict(tail=extensions([other(0, critical=b"\x01\x00")]))),
    "ext_bc_twice": (EXT, dict(tail=extensions([basic(), basic()]))),
    "ext_ku_twice": (EXT, dict(tail=extensions([key_usage(b"\x02\x04"), other(1), key_usage(b"\x02\x04")]))),
    "ext_bc_no_sequence": (EXT, dict(tail=extensions([ext(BC_OID, b"\x31\x03\x01\x01\xff", True)]))),
    "ext_bc_empty_value": (EXT, dict(tail=extensions([ext(BC_OID, b"", True)]))),
    "ext_bc_value_trailing": (EXT, dict(tail=extensions([ext(BC_OID, b"\x30\x03\x01\x01\xff\x05\x00", True)]))),
    "ext_bc_inner_trailing": (EXT, dict(tail=extensions([ext(BC_OID, tlv(0x30, b"\x01\x01\xff\x02\x01\x00\x05\x00"), True)]))),
    "ext_bc_ca_false": (EXT, dict(tail=extensions([ext(BC_OID, tlv(0x30, b"\x01\x01\x00"), True)]))),
    "ext_bc_ca_two_bytes": (EXT, dict(tail=extensions([ext(BC_OID, tlv(0x30, b"\x01\x02\xff\xff"), True)]))),
    "ext_bc_path_len_without_ca": (EXT, dict(tail=extensions([basic(ca=False, path_len=b"\x00")]))),
    "ext_bc_path_len_negative": (EXT, dict(tail=extensions([ext(BC_OID, _INT(b"\x80"), True)]))),
    "ext_bc_path_len_minus_one": (EXT, dict(tail=extensions([ext(BC_OID, _INT(b"\xff\xff"), True)]))),
    "ext_bc_path_len_not_minimal": (EXT, dict(tail=extensions([ext(BC_OID, _INT(b"\x00\x7f"), True)]))),
    "ext_bc_path_len_5_bytes": (EXT, dict(tail=extensions([ext(BC_OID, _INT(b"\x00\x80\x00\x00\x00"), True)]))),
    "ext_bc_path_len_empty": (EXT, dict(tail=extensions([ext(BC_OID, _INT(b""), True)]))),
    "ext_bc_path_len_wrong_tag": (EXT, dict(tail=extensions([ext(BC_OID, tlv(0x30, b"\x01\x01\xff\x04\x01\x00"), True)]))),
    "ext_bc_inner_indefinite": (EXT, dict(tail=extensions([ext(BC_OID, b"\x30\x80\x01\x01\xff", True)]))),
    "ext_ku_no_bit_string": (EXT, dict(tail=extensions([ext(KU_OID, tlv(0x04, b"\x02\x04"), True)]))),
    "ext_ku_one_byte": (EXT, dict(tail=extensions([key_usage(b"\x00")]))),
    "ext_ku_four_bytes": (EXT, dict(tail=extensions([key_usage(b"\x00\x01\x01\x01")]))),
    "ext_ku_unused_8": (EXT, dict(tail=extensions([key_usage(b"\x08\x00")]))),
    "ext_ku_unused_bit_set": (EXT, dict(tail=extensions([key_usage(b"\x02\x05")]))),
    "ext_ku_trailing_zero_bit": (EXT, dict(tail=extensions([key_usage(b"\x01\x04")]))),
    "ext_ku_trailing_zero_byte": (EXT, dict(tail=extensions([key_usage(b"\x00\x80\x00")]))),
    "ext_ku_no_bit": (EXT, dict(tail=extensions([key_usage(b"\x00\x00")]))),
    "ext_ku_value_trailing": (EXT, dict(tail=extensions([ext(KU_OID, tlv(0x03, b"\x02\x04") + b"\x05\x00", True)]))),
    # CRITICAL
    "critical_unknown": (CRITICAL, dict(tail=extensions([basic(), other(1, critical=True)]))),
    "critical_unknown_twice": (CRITICAL, dict(tail=extensions([other(0), other(1, critical=True), other(2, critical=True)]))),
}


def case(name, pset=44, i=0):
    return make(pset, i=i, **CASES[name][1])


def seam_case(n, seed=0, front=0):
    """(blob, certs) of n certificates, the cases dealt with a stride and every third a plain CA, mixed parameter sets, the gaps cycling 0 ... 15"""
    names = list(CASES)
    ders = []
    for i in range(n):
        pset = SETS[(i + seed) % 3]
        ders.append(make(pset, tail=CA_TAIL, i=i) if i % 3 == 2 else case(names[(11 * i + 5 * seed) % len(names)], pset, i))
    return xc.lay_out([(d, len(d)) for d in ders], [0] * n, pad=list(range(16)), front=front)


def spans(der):
    """the byte ranges of the validity TLV and of the [3] tail of a certificate the builder made"""
    p = xc.split(der)
    tbs_at = take(der, xc.walk(der)["tbs_off"], len(der))[1]
    at = tbs_at + sum(len(p[k]) for k in ("version", "serial", "inner", "issuer"))
    tail_at = at + len(p["validity"]) + len(p["subject"]) + len(p["spki"])
    assert der[at:at + len(p["validity"])] == p["validity"] and der[tail_at:tail_at + len(p["tail"])] == p["tail"]
    return list(range(at, at + len(p["validity"]))) + list(range(tail_at, tail_at + len(p["tail"])))


def mutation_batch(der, positions):
    """(blob, certs): the certificate with each of `positions` set to each of xc.MUTATION_VALUES"""
    entries = [(der[:pos] + bytes([v]) + der[pos + 1:], len(der)) for pos in positions for v in xc.MUTATION_VALUES]
    return xc.lay_out(entries, list(range(len(entries))), pad=[3, 0, 7])


# ----------------------------------------------------------------------------------------------------------------------- chains
def policy_rows(n, ca=True, not_before=1000, not_after=2000):
    """n policy rows of a v3 CA (or a plain v3 leaf) valid in [not_before, not_after]"""
    rows = np.zeros(n, dtype=_path_lib.FIELDS_DTYPE)
    rows["not_before"], rows["not_after"], rows["path_len"] = not_before, not_after, NO_PATH_LEN
    rows["flags"] = V3 | HAS_BC | IS_CA | HAS_KU if ca else V3
    rows["key_usage"] = (1 << 5) | (1 << 6) if ca else 1
    return rows


def line(depth, anchored=True):
    """issuers and anchors of one chain: certificate 0 is the root (its own issuer, the anchor), certificate k is issued by k - 1; the
    leaf, certificate `depth`, is that many steps from the anchor"""
    issuers = np.array([0] + list(range(depth)), dtype=np.uint32)
    anchor = np.zeros(depth + 1, dtype=np.uint8)
    anchor[0] = 1 if anchored else 0
    return issuers, anchor
