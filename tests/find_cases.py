"""The rules of include/mldsa_find.h restated in plain Python, and builders of certificates and CRLs that carry subjectKeyIdentifier and
authorityKeyIdentifier extensions.  The restatement knows nothing of the table's hash: candidates are a dict from key to the sorted list
of the certificates entered under it, a lookup is a dict access.  Both test_find_cpu.py and test_gpu_find.py import this module; it
loads no library."""
import numpy as np

import crl_cases as cc
import path_cases as pc
import x509_cases as xc
from fips204_amd import _crl_lib, _find_lib, _x509_lib
from x509_cases import Malformed, _bytes, take, tlv

OK, RANGE, DER, ALG, SIG = range(5)
EXT = 26
FOUND, NONE, CERT, SPACE = range(4)
MAX_EXTS, MAX_KEYID, PROBE_MAX, OVERFLOW_MAX = 32, 64, 256, 1024
NO_ISSUER = 0xFFFFFFFF
CRL_NONE = 0xFFFFFFFF
SKI_OID, AKI_OID = bytes.fromhex("551d0e"), bytes.fromhex("551d23")
ANY, SKI, NOSKI = "any", "ski", "noski"
NAME_LENGTHS = (2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ID_LENGTHS = (1, 20, 32, 64)


# ----------------------------------------------------------------------------------------------------------------------- the builders
def name_of_len(total, fill):
    """a Name TLV of exactly `total` bytes (2: the empty Name 30 00; else one commonName), filled from `fill`"""
    if total == 2:
        return b"\x30\x00"
    for cn_len in range(1, total):
        cn = (bytes(fill) * (cn_len // max(len(fill), 1) + 1))[:cn_len]
        out = tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, cn))))
        if len(out) == total:
            return out
        if len(out) > total:
            break
    raise ValueError("no one-commonName Name is %d bytes long" % total)


def ski_ext(key_id, critical=None):
    return pc.ext(SKI_OID, tlv(0x04, key_id), critical)


def aki_ext(key_id=None, issuer=None, serial=None, critical=None):
    """authorityKeyIdentifier: [0] keyIdentifier, [1] authorityCertIssuer (a Name TLV, wrapped as a directoryName) and [2]
    authorityCertSerialNumber, each where given"""
    content = (b"" if key_id is None else tlv(0x80, key_id)) + (b"" if issuer is None else tlv(0xA1, tlv(0xA4, issuer)))
    return pc.ext(AKI_OID, tlv(0x30, content + (b"" if serial is None else tlv(0x82, serial))), critical)


def cert(sig_set, key_set, issuer_name, subject_name, tag, i, exts=(), tail=None):
    """a certificate of random key and signature bytes around two Name TLVs given as bytes, with the extensions `exts` (or the raw tail)"""
    pk = _bytes(tag + b"pk", i, xc.PK_LEN.get(key_set, 270))
    spki = tlv(0x30, xc.alg_id(key_set) + tlv(0x03, b"\x00" + pk))
    if tail is None:
        tail = pc.extensions(list(exts)) if exts else b""
    body = tlv(0x30, xc.VERSION + xc.SERIAL + xc.alg_id(sig_set) + issuer_name + xc.VALIDITY + subject_name + spki + tail)
    return xc.cert(body, sig_set, _bytes(tag + b"sig", i, xc.SIG_LEN[sig_set]))


def crl(sig_set, issuer_name, tag, i, ext=b"default"):
    """a CRL without entries around an issuer Name given as bytes; ext: the content of crlExtensions (default: a cRLNumber), None: absent"""
    p = cc.random_parts(sig_set, b"x", tag, i, 0, ext=ext)
    p["issuer"] = issuer_name
    return cc.join(p)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def walk_ids(buf, pos, end):
    """walk_ids of the header over buf[pos:end], the content of an Extensions SEQUENCE: a dict of status and the two ranges (positions
    in buf)"""
    out = dict(status=DER, ski_off=0, ski_len=0, aki_off=0, aki_len=0)
    found, twice, q, k = {}, False, pos, 0
    try:
        while q < end and k < MAX_EXTS:
            tag, at, behind = take(buf, q, end)
            if tag != 0x30:
                raise Malformed("an extension is a SEQUENCE")
            otag, oat, obehind = take(buf, at, behind)
            if otag != 0x06:
                raise Malformed("extnID")
            vtag, vat, vbehind = take(buf, obehind, behind)
            if vtag == 0x01:
                vtag, vat, vbehind = take(buf, vbehind, behind)
            if vtag != 0x04 or vbehind != behind:
                raise Malformed("extnValue")
            oid = bytes(buf[oat:obehind])
            if oid in (SKI_OID, AKI_OID):
                twice = twice or oid in found
                found.setdefault(oid, (vat, behind))
            q, k = behind, k + 1
    except Malformed:
        return out
    out["status"] = EXT
    if q != end or twice:
        return out
    ids = {}
    try:
        if SKI_OID in found:
            at, behind = found[SKI_OID]
            tag, iat, ibehind = take(buf, at, behind)
            if tag != 0x04 or ibehind != behind or not 1 <= ibehind - iat <= MAX_KEYID:
                return out
            ids["ski_off"], ids["ski_len"] = iat, ibehind - iat
        if AKI_OID in found:
            at, behind = found[AKI_OID]
            tag, p, sbehind = take(buf, at, behind)
            if tag != 0x30 or sbehind != behind:
                return out
            for member in (0x80, 0xA1, 0x82):
                if p >= behind:
                    break
                tag, mat, mbehind = take(buf, p, behind)
                if tag != member:
                    continue
                if member == 0x80:
                    if not 1 <= mbehind - mat <= MAX_KEYID:
                        return out
                    ids["aki_off"], ids["aki_len"] = mat, mbehind - mat
                p = mbehind
            if p != behind:
                return out
    except Malformed:
        return out
    out.update(ids, status=OK)
    return out


def within(off, length, outer_off, outer_len):
    return outer_off <= off and off + length <= outer_off + outer_len


def expected_ids(blob, certs, policy):
    """ids [n] of _find_lib.ID_DTYPE; policy: rows of _path_lib.FIELDS_DTYPE, or None"""
    raw = blob.tobytes()
    ids = np.zeros(len(certs), dtype=_find_lib.ID_DTYPE)
    if policy is None:
        return ids
    for i, c in enumerate(certs):
        off, length, p = int(c["off"]), int(c["len"]), policy[i]
        ext_off, ext_len = int(p["ext_off"]), int(p["ext_len"])
        if int(p["status"]) in (RANGE, DER) or ext_len == 0:
            continue
        if not xc.inside(off, length, len(raw)) or not within(ext_off, ext_len, off, length):
            ids[i]["status"] = RANGE
            continue
        w = walk_ids(raw, ext_off, ext_off + ext_len)
        for f in w:
            ids[i][f] = w[f]
    return ids


def candidate_keys(raw, c, f, d):
    """the two keys of one certificate, [] where it is no candidate"""
    off, length = int(c["off"]), int(c["len"])
    if int(f["status"]) not in (OK, ALG, SIG) or int(f["key_set"]) == 0 or int(d["status"]) != OK or not xc.inside(off, length, len(raw)):
        return []
    s_off, s_len, k_off, k_len = int(f["subject_off"]), int(f["subject_len"]), int(d["ski_off"]), int(d["ski_len"])
    if not within(s_off, s_len, off, length) or (k_len and (k_len > MAX_KEYID or not within(k_off, k_len, off, length))):
        return []
    name, pset = raw[s_off:s_off + s_len], int(f["key_set"])
    return [(ANY, pset, name, b""), (SKI, pset, name, raw[k_off:k_off + k_len]) if k_len else (NOSKI, pset, name, b"")]


def candidates(blob, certs, fields, ids):
    """key -> the sorted list of the certificates entered under it"""
    raw, table = blob.tobytes(), {}
    for j in range(len(certs)):
        for key in candidate_keys(raw, certs[j], fields[j], ids[j]):
            table.setdefault(key, []).append(j)
    return table


def answer(table, pset, name, key_id, in_group=None):
    """(status, issuer, candidates) of a seeker.  in_group: None, or -- for a table whose overflow list has run over -- the keys known
    to lie in a table group: a lookup of any other key answers SPACE"""
    asked = [(ANY, pset, name, b"")] if not key_id else [(SKI, pset, name, key_id), (NOSKI, pset, name, b"")]
    if in_group is not None and any(k not in in_group for k in asked):
        return SPACE, NO_ISSUER, 0
    hits = sorted(j for k in asked for j in table.get(k, []))
    return (FOUND, hits[0], len(hits)) if hits else (NONE, NO_ISSUER, 0)


def expected_issuers(blob, certs, fields, ids, in_group=None):
    """(results [n] of _find_lib.RESULT_DTYPE, certs_out [n] of _x509_lib.CERT_DTYPE)"""
    raw, table = blob.tobytes(), candidates(blob, certs, fields, ids)
    results = np.zeros(len(certs), dtype=_find_lib.RESULT_DTYPE)
    out = np.array(certs, dtype=_x509_lib.CERT_DTYPE)
    for i, (c, f, d) in enumerate(zip(certs, fields, ids)):
        off, length = int(c["off"]), int(c["len"])
        n_off, n_len, k_off, k_len = int(f["issuer_off"]), int(f["issuer_len"]), int(d["aki_off"]), int(d["aki_len"])
        seeker = (int(f["status"]) == OK and int(f["sig_set"]) != 0 and int(d["status"]) == OK and xc.inside(off, length, len(raw))
                  and within(n_off, n_len, off, length) and (k_len == 0 or (k_len <= MAX_KEYID and within(k_off, k_len, off, length))))
        got = (CERT, NO_ISSUER, 0)
        if seeker:
            got = answer(table, int(f["sig_set"]), raw[n_off:n_off + n_len], raw[k_off:k_off + k_len], in_group)
        results[i]["status"], results[i]["issuer"], results[i]["candidates"] = got
        out[i]["issuer"] = got[1]
    return results, out


def expected_crl_issuers(blob, items, crl_fields, certs, fields, ids, in_group=None):
    """(results [n_crls], items_out [n_crls] of _crl_lib.ITEM_DTYPE)"""
    raw, table = blob.tobytes(), candidates(blob, certs, fields, ids)
    results = np.zeros(len(items), dtype=_find_lib.RESULT_DTYPE)
    out = np.array(items, dtype=_crl_lib.ITEM_DTYPE)
    for c, (item, f) in enumerate(zip(items, crl_fields)):
        off, length = int(item["off"]), int(item["len"])
        n_off, n_len, e_off, e_len = int(f["issuer_off"]), int(f["issuer_len"]), int(f["ext_off"]), int(f["ext_len"])
        seeker = int(f["status"]) == OK and int(f["sig_set"]) != 0 and xc.inside(off, length, len(raw)) and within(n_off, n_len, off, length)
        key_id = b""
        if seeker and e_len:
            seeker = within(e_off, e_len, off, length)
            if seeker:
                w = walk_ids(raw, e_off, e_off + e_len)
                seeker = w["status"] == OK
                key_id = raw[w["aki_off"]:w["aki_off"] + w["aki_len"]] if seeker else b""
        got = answer(table, int(f["sig_set"]), raw[n_off:n_off + n_len], key_id, in_group) if seeker else (CERT, NO_ISSUER, 0)
        results[c]["status"], results[c]["issuer"], results[c]["candidates"] = got
        out[c]["issuer"] = got[1]
    return results, out


def expected_cert_crls(cert_issuers, crl_issuers):
    """cert_crl [n]: the lowest CRL of every certificate's issuer"""
    n, lowest = len(cert_issuers), {}
    for c, ca in enumerate(crl_issuers):
        if int(ca) < n:
            lowest.setdefault(int(ca), c)
    return np.array([lowest.get(int(ca), CRL_NONE) if int(ca) < n else CRL_NONE for ca in cert_issuers], dtype=np.uint32)


def table_slots(n):
    s = 64
    while s < 4 * n:
        s *= 2
    return s


def scratch_bytes(n):
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    s = table_slots(n)
    return r(8 * s) + r(4 * s) + r(4 * s) + r(8 * n) + r(64 * n) + r(4 * OVERFLOW_MAX) + r(4 * n)


# ----------------------------------------------------------------------------------------------------------------------- the cases
KID = bytes(range(0x40, 0x54))  # 20 bytes


def value_cases():
    """(extensions content, status) for every rule of the two values"""
    e, t = pc.ext, xc.tlv
    ski = lambda v: e(SKI_OID, v)  # noqa: E731  (the extnValue's content given whole)
    aki = lambda v: e(AKI_OID, v)  # noqa: E731
    name = t(0xA1, t(0xA4, xc.name(b"ca")))
    out = [(ski_ext(KID) + aki_ext(KID), OK), (b"", OK), (pc.other(0), OK)]
    out += [(ski_ext(bytes(n)), OK if 1 <= n <= 64 else EXT) for n in (0, 1, 20, 32, 64, 65, 127, 128)]
    out += [(aki_ext(bytes(n)), OK if 1 <= n <= 64 else EXT) for n in (0, 1, 20, 32, 64, 65, 127, 128)]
    out += [(aki_ext(), OK), (aki_ext(None, xc.name(b"ca"), b"\x01"), OK), (aki_ext(KID, xc.name(b"ca")), OK),
            (aki_ext(KID, None, b"\x01"), OK), (aki_ext(None, None, b"\x01"), OK), (ski_ext(KID, critical=True), OK)]
    out += [(ski(t(0x04, KID) + b"\x05\x00"), EXT), (ski(t(0x03, KID)), EXT), (ski(b""), EXT), (ski(b"\x04"), EXT), (ski(b"\x04\x81\x14" + KID), EXT),
            (ski(t(0x04, KID)[:-1]), EXT), (ski_ext(KID) + ski_ext(KID), EXT), (aki_ext(KID) + aki_ext(), EXT),
            (aki(t(0x31, t(0x80, KID))), EXT), (aki(t(0x30, t(0x80, KID)) + b"\x00"), EXT), (aki(t(0x30, t(0x82, b"\x01") + t(0x80, KID))), EXT),
            (aki(t(0x30, t(0x82, b"\x01") + name)), EXT), (aki(t(0x30, t(0x80, KID) + t(0x80, KID))), EXT), (aki(t(0x30, t(0x81, KID))), EXT),
            (aki(t(0x30, t(0x80, KID) + name + t(0x82, b"\x01") + b"\x05\x00")), EXT), (aki(t(0x30, b"\x80")), EXT), (aki(t(0x30, b"\x80\x80")), EXT),
            (aki(b"\x30\x03\x80\x02\x01"), EXT), (aki(t(0x30, t(0x9F, KID))), EXT)]
    # the frames: DER, which outranks EXT; the loop's bound
    out += [(ski_ext(KID)[:-1], DER), (b"\x31" + ski_ext(KID)[1:], DER), (ski_ext(KID) + b"\x30", DER),
            (t(0x30, t(0x05, SKI_OID) + t(0x04, t(0x04, KID))), DER), (t(0x30, t(0x06, SKI_OID) + t(0x03, t(0x04, KID))), DER),
            (t(0x30, t(0x06, SKI_OID) + t(0x04, t(0x04, KID)) + b"\x05\x00"), DER), (t(0x30, t(0x06, SKI_OID)), DER),
            (ski_ext(KID) + ski_ext(KID) + b"\x30\x80", DER), (ski_ext(bytes(65)) + b"\x00", DER),
            (b"".join(pc.other(k) for k in range(31)) + ski_ext(KID), OK), (b"".join(pc.other(k) for k in range(32)) + ski_ext(KID), EXT),
            (b"".join(pc.other(k) for k in range(32)), OK), (b"".join(pc.other(k) for k in range(32)) + b"\xff", EXT)]
    return out


# ----------------------------------------------------------------------------------------------------------------------- the batches
def shuffled_chains(n, seed, depth_of=lambda c: 1 + c % 4, with_ids=True):
    """n certificates dealt as chains of depth 1 ... 4 (root first; each chain of one parameter set, its Names of the lengths of
    NAME_LENGTHS in turn, subjectKeyIdentifiers of the lengths of ID_LENGTHS, every second chain's AKIs with the A1 / 82 members), then
    shuffled by a seeded permutation.  Returns (ders in shuffled order, issuers in shuffled order: what a lookup must find)."""
    ders, issuers, chain = [], [], 0
    while len(ders) < n:
        depth, pset, first = min(depth_of(chain), n - len(ders)), xc.SETS[chain % 3], len(ders)
        names = [name_of_len(NAME_LENGTHS[(chain + j) % len(NAME_LENGTHS)], _bytes(b"nm%d" % seed, 7 * chain + j, 40)) for j in range(depth)]
        kids = [_bytes(b"kid%d" % seed, 7 * chain + j, ID_LENGTHS[(chain + j) % 4]) for j in range(depth)]
        for j in range(depth):
            up = max(j - 1, 0)
            exts = []
            if with_ids and (chain + j) % 5 != 4:  # every fifth certificate without identifiers
                exts = [ski_ext(kids[j]), aki_ext(kids[up], names[up] if chain % 2 else None, b"\x01\x02" if chain % 2 else None)]
            if j + 1 < depth:
                exts.insert(0, pc.basic())
            ders.append(cert(pset, pset, names[up], names[j], b"sh%d" % seed, first + j, exts))
            issuers.append(first + up)
        chain += 1
    perm = np.random.default_rng(seed).permutation(n)  # position p holds certificate perm[p]
    where = np.argsort(perm)
    return [ders[q] for q in perm], [int(where[issuers[q]]) for q in perm]
