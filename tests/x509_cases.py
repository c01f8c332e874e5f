"""Cases for the certificate library (include/mldsa_x509.h): a minimal DER builder for X.509 certificates, the list of defects the header
names, and a Python restatement of what the library must produce -- the walk, the link rule and the op layout --, written from the rules
the header states and not from the kernels.  Loads no library.  Not a test file: test_x509_cpu.py and test_gpu_x509.py import it by
name."""
import hashlib

import numpy as np

from fips204_amd import _rec_lib, _x509_lib
from fips204_amd.ml_dsa import certificates_blob

PK_LEN = {44: 1312, 65: 1952, 87: 2592}
SIG_LEN = {44: 2420, 65: 3309, 87: 4627}
SETS = (44, 65, 87)
OK, RANGE, DER, ALG, SIG, ISSUER, NAME, PARSE_ONLY = range(8)
CHECK_NAMES = 1
NO_ISSUER = 0xFFFFFFFF
OID = {s: bytes.fromhex("0609608648016503040311")[:-1] + bytes([0x11 + i]) for i, s in enumerate(SETS)}  # id-ml-dsa-44 / -65 / -87
RSA_ALG = bytes.fromhex("06092a864886f70d0101010500")  # rsaEncryption with NULL parameters: an SPKI algorithm that is not ML-DSA
SEAM_SIZES = (1, 63, 64, 65, 257)
MIXES = ("mod3", "only44", "only87", "all_defect", "tenth_defect")
MUTATION_VALUES = (0x00, 0x7F, 0x80, 0x81, 0x84, 0x85, 0xFF)
MUTATION_SPAN = 130


def _bytes(tag, i, n):
    return hashlib.shake_256(tag + int(i).to_bytes(8, "little")).digest(n)


# ----------------------------------------------------------------------------------------------------------------------- the builder
def der_len(n):
    """the length bytes DER requires for n: short form below 128, else the fewest bytes"""
    if n < 128:
        return bytes([n])
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(body)]) + body


def tlv(tag, content):
    return bytes([tag]) + der_len(len(content)) + bytes(content)


def name(cn):
    """Name with one commonName of 1 ... 300 bytes: the Name TLV's length is short, 0x81 or 0x82 form depending on it"""
    assert 1 <= len(cn) <= 300
    return tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, cn))))


def alg_id(pset):
    return tlv(0x30, OID[pset] if pset in OID else RSA_ALG)


SERIAL = tlv(0x02, b"\x12\x34")
VALIDITY = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))
VERSION = tlv(0xA0, tlv(0x02, b"\x02"))


def tbs(sig_set, key_set, issuer_cn, subject_cn, pk, v3=True, tail=b""):
    """TBSCertificate: [0] version (with v3), the fixed 2-byte serial, the signature algorithm of sig_set, the two Names, two UTCTime
    dates, the SPKI of key_set (anything but 44 / 65 / 87: an RSA algorithm identifier) around pk, and `tail` (unique IDs, extensions)"""
    spki = tlv(0x30, alg_id(key_set) + tlv(0x03, b"\x00" + bytes(pk)))
    return tlv(0x30, (VERSION if v3 else b"") + SERIAL + alg_id(sig_set) + name(issuer_cn) + VALIDITY + name(subject_cn) + spki + tail)


def cert(tbs_der, sig_set, sig):
    return tlv(0x30, bytes(tbs_der) + alg_id(sig_set) + tlv(0x03, b"\x00" + bytes(sig)))


def extensions(n_bytes):
    """an [3] extensions tail of about n_bytes: not walked by the library"""
    return tlv(0xA3, tlv(0x30, tlv(0x30, bytes.fromhex("0603551d13") + tlv(0x04, bytes(n_bytes)))))


def random_cert(sig_set, key_set, issuer_cn, subject_cn, tag, i, v3=True, tail=b""):
    """a certificate of the right shape around random key and signature bytes: what the seam needs, which verifies nothing"""
    pk = _bytes(tag + b"pk", i, PK_LEN.get(key_set, 270))
    return cert(tbs(sig_set, key_set, issuer_cn, subject_cn, pk, v3, tail), sig_set, _bytes(tag + b"sig", i, SIG_LEN[sig_set]))


# ------------------------------------------------------------------------------------------------------------------- the restatement
class Malformed(Exception):
    pass


def take(buf, pos, end):
    """the TLV at buf[pos:end] by the header's rules: (tag, first content byte, position behind the TLV)"""
    window = buf[pos:end]
    if pos > end or len(window) < 2:
        raise Malformed("no room for a header")
    tag, first = window[0], window[1]
    if tag & 0x1F == 0x1F:
        raise Malformed("high tag number")
    if first < 0x80:
        n, header = first, 2
    else:
        k = first - 0x80
        if k == 0 or k > 4:
            raise Malformed("indefinite or too long a length")
        digits = window[2:2 + k]
        if len(digits) < k:
            raise Malformed("length bytes overrun")
        n = int.from_bytes(digits, "big")
        if digits[0] == 0 or n < 128:
            raise Malformed("not the shortest form")
        header = 2 + k
    if header + n > len(window):
        raise Malformed("content overruns")
    return tag, pos + header, pos + header + n


def expect(buf, pos, end, tag):
    got, at, behind = take(buf, pos, end)
    if got != tag:
        raise Malformed("tag %02x where %02x belongs" % (got, tag))
    return at, behind


def set_of_oid(content):
    for pset, oid in OID.items():
        if bytes(content) == oid:
            return pset
    return 0


def walk(der):
    """dict of the certificate's fields relative to its first byte, status among OK / DER / ALG / SIG"""
    out = dict(tbs_off=0, tbs_len=0, sig_off=0, key_off=0, issuer_off=0, issuer_len=0, subject_off=0, subject_len=0, sig_set=0, key_set=0,
               status=DER)
    n = len(der)
    try:
        at, behind = expect(der, 0, n, 0x30)
        if behind != n:
            raise Malformed("bytes behind the certificate")
        tbs_at, tbs_end = expect(der, at, n, 0x30)
        alg_at, alg_end = expect(der, tbs_end, n, 0x30)
        sig_at, sig_end = expect(der, alg_end, n, 0x03)
        if sig_end != n:
            raise Malformed("bytes behind the signature")
        pos = tbs_at
        if take(der, pos, tbs_end)[0] == 0xA0:
            pos = take(der, pos, tbs_end)[2]
        pos = expect(der, pos, tbs_end, 0x02)[1]
        inner = (pos, expect(der, pos, tbs_end, 0x30)[1])
        pos = inner[1]
        issuer = (pos, expect(der, pos, tbs_end, 0x30)[1])
        pos = expect(der, issuer[1], tbs_end, 0x30)[1]
        subject = (pos, expect(der, pos, tbs_end, 0x30)[1])
        spki_at, spki_end = expect(der, subject[1], tbs_end, 0x30)
        kalg_at, kalg_end = expect(der, spki_at, spki_end, 0x30)
        key_at, key_end = expect(der, kalg_end, spki_end, 0x03)
        if key_end != spki_end:
            raise Malformed("bytes behind the key")
    except Malformed:
        return out
    out.update(tbs_off=at, tbs_len=tbs_end - at, issuer_off=issuer[0], issuer_len=issuer[1] - issuer[0], subject_off=subject[0],
               subject_len=subject[1] - subject[0])
    kset = set_of_oid(der[kalg_at:kalg_end])
    if kset and key_end - key_at == 1 + PK_LEN[kset] and der[key_at] == 0:
        out.update(key_set=kset, key_off=key_at + 1)
    sset = set_of_oid(der[alg_at:alg_end])
    if not sset or der[inner[0]:inner[1]] != der[tbs_end:alg_end]:  # the inner TLV is the outer one, byte for byte
        out["status"] = ALG
        return out
    if sig_end - sig_at != 1 + SIG_LEN[sset] or der[sig_at] != 0:
        out["status"] = SIG
        return out
    out.update(status=OK, sig_set=sset, sig_off=sig_at + 1)
    return out


def inside(off, length, blob_len):
    """[off, off + length) lies in [0, blob_len): Python integers, so nothing wraps"""
    return 0 <= off and off + length <= blob_len


def expected(blob, certs, flags=CHECK_NAMES):
    """(fields [n] of _x509_lib.FIELDS_DTYPE, ops [n] of _rec_lib.OP_DTYPE, status uint8 [n]) for a blob (uint8 array) and its
    certificate entries"""
    raw = blob.tobytes()
    n = len(certs)
    fields = np.zeros(n, dtype=_x509_lib.FIELDS_DTYPE)
    ops = np.zeros(n, dtype=_rec_lib.OP_DTYPE)
    status = np.zeros(n, dtype=np.uint8)
    for i, c in enumerate(certs):
        off, length = int(c["off"]), int(c["len"])
        if not inside(off, length, len(raw)) or length < 2:
            fields[i]["status"] = RANGE
            continue
        w = walk(raw[off:off + length])
        fields[i]["status"] = w["status"]
        if w["status"] == DER:
            continue
        for f in ("tbs_len", "issuer_len", "subject_len", "sig_set", "key_set"):
            fields[i][f] = w[f]
        for f in ("tbs_off", "issuer_off", "subject_off"):
            fields[i][f] = off + w[f]
        fields[i]["sig_off"] = off + w["sig_off"] if w["sig_set"] else 0
        fields[i]["key_off"] = off + w["key_off"] if w["key_set"] else 0
    for i, c in enumerate(certs):
        own, issuer = fields[i], int(c["issuer"])
        status[i] = link_rule(raw, fields, own, issuer, n, flags)
        if status[i] == OK:
            ops[i]["pk_off"], ops[i]["sig_off"], ops[i]["set"] = fields[issuer]["key_off"], own["sig_off"], own["sig_set"]
            ops[i]["msg_off"], ops[i]["msg_len"] = own["tbs_off"], own["tbs_len"]
    return fields, ops, status


def link_rule(raw, fields, own, issuer, n, flags):
    if own["status"] != OK:
        return int(own["status"])
    if issuer == NO_ISSUER:
        return PARSE_ONLY
    if issuer >= n:
        return ISSUER
    iss = fields[issuer]
    if iss["status"] in (RANGE, DER) or iss["key_set"] == 0 or iss["key_set"] != own["sig_set"]:
        return ISSUER
    if flags & CHECK_NAMES:
        mine = raw[int(own["issuer_off"]):int(own["issuer_off"]) + int(own["issuer_len"])]
        theirs = raw[int(iss["subject_off"]):int(iss["subject_off"]) + int(iss["subject_len"])]
        if mine != theirs:
            return NAME
    return OK


# ----------------------------------------------------------------------------------------------------------------------- the defects
def split(der):
    """the parts of a certificate the builder made, each a bytes object (whole TLVs unless the name says content)"""
    w = walk(der)
    assert w["status"] != DER
    tbs_at = take(der, w["tbs_off"], len(der))[1]
    tbs_end = w["tbs_off"] + w["tbs_len"]
    parts, pos = {}, tbs_at
    for part in ("version", "serial", "inner", "issuer", "validity", "subject", "spki"):
        tag, at, behind = take(der, pos, tbs_end)
        if part == "version" and tag != 0xA0:
            parts["version"] = b""
            continue
        parts[part] = der[pos:behind]
        if part == "spki":
            _, kat, kend = take(der, at, behind)
            parts["spki_alg"] = der[at:kend]
            parts["key_bits"] = der[take(der, kend, behind)[1]:behind]
        pos = behind
    parts["tail"] = der[pos:tbs_end]
    _, at, behind = take(der, tbs_end, len(der))
    parts["outer"] = der[tbs_end:behind]
    parts["sig_bits"] = der[take(der, behind, len(der))[1]:]
    return parts


def join(p):
    spki = p.get("spki_raw") or tlv(0x30, p["spki_alg"] + tlv(0x03, p["key_bits"]) + p.get("spki_extra", b""))
    body = p["version"] + p["serial"] + p["inner"] + p["issuer"] + p["validity"] + p["subject"] + spki + p["tail"]
    return tlv(0x30, tlv(0x30, body) + p["outer"] + tlv(0x03, p["sig_bits"]))


def _retag(part, tag):
    return bytes([tag]) + part[1:]


TBS_POSITIONS = ("version", "serial", "inner", "issuer", "validity", "subject", "spki")
# name -> the status the header documents (of a certificate that is otherwise valid and whose issuer is valid)
DEFECTS = {
    "indefinite_length": DER, "nonminimal_81_7f": DER, "nonminimal_82_00": DER, "length_85": DER, "high_tag_number": DER,
    "trailing_byte": DER, "len_one_short": DER, "len_one_long": DER, "tbs_overruns": DER,
    **{"wrong_tag_" + part: DER for part in TBS_POSITIONS},
    "spki_trailing": DER, "outer_alg_null_params": ALG, "alg_sets_differ": ALG, "sig_unused_bits": SIG, "sig_one_short": SIG,
    "key_one_short": OK, "spki_other_oid": OK,
}
KEY_SET_ZERO = ("key_one_short", "spki_other_oid")  # status 0, key_set 0: useless as an issuer only


def make_defect(der, defect):
    """(bytes to lay into the blob, the len to declare for them) of a v3 certificate the builder made, with one defect.  For
    len_one_long the caller sees to it that one more byte lies behind the certificate in the blob."""
    p, n = split(der), len(der)
    if defect == "indefinite_length":
        return der[:1] + b"\x80" + der[2:], n
    if defect == "nonminimal_81_7f":      # a serial of 127 bytes behind 81 7F
        p["serial"] = b"\x02\x81\x7f" + bytes([1] * 127)
    elif defect == "nonminimal_82_00":    # the issuer Name behind 82 00 xx
        body = p["issuer"][take(p["issuer"], 0, len(p["issuer"]))[1]:]
        # (83 00 xx xx where the Name is too long for one byte: the first length byte is 0 either way)
        p["issuer"] = (b"\x30\x82\x00" + bytes([len(body)]) if len(body) < 256 else b"\x30\x83\x00" + len(body).to_bytes(2, "big")) + body
    elif defect == "length_85":
        body = p["validity"][2:]
        p["validity"] = b"\x30\x85\x00\x00\x00\x00" + bytes([len(body)]) + body
    elif defect == "high_tag_number":
        p["subject"] = _retag(p["subject"], 0x3F)
    elif defect == "trailing_byte":
        return der + b"\x00", n + 1
    elif defect == "len_one_short":
        return der, n - 1
    elif defect == "len_one_long":
        return der, n + 1
    elif defect == "tbs_overruns":        # the TBS claims the whole rest of the certificate and one byte more
        at = take(der, 0, n)[1]
        assert der[at + 1] == 0x82
        return der[:at + 2] + (n - at - 4 + 1).to_bytes(2, "big") + der[at + 4:], n
    elif defect.startswith("wrong_tag_"):
        part = defect[len("wrong_tag_"):]
        assert p[part], "a v3 certificate expected"
        p[part] = _retag(p[part], {"version": 0xA1, "serial": 0x04}.get(part, 0x31))
        if part == "spki":
            p["spki_raw"] = p["spki"]
    elif defect == "spki_trailing":
        p["spki_extra"] = b"\x05\x00"
    elif defect == "outer_alg_null_params":
        p["outer"] = tlv(0x30, p["outer"][2:] + b"\x05\x00")
    elif defect == "alg_sets_differ":
        last = p["outer"][-1]
        p["outer"] = p["outer"][:-1] + bytes([0x12 if last != 0x12 else 0x13])
    elif defect == "sig_unused_bits":
        p["sig_bits"] = b"\x01" + p["sig_bits"][1:]
    elif defect == "sig_one_short":
        p["sig_bits"] = p["sig_bits"][:-1]
    elif defect == "key_one_short":
        p["key_bits"] = p["key_bits"][:-1]
    elif defect == "spki_other_oid":
        p["spki_alg"] = tlv(0x30, RSA_ALG)
    else:
        raise KeyError(defect)
    out = join(p)
    return out, len(out)


def signed_chain(psets, tag):
    """root -> ... -> leaf, certificate i signed by certificate i - 1's key (the root by its own): psets[i] is the set of certificate i's
    subject key.  Signed by the oracle, which is imported here: the module itself loads nothing.  Returns (ders, issuers)."""
    from oracle import oracle as orc
    keys = [orc.keygen_from_seed(p, _bytes(tag + b"xi", i, 32)) for i, p in enumerate(psets)]
    ders = []
    for i, p in enumerate(psets):
        j = max(i - 1, 0)
        body = tbs(psets[j], p, tag + b"-%d" % j, tag + b"-%d" % i, orc.pk_into_bytes(p, keys[i][0]),
                      tail=extensions(9 * i) if i else b"")
        sig = orc.sign_internal(psets[j], keys[j][1], body, _bytes(tag + b"rnd", i, 32), ctx=b"", mode=orc.MODE_PURE)
        ders.append(cert(body, psets[j], sig))
    return ders, [max(i - 1, 0) for i in range(len(psets))]


# ----------------------------------------------------------------------------------------------------------------------- seam cases
def lay_out(entries, issuers, pad=0, front=0):
    """certificates_blob for (bytes, declared len) entries, with one spare byte behind the last certificate"""
    blob, certs = certificates_blob([e[0] for e in entries], issuers, pad=pad, front=front)
    for i, e in enumerate(entries):
        certs[i]["len"] = e[1]
    return np.concatenate([blob, np.full(1, 0xC3, dtype=np.uint8)]), certs


def chain_issuers(n):
    """chains of depth 3: root (its own issuer), intermediate, leaf, root, ..."""
    return [i if i % 3 == 0 else i - 1 for i in range(n)]


def seam_case(n, mix, seed=0, front=0):
    """(blob, certs) of n random-bytes certificates dealt as chains of depth 3 (each chain of one parameter set, so that they link), the
    gaps cycling 0 ... 15, Names of every length form; with all_defect / tenth_defect every / every tenth certificate carries one of
    the defects in turn"""
    names = list(DEFECTS)
    entries = []
    for i in range(n):
        chain = i // 3
        pset = {"only44": 44, "only87": 87}.get(mix, SETS[chain % 3])
        cn = lambda j: _bytes(b"cn%d" % seed, 3 * chain + j, (4, 1, 130, 300, 17)[(3 * chain + j) % 5])  # noqa: E731
        tail = extensions(20 + i % 50) if i % 4 == 1 else b""
        der = random_cert(pset, pset, cn(max(i % 3 - 1, 0)), cn(i % 3), b"seam%d" % seed, i, tail=tail)
        if mix == "all_defect" or (mix == "tenth_defect" and i % 10 == 9):
            entries.append(make_defect(der, names[(i + seed) % len(names)]))
        else:
            entries.append((der, len(der)))
    return lay_out(entries, chain_issuers(n), pad=list(range(16)), front=front)


def mutation_batch(der):
    """(blob, certs): the certificate with each of its first MUTATION_SPAN bytes set to each of MUTATION_VALUES, every copy its own
    issuer"""
    entries = []
    for pos in range(MUTATION_SPAN):
        for v in MUTATION_VALUES:
            entries.append((der[:pos] + bytes([v]) + der[pos + 1:], len(der)))
    return lay_out(entries, list(range(len(entries))), pad=[3, 0, 7])
