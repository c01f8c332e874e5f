"""Cases for the certificate-issuing library (include/mldsa_x509sign.h) and a Python restatement of what it must produce -- status,
out_certs, ops, totals and every frame byte --, written from the rules the header states and not from the kernels: the TLV reader and
the certificate builder are tests/x509_cases.py's (take / expect / cert), imported and not copied.  Loads no library.  Not a test file:
test_x509sign_cpu.py and test_gpu_x509sign.py import it by name."""
import functools

import numpy as np

import x509_cases as xc
from fips204_amd import _recsign_lib, _x509_lib
from fips204_amd.ml_dsa import tbs_blob

SIG_LEN, PK_LEN, SETS = xc.SIG_LEN, xc.PK_LEN, xc.SETS
OK, RANGE, DER, ALG = xc.OK, xc.RANGE, xc.DER, xc.ALG
ENTRY, KEY, LONG, SPACE = 8, 9, 10, 11
FLAG_RND = 1
NO_ISSUER = xc.NO_ISSUER
FRAME = 22                                              # 4 bytes in front of the TBS, 18 behind it
MAX_TBS = {s: 65517 - SIG_LEN[s] for s in SETS}        # the longest TBS whose certificate keeps the two-byte outer length
N_KEYS = (4, 4, 4)                                      # rows of the three key tables of the seam cases
SEAM_SIZES, MIXES = xc.SEAM_SIZES, xc.MIXES
ITER_BOUND = 32  # MLDSA_OPT_SPEC_MAX as a context starts (tests/long_tail_cases.py): the candidates one round gives one op at most
_bytes = xc._bytes


# ------------------------------------------------------------------------------------------------------------------- restatement
def walk_tbs(tbs, pset):
    """OK, DER or ALG of one TBSCertificate under the set that will sign it, by the header's walk"""
    n = len(tbs)
    try:
        at, behind = xc.expect(tbs, 0, n, 0x30)
        if behind != n:
            raise xc.Malformed("bytes behind the TBS")
        pos = at
        if xc.take(tbs, pos, n)[0] == 0xA0:
            pos = xc.take(tbs, pos, n)[2]
        pos = xc.expect(tbs, pos, n, 0x02)[1]
        inner = xc.expect(tbs, pos, n, 0x30)
        pos = inner[1]
        for _ in ("issuer", "validity", "subject"):
            pos = xc.expect(tbs, pos, n, 0x30)[1]
        spki_at, spki_end = xc.expect(tbs, pos, n, 0x30)
        kalg_end = xc.expect(tbs, spki_at, spki_end, 0x30)[1]
        if xc.expect(tbs, kalg_end, spki_end, 0x03)[1] != spki_end:
            raise xc.Malformed("bytes behind the key")
    except xc.Malformed:
        return DER
    return OK if bytes(tbs[inner[0]:inner[1]]) == xc.OID[pset] else ALG


def status_before_space(raw, r, n_keys):
    """the first rule of ENTRY, KEY, RANGE, LONG, DER, ALG a request breaks: Python integers, so nothing wraps"""
    pset, flags = int(r["set"]), int(r["flags"])
    if pset not in SETS or flags & ~FLAG_RND or int(r["reserved"]) != 0:
        return ENTRY
    if int(r["key"]) >= n_keys[SETS.index(pset)]:
        return KEY
    off, length = int(r["off"]), int(r["len"])
    if not xc.inside(off, length, len(raw)) or length < 2:
        return RANGE
    if flags & FLAG_RND and not xc.inside(int(r["rnd_off"]), 32, len(raw)):
        return RANGE
    if length > MAX_TBS[pset]:
        return LONG
    return walk_tbs(raw[off:off + length], pset)


def expected(blob, reqs, n_keys, out_len):
    """dict(status uint8 [n], out_certs [n] of _x509_lib.CERT_DTYPE, ops [n] of _recsign_lib.OP_DTYPE, totals (accepted, refused,
    out_bytes), frames {i: the certificate around a signature of zeros}) for a blob (uint8 array) and its requests"""
    raw = blob.tobytes()
    n = len(reqs)
    status = np.zeros(n, dtype=np.uint8)
    out_certs = np.zeros(n, dtype=_x509_lib.CERT_DTYPE)
    out_certs["issuer"] = NO_ISSUER
    ops = np.zeros(n, dtype=_recsign_lib.OP_DTYPE)
    frames, at = {}, 0
    for i, r in enumerate(reqs):
        status[i] = status_before_space(raw, r, n_keys)
        if status[i] != OK:
            continue
        pset, off, length = int(r["set"]), int(r["off"]), int(r["len"])
        frame = xc.cert(raw[off:off + length], pset, bytes(SIG_LEN[pset]))
        assert len(frame) == length + FRAME + SIG_LEN[pset] and frame[1] == 0x82
        if at + len(frame) > out_len:
            status[i] = SPACE
        else:
            frames[i] = frame
            out_certs[i] = (at, len(frame), int(r["issuer"]))
            ops[i]["msg_off"], ops[i]["msg_len"], ops[i]["rnd_off"], ops[i]["flags"] = off, length, r["rnd_off"], r["flags"]
            ops[i]["sig_off"], ops[i]["key"], ops[i]["set"] = at + length + FRAME, r["key"], pset
        at += len(frame)  # the need counts every certificate that passes every rule but SPACE
    accepted = int((status == OK).sum())
    return dict(status=status, out_certs=out_certs, ops=ops, totals=(accepted, n - accepted, at), frames=frames)


def framed(before, want, sigs=None):
    """`before` (uint8 array, the output buffer) with every accepted certificate's frame written and its hole left as it was -- or, with
    sigs {i: signature bytes}, holding that signature"""
    out = np.array(before, dtype=np.uint8, copy=True)
    for i, frame in want["frames"].items():
        at, hole = int(want["out_certs"][i]["off"]), int(want["ops"][i]["sig_off"])
        out[at:hole] = np.frombuffer(frame[:hole - at], dtype=np.uint8)
        assert hole - at + SIG_LEN[int(want["ops"][i]["set"])] == len(frame)
        if sigs is not None:
            out[hole:at + len(frame)] = np.frombuffer(sigs[i], dtype=np.uint8)
    return out


def _r(x):
    return (x + 255) // 256 * 256


def plan_bytes(n):
    """mldsa_x509sign_plan_bytes as the header spells it"""
    return _r(16 * ((n + 255) // 256)) + _r(4 * n)


def cert_len(pset, tbs_len):
    return tbs_len + FRAME + SIG_LEN[pset] if pset in SETS and tbs_len <= MAX_TBS[pset] else 0


def out_bytes_max(n, tbs_bytes):
    return tbs_bytes + n * (FRAME + 4627)


# ------------------------------------------------------------------------------------------------------------------- TBSs
def good_tbs(pset, tag, i, tail=b"", v3=True, cns=(b"issuer", b"subject"), key_set=None):
    """a TBSCertificate to be signed by a key of `pset`, around random subject-key bytes"""
    key_set = pset if key_set is None else key_set
    return xc.tbs(pset, key_set, cns[0], cns[1], _bytes(tag + b"pk", i, PK_LEN.get(key_set, 270)), v3, tail)


def tbs_of_len(pset, target, tag=b"edge"):
    """a TBSCertificate of exactly `target` bytes (tens of kilobytes: every nested length is then of the 0x82 form, so one byte more of
    extension is one byte more of TBS)"""
    probe = good_tbs(pset, tag, pset, tail=xc.extensions(40000))
    tbs = good_tbs(pset, tag, pset, tail=xc.extensions(40000 + target - len(probe)))
    assert len(tbs) == target
    return tbs


def _tbs_in(der):
    """the TBSCertificate TLV of a certificate the builder made"""
    at = xc.take(der, 0, len(der))[1]
    return der[at:xc.take(der, at, len(der))[2]]


# defects of the TBS's bytes: name -> status.  The first group is x509_cases.make_defect's, applied to the TBS alone.
BUILDER_DEFECTS = tuple("wrong_tag_" + part for part in xc.TBS_POSITIONS) + ("nonminimal_81_7f", "nonminimal_82_00", "length_85",
                                                                             "high_tag_number", "spki_trailing")
BYTE_DEFECTS = {**{name: DER for name in BUILDER_DEFECTS}, "inner_oid_other_set": ALG, "inner_oid_null_params": ALG,
                "trailing_byte": DER, "len_one_short": DER}
# defects of the entry: name -> status
ENTRY_DEFECTS = {"unknown_set": ENTRY, "flag_bit_1": ENTRY, "reserved": ENTRY, "key_is_n_keys": KEY, "off_wraps": RANGE, "len_zero": RANGE,
                 "len_one": RANGE, "ends_one_past_blob": RANGE, "off_behind_blob": RANGE, "rnd_one_past_blob": RANGE, "rnd_wraps": RANGE}
DEFECTS = {**BYTE_DEFECTS, **ENTRY_DEFECTS}


def byte_defect(tbs, pset, name):
    """(bytes to lay into the blob, the len to declare for them) of a v3 TBS the builder made, with one defect of its bytes"""
    if name in BUILDER_DEFECTS:
        data, _ = xc.make_defect(xc.cert(tbs, pset, bytes(SIG_LEN[pset])), name)
        out = _tbs_in(data)
        return out, len(out)
    if name in ("inner_oid_other_set", "inner_oid_null_params"):
        p = xc.split(xc.cert(tbs, pset, bytes(SIG_LEN[pset])))
        p["inner"] = xc.alg_id(SETS[(SETS.index(pset) + 1) % 3]) if name == "inner_oid_other_set" else xc.tlv(0x30, xc.OID[pset] + b"\x05\x00")
        out = _tbs_in(xc.join(p))
        return out, len(out)
    if name == "trailing_byte":
        return tbs + b"\x00", len(tbs) + 1
    if name == "len_one_short":
        return tbs, len(tbs) - 1
    raise KeyError(name)


def entry_defect(reqs, i, name, blob_len, n_keys=N_KEYS):
    """damages entry i (of a request that is otherwise accepted) with one of ENTRY_DEFECTS"""
    r = reqs[i]
    if name == "unknown_set":
        r["set"] = (43, 0, 66, 255)[i % 4]
    elif name == "flag_bit_1":
        r["flags"] = int(r["flags"]) | (2, 0x80)[i % 2]
    elif name == "reserved":
        r["reserved"] = 1 + i % 0xFFFF
    elif name == "key_is_n_keys":
        r["key"] = n_keys[SETS.index(int(r["set"]))]
    elif name == "off_wraps":
        r["off"] = 2 ** 64 - 8
    elif name == "len_zero":
        r["len"] = 0
    elif name == "len_one":
        r["len"] = 1
    elif name == "ends_one_past_blob":
        r["off"] = blob_len + 1 - int(r["len"])
    elif name == "off_behind_blob":
        r["off"], r["len"] = blob_len + 1, 2
    elif name == "rnd_one_past_blob":
        r["flags"], r["rnd_off"] = FLAG_RND, blob_len + 1 - 32
    elif name == "rnd_wraps":
        r["flags"], r["rnd_off"] = FLAG_RND, 2 ** 64 - 16
    else:
        raise KeyError(name)


def lay_out(entries, pad=0, front=0):
    """tbs_blob for entries (pset, key, bytes, declared len, rnd or None, issuer), with 40 spare bytes behind the last field"""
    blob, reqs = tbs_blob([(e[0], e[1], e[2], e[4], e[5]) for e in entries], pad=pad, front=front)
    for i, e in enumerate(entries):
        reqs[i]["len"] = e[3]
    return np.concatenate([blob, np.full(40, 0xC3, dtype=np.uint8)]), reqs


def _entry(pset, key, tbs, rnd, issuer, defect=None):
    data, length = (tbs, len(tbs)) if defect not in BYTE_DEFECTS else byte_defect(tbs, pset, defect)
    return (pset, key, data, length, rnd, issuer)


def defect_batch():
    """(blob, reqs, {defect: index}): every defect between two valid neighbours, the sets in turn"""
    entries, at, late = [], {}, []
    for k, name in enumerate(DEFECTS):
        pset = SETS[k % 3]
        rnd = None if k % 2 else _bytes(b"drnd", k, 32)
        for j in range(3):
            tbs = good_tbs(pset, b"def", 3 * k + j, tail=xc.extensions(k) if j == 1 else b"")
            entries.append(_entry(pset, (k + j) % 4, tbs, rnd, len(entries), name if j == 1 else None))
        at[name] = len(entries) - 2
        if name in ENTRY_DEFECTS:
            late.append(name)
    blob, reqs = lay_out(entries, pad=[0, 3, 8, 13, 5], front=2)
    for name in late:
        entry_defect(reqs, at[name], name, blob.size)
    return blob, reqs, at


def seam_case(n, mix, seed=0, front=0):
    """(blob, reqs) of n requests dealt as chains of depth 3 (each chain of one parameter set), the gaps cycling 0 ... 15, every third
    without rnd, keys dealt round-robin, Names and extension tails of varying length; with all_defect / tenth_defect every / every tenth
    request carries one of DEFECTS in turn"""
    names = list(DEFECTS)
    entries, late = [], []
    for i in range(n):
        chain = i // 3
        pset = {"only44": 44, "only87": 87}.get(mix, SETS[chain % 3])
        cn = lambda j: _bytes(b"scn%d" % seed, 3 * chain + j, (4, 1, 130, 300, 17)[(3 * chain + j) % 5])  # noqa: E731
        tail = xc.extensions(20 + (7 * i) % 50) if i % 4 != 2 else b""
        tbs = good_tbs(pset, b"sseam%d" % seed, i, tail=tail, cns=(cn(max(i % 3 - 1, 0)), cn(i % 3)), v3=i % 5 != 4)
        rnd = None if i % 3 == 2 else _bytes(b"srnd%d" % seed, i, 32)
        defect = names[(i + seed) % len(names)] if mix == "all_defect" or (mix == "tenth_defect" and i % 10 == 9) else None
        if defect in BUILDER_DEFECTS or defect in ("inner_oid_other_set", "inner_oid_null_params"):
            tbs = good_tbs(pset, b"sseam%d" % seed, i, tail=tail, cns=(cn(0), cn(1)))  # (the builder's defects want a v3 TBS)
        entries.append(_entry(pset, i % 4, tbs, rnd, xc.chain_issuers(n)[i], defect))
        if defect in ENTRY_DEFECTS:
            late.append((i, defect))
    blob, reqs = lay_out(entries, pad=list(range(16)), front=front)
    for i, defect in late:
        entry_defect(reqs, i, defect, blob.size)
    return blob, reqs


def mutation_batch(tbs, pset=44):
    """(blob, reqs): the TBS with each of its first xc.MUTATION_SPAN bytes set to each of xc.MUTATION_VALUES"""
    entries = []
    for pos in range(xc.MUTATION_SPAN):
        for v in xc.MUTATION_VALUES:
            entries.append((pset, len(entries) % 4, tbs[:pos] + bytes([v]) + tbs[pos + 1:], len(tbs), None, len(entries)))
    return lay_out(entries, pad=[3, 0, 7])


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(blob, reqs, want status): per set a TBS of exactly the LONG bound and one of a byte more, small ones between them"""
    entries, status = [], []
    for pset in SETS:
        for extra in (0, 1):
            entries.append(_entry(pset, 1, tbs_of_len(pset, MAX_TBS[pset] + extra), None, len(entries)))
            entries.append(_entry(pset, 2, good_tbs(pset, b"edge-s", len(entries)), _bytes(b"ernd", pset, 32), len(entries)))
            status += [LONG if extra else OK, OK]
    blob, reqs = lay_out(entries, pad=[5, 0, 11])
    return blob, reqs, status


def alignment_batch(front=0):
    """(blob, reqs) of 65 requests whose TBS lengths grow by one byte each: over the batch every residue mod 16 occurs both for the TBS's
    place in the blob and for the certificate's place in the output buffer"""
    entries = [_entry(SETS[i % 3], i % 4, good_tbs(SETS[i % 3], b"align", i, tail=xc.extensions(i)), None if i % 2 else _bytes(b"arnd", i, 32), i)
               for i in range(65)]
    return lay_out(entries, pad=[0, 9, 2, 7], front=front)


# ------------------------------------------------------------------------------------------------------------------- signing cases
SIGN_N_KEYS = (2, 2, 2)


def key_seeds():
    """{pset: the seeds of the two issuer keys of the signing cases}"""
    return {pset: [bytes([0x30 + 16 * c + j]) * 32 for j in range(2)] for c, pset in enumerate(SETS)}


@functools.lru_cache(maxsize=None)
def oracle_keys():
    from oracle import oracle as orc
    return {pset: [orc.keygen_from_seed(pset, xi) for xi in seeds] for pset, seeds in key_seeds().items()}


def signing_requests(n, tag):
    """n requests (pset, key_row, tbs, rnd or None, issuer): sets dealt i mod 3, the two keys of a set in turn, every other request
    deterministic, TBSs of growing length around random subject keys"""
    return [(SETS[i % 3], (i // 3) % 2, good_tbs(SETS[i % 3], tag, i, tail=xc.extensions(i % 40) if i % 3 else b""),
             None if i % 2 else _bytes(tag + b"rnd", i, 32), i if i % 3 == 0 else i - 1) for i in range(n)]


@functools.lru_cache(maxsize=None)
def chain_requests():
    """requests: four chains root -> intermediate -> leaf, one per parameter set and one that crosses them, issued in ONE
    batch: request i's TBS carries the public key of subject i and is signed by its issuer's key.  Each subject's key is one of the two
    keys of its set, so the issuer's key row is known: row = the issuer's index mod 2."""
    from oracle import oracle as orc
    keys = oracle_keys()
    reqs, base = [], 0
    for psets, tag in (((44, 44, 44), b"i44"), ((65, 65, 65), b"i65"), ((87, 87, 87), b"i87"), ((87, 65, 44), b"ix")):
        for j, p in enumerate(psets):
            i, iss = base + j, base + max(j - 1, 0)
            iss_set = psets[max(j - 1, 0)]
            pk = orc.pk_into_bytes(p, keys[p][i % 2][0])
            tbs = xc.tbs(iss_set, p, tag + b"-%d" % max(j - 1, 0), tag + b"-%d" % j, pk, tail=xc.extensions(9 * j) if j else b"")
            reqs.append((iss_set, iss % 2, tbs, None if i % 2 else _bytes(tag + b"rnd", i, 32), iss))
        base += 3
    return reqs


def signing_cases():
    """name -> requests: every batch the GPU file signs"""
    chains = list(chain_requests())
    wrong = list(chains)
    wrong[4] = (wrong[4][0], 1 - wrong[4][1]) + wrong[4][2:]  # the 65 intermediate under the other key row of its issuer's set
    return {"pass65": signing_requests(65, b"p65"), "pass257": signing_requests(257, b"p257"), "chains": chains, "chains_wrong_row": wrong,
            "front": signing_requests(7, b"front")}


@functools.lru_cache(maxsize=None)
def oracle_signed(name):
    """(signatures, iterations) of the oracle for signing_cases()[name]: pure ML-DSA, empty context, rnd of zeros where there is none"""
    from oracle import oracle as orc
    keys = oracle_keys()
    out = [orc.sign_internal(pset, keys[pset][key][1], tbs, rnd or bytes(32), ctx=b"", mode=orc.MODE_PURE, want_iters=True)
           for pset, key, tbs, rnd, _ in signing_cases()[name]]
    return [s for s, _ in out], [it for _, it in out]
