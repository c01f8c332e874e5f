"""The revocation-list library on the device (include/mldsa_crl.h): mldsa_crl_parse, mldsa_crl_ops, mldsa_crl_table and mldsa_crl_check byte
for byte against the restatement of tests/crl_cases.py -- the shapes that meet the wave seam and the LDS window's edges, every defect
alone and among valid neighbours, a sweep of single-byte changes, the link rules, the SPACE rule under guard patterns, the lookup with
its probing, and whole chains with signed CRLs through the Python front against the oracle."""
from gpu_common import *  # noqa: F401,F403

import crl_cases as cc
import x509_cases as xc
from fips204_amd import _crl_lib, _rec_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsa, MlDsaRevocationLists

pytestmark = pytest.mark.gpu

CANARY = 0x77
ROWS = 3  # canary rows behind each output array


@pytest.fixture(scope="module")
def rl(hp):
    return MlDsaRevocationLists(hotpath=hp)


def guarded(nbytes, extra):
    return torch.full((nbytes + extra,), CANARY, dtype=torch.uint8, device="cuda")


def blob_dev(blob, shift=0):
    """the blob on the device, `shift` bytes into its allocation (so its address is that far from 16-byte alignment)"""
    t = torch.full((blob.size + shift + 1,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + blob.size] = torch.from_numpy(blob.copy())
    assert t.data_ptr() % 16 == 0
    return t[shift:shift + blob.size]


def rows_dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).cuda()


def run_ops(rl, blob, items, cert_fields, max_entries, flags=cc.CHECK_NAMES, shift=0):
    """mldsa_crl_ops into guarded buffers: a dict of the device tensors (b, items, cert_fields, fields, entries, status, totals) and of
    the five results as numpy arrays (got), after checking the guard rows behind every written buffer"""
    n = len(items)
    d = dict(b=blob_dev(blob, shift), items=rl.items_tensor(items)[:n * 16], cert_fields=rows_dev(cert_fields))
    d["fields"] = guarded(n * 88, ROWS * 88)
    d["entries"] = guarded(max_entries * 32, ROWS * 32)
    ops = guarded(n * 40, ROWS * 40)
    d["status"] = guarded(n, ROWS)
    d["totals"] = guarded(40, ROWS * 8)
    scratch = guarded(rl.lib.mldsa_crl_scratch_bytes(n), 256)
    _crl_lib.check(rl.lib.mldsa_crl_ops(rl.hp._h, _ptr(d["b"]), d["b"].numel(), _ptr(d["items"]), n, _ptr(d["cert_fields"]), len(cert_fields), flags,
                                        _ptr(d["fields"]), _ptr(d["entries"]), max_entries, _ptr(ops), _ptr(d["status"]), _ptr(d["totals"]),
                                        _ptr(scratch), rl.lib.mldsa_crl_scratch_bytes(n), _stream(rl.device)))
    f, e, o, st, t, sc = host(d["fields"]), host(d["entries"]), host(ops), host(d["status"]), host(d["totals"]), host(scratch)
    assert (f[n * 88:] == CANARY).all() and (e[max_entries * 32:] == CANARY).all() and (o[n * 40:] == CANARY).all()
    assert (st[n:] == CANARY).all() and (t[40:] == CANARY).all() and (sc[rl.lib.mldsa_crl_scratch_bytes(n):] == CANARY).all()
    d["got"] = (f[:n * 88].view(_crl_lib.FIELDS_DTYPE), e[:max_entries * 32].view(_crl_lib.ENTRY_DTYPE), o[:n * 40].view(_rec_lib.OP_DTYPE),
                st[:n], t[:40].view(_crl_lib.TOTALS_DTYPE))
    for k in ("fields", "entries", "status", "totals"):
        d[k] = d[k][:{"fields": n * 88, "entries": max_entries * 32, "status": n, "totals": 40}[k]]
    return d


def check_ops(got, want):
    for g, w, what in zip(got, want, ("fields", "entries", "ops", "status", "totals")):
        if not np.array_equal(g, w):
            bad = [i for i in range(len(w)) if g[i] != w[i]]
            raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], g[bad[0]], w[bad[0]]))


def ops_match(rl, case, max_entries=None, flags=cc.CHECK_NAMES, shift=0):
    blob, certs, items, cert_fields = case
    m = cc.max_entries_of(items) if max_entries is None else max_entries
    d = run_ops(rl, blob, items, cert_fields, m, flags, shift)
    want = cc.expected(blob, items, cert_fields, m, flags)
    check_ops(d["got"], want)
    return d, want


def run_table(rl, d):
    table, _ = rl.table_device(d["entries"], d["totals"].view(torch.int64))
    t = host(table).view(np.uint32)
    assert not host(d["totals"]).view(_crl_lib.TOTALS_DTYPE)[0]["overflow"]
    return table, t


def run_check(rl, d, table, certs, cert_fields, cover, crl_ok=None):
    n = len(certs)
    rev = guarded(n, 64)
    got = rl.check_device(d["b"], rows_dev(certs), rows_dev(cert_fields), kidx_dev(cover), d["items"], d["fields"], d["status"],
                          None if crl_ok is None else dev(np.asarray(crl_ok, dtype=np.uint8)), d["entries"], table, revocation=rev)
    out = host(rev)
    assert (out[n:] == CANARY).all() and got.data_ptr() == rev.data_ptr()
    return out[:n]


# ------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", cc.SEAM_SIZES)
def test_mixed_sets_match_the_restatement_byte_for_byte(rl, n):
    shift = (0, 1, 3, 15, 8)[cc.SEAM_SIZES.index(n)]
    d, want = ops_match(rl, cc.seam_case(n, seed=n % 7, defect_every=0 if n in (1, 64) else 5), shift=shift)
    assert (want[3] == 0).sum() >= n - n // 5 and int(want[4][0]["accepted"]) + int(want[4][0]["refused"]) == n
    # mldsa_crl_parse on its own gives the rows of the walk
    blob, certs, items, _ = cc.seam_case(n, seed=n % 7, defect_every=5)
    fields = guarded(n * 88, 88)
    b = blob_dev(blob, shift)
    _crl_lib.check(rl.lib.mldsa_crl_parse(rl.hp._h, _ptr(b), b.numel(), _ptr(rl.items_tensor(items)), n, _ptr(fields), _stream(rl.device)))
    f = host(fields)
    assert (f[n * 88:] == CANARY).all() and np.array_equal(f[:n * 88].view(_crl_lib.FIELDS_DTYPE), cc.expected_parse(blob, items))


CARRY_N = 64 * 256 + 1  # 65 workgroups of the scan: the one-wave offsets kernel goes round its carry loop a second time
CARRY_AT = (0, 255, 256, 16127, 16128, 16383, 16384)  # the accepted few: both ends of the first and the 64th workgroup, and the 65th


def test_placement_scan_carries_past_64_workgroups(rl):
    """16 385 CRLs of which seven are accepted; every other one is a RANGE refusal (no length, or an offset behind the blob's end), so
    the blob stays seven CRLs long.  Then the same with one slot too few: the first CRL whose slots do not fit is the one behind the
    carry."""
    crls = [cc.random_crl(cc.SETS[j % 3], cc.CA_CN[cc.SETS[j % 3]], b"carry", j, 2 + j) for j in range(len(CARRY_AT))]
    blob, certs, few, cert_fields = cc.lay_out(cc.ca_certs(), [0, 1, 2], [(d, len(d)) for d in crls], [j % 3 for j in range(len(crls))],
                                               pad=[0, 5, 11, 2], front=1)
    items = np.zeros(CARRY_N, dtype=few.dtype)
    items["off"][1::2], items["len"][1::2] = blob.size + 1, 100  # behind the end; the even ones have no length
    items[list(CARRY_AT)] = few
    need = int(cc.expected(blob, items, cert_fields, cc.max_entries_of(few))[4][0]["slots"])  # the sum of the seven bounds
    d, want = ops_match(rl, (blob, certs, items, cert_fields), max_entries=need, shift=1)
    fields, entries, ops, status, totals = want
    assert np.nonzero(status == cc.OK)[0].tolist() == list(CARRY_AT) and (status == cc.RANGE).sum() == CARRY_N - len(CARRY_AT)
    assert fields["count"][list(CARRY_AT)].tolist() == [2 + j for j in range(len(CARRY_AT))]
    assert int(fields[CARRY_AT[-1]]["first"]) == need - int(fields[CARRY_AT[-1]]["revoked_len"]) // cc.ENTRY_MIN > 20
    assert (int(totals[0]["accepted"]), int(totals[0]["refused"]), int(totals[0]["slots"])) == (len(CARRY_AT), CARRY_N - len(CARRY_AT), need)
    d, want = ops_match(rl, (blob, certs, items, cert_fields), max_entries=need - 1, shift=1)
    assert np.nonzero(want[3] == cc.SPACE)[0].tolist() == [CARRY_AT[-1]] and int(want[4][0]["accepted"]) == len(CARRY_AT) - 1


@pytest.mark.parametrize("shift", (0, 1, 7, 15))
def test_entry_counts_at_the_wave_seam_and_two_window_reloads(rl, shift):
    cas = cc.ca_certs()
    crls = [cc.random_crl(cc.SETS[k % 3], cc.CA_CN[cc.SETS[k % 3]], b"count", k, count, next_update=k % 2 == 0)
            for k, count in enumerate(cc.ENTRY_COUNTS * 2)]
    case = cc.lay_out(cas, [0, 1, 2], [(d, len(d)) for d in crls], [k % 3 for k in range(len(crls))], pad=[0, 5, 11, 2], front=shift)
    d, want = ops_match(rl, case, shift=shift)
    assert want[0]["count"].tolist() == list(cc.ENTRY_COUNTS) * 2 and not want[3].any()
    assert max(int(x) for x in want[0]["revoked_len"]) > 2 * 1024 + 64  # the 130-entry list outgrows two windows


def test_an_entry_that_outgrows_the_window(rl):
    # 1.5 KiB of crlEntryExtensions in the middle of a list: the entry is longer than the window, the hop leaves it in one step
    big = cc.entry(b"\x02\x03", ext=cc.tlv(0x30, bytes(range(256)) * 6))
    entries = cc.random_entries(b"big", 0, 40) + [big] + cc.random_entries(b"big", 1, 40)
    der = cc.join(cc.parts(65, cc.CA_CN[65], entries, xc._bytes(b"bigsig", 0, xc.SIG_LEN[65])))
    assert len(big) > 1536
    for shift in (0, 9):
        d, want = ops_match(rl, cc.lay_out(cc.ca_certs(), [0, 1, 2], [(der, len(der))], [1], pad=3), shift=shift)
        assert want[3].tolist() == [0] and int(want[0][0]["count"]) == 81 and want[1][40]["serial"][:2].tolist() == [2, 3]


@pytest.mark.parametrize("shift", range(16))
def test_an_entry_header_that_straddles_the_window_edge(rl, shift):
    """at every alignment of the CRL: 49 entries of 20 bytes and one sized so that the next entry's header begins on the last byte of
    the first window (frame coordinate ws + 1023) -- its second byte lies in the next one"""
    small = [cc.entry(bytes([1 + k])) for k in range(49)]
    tail = cc.random_entries(b"straddle", shift, 9)

    def build(filler):
        return cc.join(cc.parts(44, cc.CA_CN[44], small + [cc.entry(b"\x7f", ext=bytes(filler))] + tail, xc._bytes(b"ssig", shift, xc.SIG_LEN[44])))

    probe = build(6)
    case = cc.lay_out(cc.ca_certs(), [0, 1, 2], [(probe, len(probe))], [0], pad=shift)
    off = int(case[2][0]["off"])
    revoked_at = ((shift + off) % 16) + cc.walk_crl(probe)["revoked_off"]  # frame coordinate of the list's first byte
    target = (revoked_at & ~15) + 1023 - revoked_at  # bytes of the list in front of the straddling header
    filler = target - 49 * 20 - 22
    assert 6 <= filler <= 21
    der = build(filler)
    case = cc.lay_out(cc.ca_certs(), [0, 1, 2], [(der, len(der))], [0], pad=shift)
    w = cc.walk_crl(der)
    rows = cc.list_entries(der, w)
    assert int(case[2][0]["off"]) == off and w["revoked_off"] == cc.walk_crl(probe)["revoked_off"]
    assert revoked_at + rows[50][1] - w["revoked_off"] == (revoked_at & ~15) + 1023 and len(rows) == 59
    d, want = ops_match(rl, case, shift=shift)
    assert want[3].tolist() == [0] and int(want[0][0]["count"]) == 59


# ------------------------------------------------------------------------------------------------------------------ defects
def test_every_defect_among_valid_neighbours_and_alone(rl):
    names = list(cc.DEFECTS)
    cas = cc.ca_certs()
    crls, issuers, at = [], [], {}
    for k, defect in enumerate(names):
        pset = cc.SETS[k % 3]
        good = [cc.random_parts(pset, cc.CA_CN[pset], b"nb", 3 * k + j, 3 + (k + j) % 5) for j in range(3)]
        at[defect] = len(crls) + 1
        crls += [(cc.join(good[0]), len(cc.join(good[0]))), cc.make_defect(good[1], defect), (cc.join(good[2]), len(cc.join(good[2])))]
        issuers += [k % 3] * 3
    case = cc.lay_out(cas, [0, 1, 2], crls, issuers, pad=[0, 3, 8, 13], front=2)
    d, want = ops_match(rl, case, shift=3)
    fields, entries, ops, status, totals = d["got"]
    for defect, i in at.items():
        assert status[i] == cc.DEFECTS[defect], defect
        assert ops[i].tobytes() == bytes(40) and fields[i]["count"] == 0 and not (entries["crl"][entries["serial_len"] != 0] == i).any(), defect
        for j in (i - 1, i + 1):  # the neighbours are untouched
            assert status[j] == 0 and ops[j]["set"] in cc.SETS and fields[j]["count"] >= 3, defect
    # one byte short with the missing byte in the blob behind it: malformed, not accepted
    i = at["len_one_short"]
    assert case[0][int(case[2][i]["off"]) + int(case[2][i]["len"])] == crls[i][0][-1] and status[i] == cc.DER
    # and each alone: a call of one CRL
    for k, defect in enumerate(names):
        one = cc.lay_out(cas, [0, 1, 2], [crls[at[defect]]], [k % 3], pad=k % 16)
        d, want = ops_match(rl, one, shift=k % 16)
        assert want[3].tolist() == [cc.DEFECTS[defect]], defect


def test_range_rule_and_the_ends_of_the_blob(rl):
    good = cc.random_crl(44, cc.CA_CN[44], b"rng", 0, 4)
    blob, certs, items, cert_fields = cc.lay_out(cc.ca_certs(), [0, 1, 2], [(good, len(good))] * 8, [0] * 8, pad=0)
    blob = blob[:-1]  # flush against the end of the blob
    assert int(items[7]["off"]) + len(good) == blob.size
    items[1]["off"], items[1]["len"] = blob.size - 1, 2            # ends one byte behind the blob
    items[2]["off"] = 2 ** 64 - 1                                  # no wrap gets past the test
    items[3]["len"] = 1                                            # shorter than a header
    items[4]["off"], items[4]["len"] = blob.size, 0
    items[5]["off"], items[5]["len"] = blob.size - 2, 2            # the last two bytes: inside, and malformed
    items[6]["len"] = 2 ** 32 - 1
    for shift in (0, 1):
        d, want = ops_match(rl, (blob, certs, items, cert_fields), max_entries=64, shift=shift)
        assert want[3].tolist() == [0, cc.RANGE, cc.RANGE, cc.RANGE, cc.RANGE, cc.DER, cc.RANGE, 0]


def test_single_byte_mutation_sweep(rl):
    ca = cc.ca_certs()[0]
    # the first 130 bytes of a CRL: the headers, the version, the algorithm, the issuer Name, the dates, the list's header and first entries
    der = cc.random_crl(44, cc.CA_CN[44], b"mut", 0, 5)
    case = cc.mutation_batch(der, range(xc.MUTATION_SPAN), ca)
    assert len(case[2]) == xc.MUTATION_SPAN * len(xc.MUTATION_VALUES) == 910
    d, want = ops_match(rl, case, shift=1)
    hist = np.bincount(want[3], minlength=22)
    assert hist[cc.ALG] == 77 and min(hist[cc.DER], hist[cc.VERSION], hist[cc.NAME], hist[cc.ENTRY], hist[cc.OK]) > 0 and hist.sum() == 910
    # one whole entry in the middle of a 65-entry list
    p = cc.random_parts(44, cc.CA_CN[44], b"mut", 1, 65)
    der = cc.join(p)
    mid = cc.list_entries(der, cc.walk_crl(der))[32][1]
    case = cc.mutation_batch(der, range(mid, mid + len(p["entries"][32])), ca)
    d, want = ops_match(rl, case, shift=6)
    hist = np.bincount(want[3], minlength=22)
    assert hist[cc.ENTRY] > 0 and hist[cc.OK] > 0 and hist[cc.ENTRY] + hist[cc.OK] == len(case[2])
    assert set(int(c) for c in want[0]["count"]) == {0, 65}


# ------------------------------------------------------------------------------------------------------------------ the link
def test_link_rules(rl):
    cn = {k: b"n" * k for k in (40, 51, 52, 116, 300)}  # Names of 53, 64, 65, 129 and 321 bytes: one step of the comparison and more
    last = lambda b: b[:-1] + b"N"   # noqa: E731
    first = lambda b: b"N" + b[1:]   # noqa: E731
    certs_der = [xc.random_cert(87, 87, c, c, b"lk", k) for k, c in enumerate(cn.values())]
    rsa = xc.random_cert(44, 0, b"rsa", b"rsa", b"lk", 90)                            # its key is no ML-DSA key
    broken = xc.make_defect(xc.random_cert(87, 87, b"b", b"b", b"lk", 91), "wrong_tag_subject")[0]
    badsig = xc.make_defect(certs_der[1], "sig_one_short")[0]                       # its own signature field is bad: it still lends its key
    cas = certs_der + [rsa, broken, badsig, xc.random_cert(65, 65, cn[51], cn[51], b"lk", 92)]
    n_ca = len(cas)
    crls, issuers = [], []
    for k, c in enumerate(cn.values()):  # under each root: a CRL that names it, one whose issuer Name differs in the last byte, one in the first
        crls += [cc.random_crl(87, c, b"lk", 3 * k, 2), cc.random_crl(87, last(c), b"lk", 3 * k + 1, 2), cc.random_crl(87, first(c), b"lk", 3 * k + 2, 2)]
        issuers += [k, k, k]
    n0 = len(crls)
    crls += [cc.random_crl(87, cn[51] + b"n", b"lk", 90, 1),      # n0: an issuer Name one byte longer than the root's
             cc.random_crl(87, cn[51][:-1], b"lk", 91, 1),        # n0 + 1: one byte shorter
             cc.random_crl(44, b"rsa", b"lk", 92, 1),             # n0 + 2: under the RSA key
             cc.random_crl(44, cn[51], b"lk", 93, 1),             # n0 + 3: a 44 signature under the 87 root: cross-set
             cc.random_crl(87, b"b", b"lk", 94, 1),               # n0 + 4: under the malformed certificate
             cc.random_crl(87, cn[51], b"lk", 95, 1),             # n0 + 5: under the certificate with the bad signature field
             cc.random_crl(87, cn[51], b"lk", 96, 1),             # n0 + 6: issuer out of range
             cc.random_crl(87, cn[51], b"lk", 97, 1),             # n0 + 7: issuer out of range by far
             cc.random_crl(65, cn[51], b"lk", 98, 1)]             # n0 + 8: the right Name, under the 65 CA of that Name
    issuers += [1, 1, n_ca - 4, 1, n_ca - 3, n_ca - 2, n_ca, 2 ** 32 - 1, n_ca - 1]
    case = cc.lay_out(cas, list(range(n_ca)), [(d, len(d)) for d in crls], issuers, pad=[1, 6, 11, 0], front=5)
    d, want = ops_match(rl, case, shift=3)
    assert want[3].tolist() == [0, cc.NAME, cc.NAME] * len(cn) + [cc.NAME, cc.NAME, cc.ISSUER, cc.ISSUER, cc.ISSUER, 0, cc.ISSUER, cc.ISSUER, 0]
    assert not (want[1]["crl"][want[1]["serial_len"] != 0] == 1).any()  # a CRL refused by the link lists nobody
    d, want0 = ops_match(rl, case, flags=0)  # without the flag no Name is compared
    assert want0[3].tolist()[:n0 + 2] == [0] * (n0 + 2)


def test_link_does_not_follow_a_fields_row_out_of_the_blob(rl):
    cas = cc.ca_certs()
    crls = [cc.random_crl(44, cc.CA_CN[44], b"tamper", i, 2) for i in range(4)]
    blob, certs, items, cert_fields = cc.lay_out(cas + [cas[0]] * 3, list(range(6)), [(d, len(d)) for d in crls], [0, 3, 4, 5], pad=3)
    assert cc.expected(blob, items, cert_fields, 16)[3].tolist() == [0, 0, 0, 0]
    cert_fields[3]["subject_off"] = blob.size - 3                       # ends behind the blob
    cert_fields[4]["subject_off"] = 2 ** 64 - 8                         # wraps
    cert_fields[5]["subject_len"] = cert_fields[0]["subject_len"] + 1   # another length
    d, want = ops_match(rl, (blob, certs, items, cert_fields), max_entries=16, shift=1)
    assert want[3].tolist() == [0, cc.NAME, cc.NAME, cc.NAME] and not d["got"][2][1:].view(np.uint8).any()


# ------------------------------------------------------------------------------------------------------------------ SPACE
def test_space_rule_under_guard_patterns(rl):
    cas = cc.ca_certs()
    crls = [cc.random_crl(cc.SETS[k % 3], cc.CA_CN[cc.SETS[k % 3]], b"space", k, count) for k, count in enumerate((3, 0, 65, 1, 7))]
    case = cc.lay_out(cas, [0, 1, 2], [(d, len(d)) for d in crls], [k % 3 for k in range(5)], pad=[4, 9])
    bounds = [cc.walk_crl(d)["revoked_len"] // 20 for d in crls]
    total = sum(bounds)
    d, want = ops_match(rl, case, max_entries=total)
    assert not want[3].any() and int(want[4][0]["slots"]) == total and int(want[4][0]["entries"]) == 76
    d, want = ops_match(rl, case, max_entries=total - 1, shift=5)  # the last CRL no longer fits: the others keep their slots
    assert want[3].tolist() == [0, 0, 0, 0, cc.SPACE] and int(want[4][0]["slots"]) == total - bounds[4]
    assert not d["got"][1][total - bounds[4]:]["serial_len"].any()  # no slot of the refused CRL is written
    d, want = ops_match(rl, case, max_entries=0)
    assert want[3].tolist() == [cc.SPACE] * 5 and d["got"][4][0]["slots"] == 0 and d["got"][4][0]["refused"] == 5
    d, want = ops_match(rl, case, max_entries=bounds[0] + bounds[2] - 1, shift=2)  # the big list in the middle does not fit; nothing behind it does
    assert want[3].tolist() == [0, 0, cc.SPACE, cc.SPACE, cc.SPACE] and int(want[4][0]["entries"]) == 3


# ------------------------------------------------------------------------------------------------------------------ the lookup
def colliding_serials(crl, count, slots, home):
    """`count` serials of CRL `crl`, found on the CPU with the restated hash, that share the home slot `home` of a table of `slots`"""
    out, k = [], 0
    while len(out) < count:
        s = b"\x01" + k.to_bytes(3, "big")
        if cc.hash_serial(crl, s) & (slots - 1) == home:
            out.append(s)
        k += 1
    return out


def test_lookup_serial_forms_probing_and_every_answer(rl):
    ca = cc.CA_CN[44]
    cas = cc.ca_certs()
    # CRL 0: serials of every length 1 ... 20, negative ones among them, one twice, and pairs that differ in the last byte or in length
    every = [bytes([0x80 + n]) + bytes(range(1, n)) for n in range(1, 21)] + [bytes([n]) + bytes(range(1, n)) for n in range(1, 21)]
    pairs = [b"\x01", b"\x00\x81", b"\x00\x81\x00", b"\x42\x10", b"\x42\x11"]
    list0 = every + pairs + [pairs[3]]
    # CRL 1: the same serial bytes as some of CRL 0, and 65 serials of four bytes that share the last home slot but two of the table:
    # probing wraps.  (The table's size follows from the lists' lengths, which do not depend on the serials' values.)
    def both(collide):
        return [cc.join(cc.parts(44, ca, [cc.entry(s) for s in lst], xc._bytes(b"lksig", k, 2420)))
                for k, lst in enumerate((list0, [every[3], pairs[0]] + collide))]

    extra = [cc.random_crl(44, ca, b"lk", 2, 2, v2=False, ext=cc.crl_number()),      # CRL 2: refused (VERSION)
             cc.random_crl(65, cc.CA_CN[65], b"lk", 3, 2)]                          # CRL 3: another issuer's
    slots = cc.table_slots(sum(len(d) // 20 for d in both([b"\x01\x00\x00" + bytes([k]) for k in range(65)]) + extra))
    collide = colliding_serials(1, 65, slots, slots - 3)
    list1 = [every[3], pairs[0]] + collide
    crls = both(collide) + extra
    # the certificates: 3 CAs, then leaves under CA 0
    probe = [(every[0], 0), (every[19], 0), (every[39], 0), (pairs[0], 0), (pairs[1], 0), (pairs[2], 0), (pairs[4], 0), (pairs[3], 0),
             (b"\x42\x12", 0), (b"\x00\x82", 0), (every[3], 1), (pairs[0], 1), (pairs[1], 1), (collide[0], 1), (collide[64], 1), (collide[64], 0),
             (b"\x01\xff\xff\xff", 1)]
    leaves = [cc.cert_with_serial(44, 44, ca, b"leaf%d" % k, s, b"lkleaf", k, v3=k % 2 == 0) for k, (s, _) in enumerate(probe)]
    special = [cc.cert_with_serial(44, 44, ca, b"long", b"\x11" * 21, b"lkleaf", 50),     # a serial of 21 bytes
               cc.cert_with_serial(44, 44, ca, b"nonmin", b"\x00\x05", b"lkleaf", 51),    # not minimal
               xc.make_defect(cc.cert_with_serial(44, 44, ca, b"der", b"\x05", b"lkleaf", 52), "wrong_tag_validity")[0],  # its own row is DER
               cc.cert_with_serial(44, 44, ca, b"alg", b"\x05", b"lkleaf", 53)]
    n_l, n_s = len(leaves), len(special)
    case = cc.lay_out(cas + leaves + special, [0, 1, 2] + [0] * (n_l + n_s), [(d, len(d)) for d in crls], [0, 0, 0, 1], pad=[3, 0, 14, 7])
    blob, certs, items, cert_fields = case
    m = cc.max_entries_of(items)
    assert cc.table_slots(m) == slots
    d, want = ops_match(rl, case, max_entries=m, shift=3)
    assert want[3].tolist() == [0, 0, cc.VERSION, 0] and want[0]["count"].tolist() == [len(list0), len(list1), 0, 2]
    table, t = run_table(rl, d)
    assert t.size == slots and cc.table_is_sound(t, d["got"][1])
    homes = [cc.hash_serial(1, s) & (slots - 1) for s in collide]
    assert set(homes) == {slots - 3} and all(t[s] != 0 for s in (slots - 3, slots - 2, slots - 1, 0, 1, 2))  # the chain runs over the table's end
    cover = [cc.NONE] * 3 + [c for _, c in probe] + [0, 0, 0, 0]
    got = run_check(rl, d, table, certs, cert_fields, cover)
    want_rev = cc.expected_check(blob, certs, cert_fields, cover, items, want[0], want[3], None, want[1])
    assert np.array_equal(got, want_rev)
    R, G = cc.REVOKED, cc.GOOD
    assert want_rev.tolist() == [cc.NO_CRL] * 3 + [R, R, R, R, R, R, R, R, G, G, R, R, G, R, R, G, G] + [cc.CERT, cc.CERT, cc.CERT, G]
    # every answer in the order of its rules: one certificate (revoked under CRL 0, serial 42 10) under every condition in turn
    k = 3 + 7
    one = lambda **kw: run_check(rl, d, table, certs, cert_fields, kw.get("cover", cover), kw.get("ok"))  # noqa: E731
    for c, ok, answer in ((cc.NONE, None, cc.NO_CRL), (4, None, cc.CRL_INDEX), (2 ** 32 - 2, None, cc.CRL_INDEX), (2, None, cc.CRL_REFUSED),
                          (0, [0, 1, 1, 1], cc.CRL_REFUSED), (0, [1, 0, 0, 0], R), (3, None, cc.SCOPE), (3, [1, 1, 1, 0], cc.CRL_REFUSED), (1, None, G)):
        cv = list(cover)
        cv[k] = c
        got = one(cover=cv, ok=ok)
        assert got[k] == answer == cc.expected_check(blob, certs, cert_fields, cv, items, want[0], want[3], ok, want[1])[k], (c, ok)
    # NO_CRL and CRL_INDEX before CERT, CRL_REFUSED before CERT, CERT before SCOPE
    bad = 3 + n_l  # the 21-byte serial
    for c, answer in ((cc.NONE, cc.NO_CRL), (9, cc.CRL_INDEX), (2, cc.CRL_REFUSED), (3, cc.CERT), (0, cc.CERT)):
        cv = list(cover)
        cv[bad] = c
        assert one(cover=cv)[bad] == answer
    # a certificate row whose TBS range leaves the blob is CERT, and nothing is read for it
    tampered = cert_fields.copy()
    tampered[k]["tbs_off"] = blob.size - 3
    tampered[k + 1]["tbs_off"] = 2 ** 64 - 2
    got = run_check(rl, d, table, certs, tampered, cover)
    assert got[k] == got[k + 1] == cc.CERT and np.array_equal(np.delete(got, [k, k + 1]), np.delete(want_rev, [k, k + 1]))


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def pki(hp):
    """per parameter set: root -> intermediate -> 8 leaves with serials of their own, and two CRLs signed through sign_host -- the
    root's lists the intermediate, the intermediate's lists leaves 1, 4 and 6"""
    ders, issuers, crls, crl_issuers, cover, revoked = [], [], [], [], [], []
    for j, pset in enumerate(cc.SETS):
        ml = MlDsa(pset, hotpath=hp)
        pk, sk = ml.keygen_host(np.frombuffer(b"".join(xc._bytes(b"e2e-xi%d" % pset, i, 32) for i in range(10)), dtype=np.uint8))
        cns = [b"e2e root %d" % pset, b"e2e intermediate %d" % pset] + [b"e2e leaf %d-%d" % (pset, i) for i in range(8)]
        signer = [0, 0] + [1] * 8
        serials = [b"\x01", b"\x00\x90\x00" + bytes([j])] + [bytes([0x20 + i, j, 0xEE]) + bytes(i) for i in range(8)]
        body = [xc.tlv(0x30, xc.VERSION + xc.tlv(0x02, serials[i]) + xc.alg_id(pset) + xc.name(cns[signer[i]]) + xc.VALIDITY + xc.name(cns[i]) +
                       xc.tlv(0x30, xc.alg_id(pset) + xc.tlv(0x03, b"\x00" + pk[i].tobytes()))) for i in range(10)]
        lists = [(0, [serials[1]]), (1, [serials[2 + i] for i in (1, 4, 6)])]
        parts = [cc.parts(pset, cns[ca], [cc.entry(s, ext=cc.reason()) for s in lst], bytes(xc.SIG_LEN[pset])) for ca, lst in lists]
        msgs = body + [cc.tbs_of(p) for p in parts]
        keys = np.ascontiguousarray(sk[signer + [0, 1]])
        rnd = np.frombuffer(b"".join(xc._bytes(b"e2e-rnd%d" % pset, i, 32) for i in range(12)), dtype=np.uint8)
        sigs = ml.sign_host(keys, msgs, rnd)
        base, cbase = len(ders), len(crls)
        ders += [xc.cert(body[i], pset, sigs[i].tobytes()) for i in range(10)]
        issuers += [base + s for s in signer]
        for k, p in enumerate(parts):
            p["sig_bits"] = b"\x00" + sigs[10 + k].tobytes()
            crls.append(cc.join(p))
        crl_issuers += [base, base + 1]
        cover += [None, cbase] + [cbase + 1] * 8
        revoked += [cc.NO_CRL, cc.REVOKED] + [cc.REVOKED if i in (1, 4, 6) else cc.GOOD for i in range(8)]
    return dict(ders=ders, issuers=issuers, crls=crls, crl_issuers=crl_issuers, cover=cover, revoked=revoked)


def oracle_ok(blob, ops, status):
    raw = blob.tobytes()
    cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
    return np.array([st == 0 and bool(orc.verify_internal(int(op["set"]), orc.pk_try_from_bytes(int(op["set"]), cut(op["pk_off"], xc.PK_LEN[int(op["set"])])),
                                                          cut(op["msg_off"], op["msg_len"]), cut(op["sig_off"], xc.SIG_LEN[int(op["set"])]), ctx=b"",
                                                          mode=orc.MODE_PURE)) for op, st in zip(ops, status)], dtype=bool)


def test_python_front_against_the_restatement_and_the_oracle(rl, pki):
    rev, cert_ok, cert_status, crl_ok, crl_status = rl.check(pki["ders"], pki["issuers"], pki["crls"], pki["crl_issuers"], pki["cover"], pad=[0, 5, 11])
    assert rev.tolist() == pki["revoked"] and cert_ok.all() and crl_ok.all() and not cert_status.any() and not crl_status.any()
    # one CRL with a flipped signature byte, one with a flipped entry byte (a serial's length byte: the entry no longer reads)
    crls = list(pki["crls"])
    crls[1] = crls[1][:-9] + bytes([crls[1][-9] ^ 4]) + crls[1][-8:]
    w = cc.walk_crl(crls[3])
    at = cc.list_entries(crls[3], w)[1][1] + 3
    crls[3] = crls[3][:at] + bytes([crls[3][at] ^ 0x10]) + crls[3][at + 1:]
    rev, cert_ok, cert_status, crl_ok, crl_status = rl.check(pki["ders"], pki["issuers"], crls, pki["crl_issuers"], pki["cover"], pad=3)
    # the restatement and the oracle on the same layout
    blob, certs, items, cert_fields = cc.lay_out(pki["ders"], pki["issuers"], [(d, len(d)) for d in crls], pki["crl_issuers"], pad=3)
    blob = blob[:-1]
    f, e, ops, status, _ = cc.expected(blob, items, cert_fields, cc.max_entries_of(items))
    want_ok = oracle_ok(blob, ops, status)
    assert status.tolist() == [0, 0, 0, cc.ENTRY, 0, 0] and want_ok.tolist() == [True, False, True, False, True, True]
    assert np.array_equal(crl_status, status) and np.array_equal(crl_ok, want_ok) and cert_ok.all() and not cert_status.any()
    cover = [cc.NONE if c is None else c for c in pki["cover"]]
    want_rev = cc.expected_check(blob, certs, cert_fields, cover, items, f, status, want_ok, e)
    assert np.array_equal(rev, want_rev)
    assert rev.tolist()[:20] == ([cc.NO_CRL, cc.REVOKED] + [cc.CRL_REFUSED] * 8) * 2 and rev.tolist()[20:] == pki["revoked"][20:]
    assert rl.check([], [], [], [], [])[0].size == 0


def test_one_table_serves_two_batches_of_certificates(rl, pki):
    """table_device once, check_device twice: the second batch is the same certificates' rows in another order"""
    blob, certs, items, cert_fields = cc.lay_out(pki["ders"], pki["issuers"], [(d, len(d)) for d in pki["crls"]], pki["crl_issuers"], pad=7)
    d, want = ops_match(rl, (blob, certs, items, cert_fields), shift=2)
    assert not want[3].any()
    table, t = run_table(rl, d)
    assert cc.table_is_sound(t, d["got"][1])
    cover = [cc.NONE if c is None else c for c in pki["cover"]]
    first = run_check(rl, d, table, certs, cert_fields, cover)
    assert first.tolist() == pki["revoked"]
    # the second batch: the rows in reverse order.  `issuer` means the same rows for certificates and CRLs, so the numbers stay.
    n = len(certs)
    perm = list(range(n))[::-1]
    certs2, fields2 = certs[perm].copy(), cert_fields[perm].copy()
    cover2 = [cover[i] for i in perm]
    second = run_check(rl, d, table, certs2, fields2, cover2)
    assert second.tolist() == [pki["revoked"][i] for i in perm]
    assert np.array_equal(host(table).view(np.uint32), t)  # the lookups leave the table as it was
