"""The path-validation library on the device (include/mldsa_path.h): mldsa_path_times, mldsa_path_parse, mldsa_path_crl_times and
mldsa_path_chain byte for byte against the restatement of tests/path_cases.py -- a century of days, every defect class, a sweep of
single-byte changes, the freshness of CRLs in front of mldsa_crl_check, the climb on synthetic rows with every rule at every place --
and whole signed chains with a CRL through the Python front against the restatement run on the oracle's verdicts."""
import calendar
import datetime

from gpu_common import *  # noqa: F401,F403

import crl_cases as cc
import path_cases as pc
import x509_cases as xc
from fips204_amd import _crl_lib, _lib, _path_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsaPathValidator

pytestmark = pytest.mark.gpu

CANARY = 0x77
ROWS = 3  # canary rows behind each output array


@pytest.fixture(scope="module")
def pv(hp):
    return MlDsaPathValidator(hotpath=hp)


def guarded(nbytes, extra):
    return torch.full((nbytes + extra,), CANARY, dtype=torch.uint8, device="cuda")


def blob_dev(blob, shift=0):
    """the blob on the device between canary bytes, `shift` bytes into its allocation"""
    t = torch.full((blob.size + shift + 1,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + blob.size] = torch.from_numpy(blob.copy())
    return t, t[shift:shift + blob.size]


def rows_dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(8, np.uint8)).cuda()


def differ(got, want, what):
    if not np.array_equal(got, want):
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], got[bad[0]], want[bad[0]]))


# ------------------------------------------------------------------------------------------------------------------ times
def run_times(pv, blob, offs, shift=0):
    n = len(offs)
    whole, b = blob_dev(blob, shift)
    seconds, status, d_offs = guarded(n * 8, ROWS * 8), guarded(n, ROWS), dev_off(offs)
    _path_lib.check(pv.lib.mldsa_path_times(pv.hp._h, _ptr(b), b.numel(), _ptr(d_offs), n, _ptr(seconds), _ptr(status), _stream(pv.device)))
    s, st, w = host(seconds), host(status), host(whole)
    assert (s[n * 8:] == CANARY).all() and (st[n:] == CANARY).all() and (w[:shift] == CANARY).all() and w[-1] == CANARY
    assert np.array_equal(w[shift:shift + blob.size], blob)
    return s[:n * 8].view(np.int64), st[:n]


def test_every_day_of_a_century_in_one_launch(pv):
    tlvs, want = [], []
    day, end = datetime.date(1950, 1, 1), datetime.date(2049, 12, 31)
    while day <= end:
        for clock in ((0, 0, 0), (23, 59, 59)):
            tlvs.append(pc.utc(day.year, day.month, day.day, *clock))
            want.append(calendar.timegm((day.year, day.month, day.day) + clock))
        day += datetime.timedelta(days=1)
    assert len(tlvs) == 2 * 36525
    blob = np.frombuffer(b"".join(tlvs), dtype=np.uint8)
    offs = np.arange(len(tlvs), dtype=np.uint64) * 15
    seconds, status = run_times(pv, blob, offs, shift=3)
    assert not status.any()
    differ(seconds, np.array(want, dtype=np.int64), "seconds")


def test_generalized_month_ends_and_every_refusal(pv):
    good = []
    for y in (1, 1600, 1900, 1970, 2000, 2038, 2100, 2400, 9999):
        leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
        for mo in range(1, 13):
            last = 29 if mo == 2 and leap else pc.MONTH_DAYS[mo - 1]
            good += [(pc.generalized(y, mo, last, 23, 59, 59), calendar.timegm((y, mo, last, 23, 59, 59))), (pc.generalized(y, mo, last + 1), None)]
    bad = [pc.generalized(1900, 2, 29), pc.generalized(2100, 2, 29), pc.utc(2025, 2, 29), pc.utc(2025, 1, 1, 0, 0, 60), pc.utc(2025, 1, 1, 24),
           pc.utc(2025, 1, 1, 0, 60), pc.utc(2025, 0, 1), pc.utc(2025, 13, 1), pc.utc(2025, 1, 0), pc.utc(2025, 4, 31), pc.generalized(0),
           xc.tlv(0x17, b"25010100000Z"), xc.tlv(0x17, b"2501010000000Z"), xc.tlv(0x18, b"2025010100000Z"), xc.tlv(0x18, b"20250101000000.Z"),
           xc.tlv(0x17, b"250101000000z"), xc.tlv(0x18, b"20250101000000z"), xc.tlv(0x16, b"250101000000Z"), xc.tlv(0x17, b"25010100000/Z"),
           xc.tlv(0x17, b"2501:1000000Z"), b"\x17\x81\x0d250101000000Z", b"\x17\x80250101000000Z", xc.tlv(0x17, b""), xc.tlv(0x18, b"Z"),
           xc.tlv(0x17, b"250101000000+"), xc.tlv(0x18, b"20250101000000\x00")]
    tlvs = [t for t, _ in good] + bad + [pc.utc(2049, 12, 31, 23, 59, 59)]
    data = b"".join(tlvs)
    offs = np.cumsum([0] + [len(t) for t in tlvs[:-1]]).astype(np.uint64)
    # the last Time ends one byte behind the blob; offsets at, one before and far behind the blob's end are no Time at all
    blob = np.frombuffer(data[:-1], dtype=np.uint8)
    offs = np.concatenate([offs, np.array([blob.size - 1, blob.size, blob.size + 1, 2 ** 63, 2 ** 64 - 1, blob.size - 2], dtype=np.uint64)])
    want_s, want_st = pc.expected_times(blob, offs)
    n_good = len(good)
    assert want_st[:n_good].tolist() == [0, pc.TIME] * (n_good // 2) and [int(x) for x in want_s[:n_good:2]] == [s for _, s in good[::2]]
    assert (want_st[n_good:n_good + len(bad) + 1] == pc.TIME).all() and want_st[-6:].tolist() == [pc.RANGE] * 5 + [pc.TIME]
    for shift in (0, 5):
        seconds, status = run_times(pv, blob, offs, shift)
        differ(status, want_st, "status")
        differ(seconds, want_s, "seconds")


# ------------------------------------------------------------------------------------------------------------------ parse
def run_parse(pv, blob, certs, flags=0, shift=0):
    n = len(certs)
    whole, b = blob_dev(blob, shift)
    fields, d_certs = guarded(n * 48, ROWS * 48), pv.certificates.certs_tensor(certs)
    _path_lib.check(pv.lib.mldsa_path_parse(pv.hp._h, _ptr(b), b.numel(), _ptr(d_certs), n, flags, _ptr(fields), _stream(pv.device)))
    f, w = host(fields), host(whole)
    assert (f[n * 48:] == CANARY).all() and (w[:shift] == CANARY).all() and w[-1] == CANARY and np.array_equal(w[shift:shift + blob.size], blob)
    return f[:n * 48].view(_path_lib.FIELDS_DTYPE)


@pytest.mark.parametrize("n", pc.SEAM_SIZES)
def test_parse_matches_the_restatement_byte_for_byte(pv, n):
    shift = (0, 1, 3, 15, 8)[pc.SEAM_SIZES.index(n)]
    blob, certs = pc.seam_case(n, seed=n % 7)
    if n >= 65:  # the gaps cycle through 0 ... 15: with certificates of three lengths every alignment of a start occurs
        assert {int(c["off"] + shift) % 16 for c in certs} == set(range(16))
    want = pc.expected_parse(blob, certs)
    assert (want["status"][2::3] == 0).all() and (n < 63 or len(set(want["status"].tolist())) >= 5)
    differ(run_parse(pv, blob, certs, shift=shift), want, "fields")
    differ(run_parse(pv, blob, certs, pc.ALLOW_UNKNOWN_CRITICAL, shift), pc.expected_parse(blob, certs, pc.ALLOW_UNKNOWN_CRITICAL), "fields")
    # the device wrapper gives the same rows
    whole, b = blob_dev(blob, shift)
    got = host(pv.parse_device(b, pv.certificates.certs_tensor(certs), n)).view(_path_lib.FIELDS_DTYPE)
    differ(got, want, "fields")


def test_every_case_of_the_header_on_every_set(pv):
    names = list(pc.CASES)
    ders = [pc.case(name, pset, k) for k, pset in enumerate(pc.SETS) for name in names]
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [0] * len(ders), pad=[7, 0, 2, 13, 5])
    want = pc.expected_parse(blob, certs)
    assert want["status"].tolist() == [pc.CASES[name][0] for name in names] * 3
    got = run_parse(pv, blob, certs, shift=1)
    differ(got, want, "fields")
    by_name = {name: got[i] for i, name in enumerate(names)}
    assert (by_name["ok_32_extensions"]["n_ext"], by_name["ext_33_extensions"]["n_ext"], by_name["ok_v3_plain"]["n_ext"]) == (32, 32, 0)
    assert by_name["ok_ku_9_bits"]["key_usage"] == 0x160 and by_name["ok_path_len_max"]["path_len"] == 2 ** 31 - 1 and by_name["ok_path_len_128"]["path_len"] == 128
    assert by_name["der_tail_trailing"].tobytes() == bytes(44) + bytes([pc.DER]) + bytes(3)
    # unknown critical extensions with the flag: accepted, the first one still recorded
    allowed = run_parse(pv, blob, certs, pc.ALLOW_UNKNOWN_CRITICAL, shift=1)
    differ(allowed, pc.expected_parse(blob, certs, pc.ALLOW_UNKNOWN_CRITICAL), "fields")
    i = names.index("critical_unknown")
    assert got[i]["status"] == pc.CRITICAL and allowed[i]["status"] == 0 and got[i]["crit_off"] == allowed[i]["crit_off"] != 0
    assert (allowed["status"] != got["status"]).sum() == 6  # the two critical cases of each set, nothing else


def test_range_rule_and_the_ends_of_the_blob(pv):
    der = pc.case("ok_ca")
    blob, certs = xc.lay_out([(der, len(der))] * 6, [0] * 6, pad=[4, 0])
    certs[1]["len"] = 1
    certs[2]["len"] = len(der) + 1          # one byte more than the certificate has: DER, inside the blob
    certs[3]["off"] = 2 ** 64 - 1
    certs[4]["len"] = 2 ** 32 - 1
    certs[5]["len"] = len(der) + 2          # the last certificate and the spare byte and one more: behind the blob's end
    want = pc.expected_parse(blob, certs)
    assert want["status"].tolist() == [0, pc.RANGE, pc.DER, pc.RANGE, pc.RANGE, pc.RANGE]
    differ(run_parse(pv, blob, certs, shift=2), want, "fields")
    # a certificate that ends with the blob
    differ(run_parse(pv, blob[:-1], certs[:1], shift=0), want[:1], "fields")


def test_single_byte_mutation_sweep_over_validity_and_extensions(pv):
    der = pc.case("ok_v3_uid_and_ca", 44)
    positions = pc.spans(der)
    assert len(positions) >= 32 + len(pc.CA_TAIL)
    blob, certs = pc.mutation_batch(der, positions)
    want = pc.expected_parse(blob, certs)
    seen = set(want["status"].tolist())
    assert seen == {pc.OK, pc.DER, pc.TIME, pc.EXT, pc.CRITICAL}  # (a changed OID of a critical extension is an unknown critical one)
    assert 0 < (want["status"] == 0).sum() < len(certs) // 2
    differ(run_parse(pv, blob, certs, shift=5), want, "fields")


# ------------------------------------------------------------------------------------------------------------------ CRL times
T0, T1 = calendar.timegm((2025, 6, 1, 12, 0, 0)), calendar.timegm((2025, 7, 1, 12, 0, 0))


def crl_batch():
    """(blob, certs, items, cert_fields, cover): six CRLs under the ML-DSA-44 CA -- 0 with both times, 1 without nextUpdate, 2 refused by
    its walk, 3 with a thisUpdate and 4 with a nextUpdate that is no Time, 5 as 0 under a CA of another set (refused by the link) --
    and four leaves, two of them listed by CRL 0 and CRL 1"""
    cas = cc.ca_certs()
    this, after = pc.utc(2025, 6, 1, 12), pc.generalized(2025, 7, 1, 12)
    serials = [cc.serial_of(b"fresh", 0, k) for k in range(2)]
    crls = []
    for k, (t, nx) in enumerate(((this, after), (this, b""), (this, after), (pc.utc(2025, 6, 31, 12), after), (this, pc.generalized(2025, 7, 1, 24)),
                                 (this, after))):
        p = cc.random_parts(44, cc.CA_CN[44], b"fresh", k, 0)
        p.update(entries=[cc.entry(s) for s in serials], this=t, next=nx)
        crls.append(cc.make_defect(p, "version_v1") if k == 2 else (cc.join(p), len(cc.join(p))))
    leaves = [cc.cert_with_serial(44, 44, cc.CA_CN[44], b"leaf%d" % k, serials[k] if k < 2 else b"\x55" + bytes([k]), b"fresh-leaf", k) for k in range(4)]
    blob, certs, items, cert_fields = cc.lay_out(cas + leaves, [0, 1, 2] + [0] * 4, crls, [0, 0, 0, 0, 0, 1], pad=[5, 0, 9])
    return blob, certs, items, cert_fields, np.array([cc.NONE] * 3 + [0, 1, 0, 1], dtype=np.uint32)


def run_crl_times(pv, b, fields, status, crl_ok, now, flags=0):
    n = status.numel()
    this_s, next_s = guarded(n * 8, ROWS * 8), guarded(n * 8, ROWS * 8)
    time_status, fresh = guarded(n, ROWS), guarded(n, ROWS)
    _path_lib.check(pv.lib.mldsa_path_crl_times(pv.hp._h, _ptr(b), b.numel(), _ptr(fields), _ptr(status), None if crl_ok is None else _ptr(crl_ok), n,
                                                now, flags, _ptr(this_s), _ptr(next_s), _ptr(time_status), _ptr(fresh), _stream(pv.device)))
    out = [host(t) for t in (this_s, next_s, time_status, fresh)]
    for t, size in zip(out, (n * 8, n * 8, n, n)):
        assert (t[size:] == CANARY).all()
    return out[0][:n * 8].view(np.int64), out[1][:n * 8].view(np.int64), out[2][:n], out[3][:n], fresh[:n]


def test_crl_freshness_in_front_of_the_lookup(pv):
    blob, certs, items, cert_fields, cover = crl_batch()
    whole, b = blob_dev(blob, 3)
    rl, n = pv.lists, len(items)
    d_items, d_cert_fields = rl.items_tensor(items)[:n * 16], rows_dev(cert_fields)
    ops, status, fields, entries, totals = rl.ops_device(b, d_items, d_cert_fields, n, cc.max_entries_of(items))
    table, totals = rl.table_device(entries, totals)
    f, st = host(fields).view(_crl_lib.FIELDS_DTYPE), host(status)
    want_f, _, _, want_st, _ = cc.expected(blob, items, cert_fields, cc.max_entries_of(items))
    assert np.array_equal(f, want_f) and st.tolist() == want_st.tolist() == [0, 0, cc.VERSION, 0, 0, cc.ISSUER]
    crl_ok = np.array([1, 1, 1, 1, 1, 1], dtype=np.uint8)
    for flags in (0, pc.REQUIRE_NEXT_UPDATE):
        for now, first in ((T0 - 1, pc.CRL_NOT_YET), (T0, pc.CRL_FRESH), (T1, pc.CRL_FRESH), (T1 + 1, pc.CRL_STALE)):
            got = run_crl_times(pv, b, fields, status, dev(crl_ok), now, flags)
            want = pc.expected_crl_times(blob, f, st, crl_ok, now, flags)
            for g, w, what in zip(got, want, ("this_s", "next_s", "time_status", "fresh_ok")):
                differ(g, w, what)
            no_next = pc.CRL_NOT_YET if now < T0 else pc.CRL_STALE if flags else pc.CRL_FRESH
            assert got[2].tolist() == [first, no_next, pc.CRL_REFUSED, pc.CRL_TIME, pc.CRL_TIME, pc.CRL_REFUSED]
            assert got[0].tolist() == [T0, T0, 0, 0, T0, 0] and got[1].tolist() == [T1, 0, 0, T1, 0, 0]
            # the lookup behind it: a CRL that is not fresh answers for nobody
            rev = host(rl.check_device(b, pv.certificates.certs_tensor(certs), d_cert_fields, kidx_dev(cover), d_items, fields, status, got[4], entries,
                                       table))
            under = lambda c, listed: (cc.REVOKED if listed else cc.GOOD) if got[3][c] else cc.CRL_REFUSED  # noqa: E731
            assert rev.tolist() == [cc.NO_CRL] * 3 + [under(0, True), under(1, True), under(0, False), under(1, False)]
    # the signature verdicts: NULL counts as all good, a zero refuses its CRL's freshness alone
    got = run_crl_times(pv, b, fields, status, None, T0)
    assert got[3].tolist() == [1, 1, 0, 0, 0, 0]
    got = run_crl_times(pv, b, fields, status, dev(np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)), T0)
    assert got[3].tolist() == [0, 1, 0, 0, 0, 0] and got[2].tolist()[:2] == [pc.CRL_FRESH, pc.CRL_FRESH]
    # rows whose offsets point outside the blob are not followed
    rows = f.copy()
    rows[0]["this_off"], rows[1]["this_off"], rows[1]["next_off"] = blob.size - 1, 2 ** 64 - 1, 0
    rows[4]["next_off"] = blob.size  # (its nextUpdate is no Time anyway)
    rows[3]["this_off"], rows[3]["next_off"] = f[0]["this_off"], 2 ** 63
    got = run_crl_times(pv, b, rows_dev(rows), status, None, T0)
    want = pc.expected_crl_times(blob, rows, st, None, T0)
    for g, w, what in zip(got, want, ("this_s", "next_s", "time_status", "fresh_ok")):
        differ(g, w, what)
    assert got[2].tolist() == [pc.CRL_TIME, pc.CRL_TIME, pc.CRL_REFUSED, pc.CRL_TIME, pc.CRL_TIME, pc.CRL_REFUSED] and not got[3].any()
    assert got[0].tolist() == [0, 0, 0, T0, T0, 0]
    assert host(whole)[-1] == CANARY and (host(whole)[:3] == CANARY).all()
    # the Python front gives the same four arrays
    this_s, next_s, time_status, fresh = pv.crl_times_device(b, fields, status, None, T1 + 1, require_next_update=True)
    assert host(time_status).tolist() == [pc.CRL_STALE, pc.CRL_STALE, pc.CRL_REFUSED, pc.CRL_TIME, pc.CRL_TIME, pc.CRL_REFUSED] and not host(fresh).any()


# ------------------------------------------------------------------------------------------------------------------ the chain
NOW = 1500


def run_chain(pv, issuers, policy, cert_status, cert_ok, revocation, anchor, now=NOW, flags=0):
    """mldsa_path_chain into guarded buffers: (results, nodes) as numpy arrays"""
    n = len(issuers)
    certs = np.zeros(n, dtype=_path_lib_cert_dtype())
    certs["issuer"] = issuers
    size = pv.lib.mldsa_path_scratch_bytes(n)
    results, scratch = guarded(n * 8, ROWS * 8), guarded(size, 256)
    d = [rows_dev(certs), rows_dev(policy), dev(cert_status), dev(cert_ok), None if revocation is None else dev(revocation), dev(anchor)]  # kept alive
    _path_lib.check(pv.lib.mldsa_path_chain(pv.hp._h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), None if d[4] is None else _ptr(d[4]), _ptr(d[5]),
                                            n, now, flags, _ptr(results), _ptr(scratch), size, _stream(pv.device)))
    r, s = host(results), host(scratch)
    assert (r[n * 8:] == CANARY).all() and (s[size:] == CANARY).all() and (s[n * 8:size] == CANARY).all()
    return r[:n * 8].view(_path_lib.RESULT_DTYPE), s[:n * 8].view(_path_lib.NODE_DTYPE)


def _path_lib_cert_dtype():
    from fips204_amd import _x509_lib
    return _x509_lib.CERT_DTYPE


class Forest:
    """chains laid side by side in one batch: every array of mldsa_path_chain, and where each chain begins"""

    def __init__(self):
        self.issuers, self.policy, self.status, self.ok, self.rev, self.anchor, self.starts = [], [], [], [], [], [], []

    def add(self, issuers, anchor, policy=None, status=None, ok=None, rev=None, absolute=False):
        base, n = len(self.issuers), len(issuers)
        self.starts.append(base)
        self.issuers += [int(x) if absolute or int(x) == pc.NO_ISSUER else base + int(x) for x in issuers]
        self.policy += list(pc.policy_rows(n) if policy is None else policy)
        self.status += list(np.zeros(n, np.uint8) if status is None else status)
        self.ok += list(np.ones(n, np.uint8) if ok is None else ok)
        self.rev += list(np.zeros(n, np.uint8) if rev is None else rev)
        self.anchor += list(anchor)
        return base

    def arrays(self):
        return (np.array(self.issuers, dtype=np.uint32), np.array(self.policy, dtype=_path_lib.FIELDS_DTYPE), np.array(self.status, dtype=np.uint8),
                np.array(self.ok, dtype=np.uint8), np.array(self.rev, dtype=np.uint8), np.array(self.anchor, dtype=np.uint8))


def check_chain(pv, arrays, with_revocation=True, now=NOW, flags=0):
    issuers, policy, status, ok, rev, anchor = arrays
    rev = rev if with_revocation else None
    got, nodes = run_chain(pv, issuers, policy, status, ok, rev, anchor, now, flags)
    differ(nodes, pc.nodes_of(issuers, policy, status, ok, rev, anchor, now, flags), "nodes")
    differ(got, pc.expected_chain(issuers, policy, status, ok, rev, anchor, now, flags), "results")
    return got


def test_depths_loops_cycles_and_issuers_out_of_range(pv):
    f = Forest()
    at = {}
    for depth in (0, 1, 2, 16, 17):
        at[depth] = f.add(*pc.line(depth))
    at["loop"] = f.add([0], [0])                         # its own issuer and no anchor
    at["cycle2"] = f.add([1, 0], [0, 0])
    at["cycle3"] = f.add([1, 2, 0], [0, 0, 0])
    at["none"] = f.add([pc.NO_ISSUER, 0], [0, 0])        # a root that was parsed only, and its child
    at["far"] = f.add([0, 0], [0, 0])
    arrays = f.arrays()
    n = len(arrays[0])
    arrays[0][at["far"]] = n                             # the first index that is no certificate
    arrays[0][at["far"] + 1] = at["far"]
    got = check_chain(pv, arrays)
    verdict = lambda i: (int(got[i]["verdict"]), int(got[i]["where"]), int(got[i]["depth"]))  # noqa: E731
    for depth in (0, 1, 2, 16):
        assert verdict(at[depth] + depth) == (pc.TRUSTED, at[depth], depth)
    assert verdict(at[17] + 17) == (pc.DEPTH, at[17] + 1, 16) and verdict(at[17] + 16) == (pc.TRUSTED, at[17], 16)
    assert verdict(at["loop"]) == (pc.NO_ANCHOR, at["loop"], 0)
    assert verdict(at["cycle2"]) == (pc.DEPTH, at["cycle2"], 16) and verdict(at["cycle3"]) == (pc.DEPTH, at["cycle3"] + 1, 16)
    assert verdict(at["none"] + 1) == (pc.NO_ANCHOR, at["none"], 1) and verdict(at["far"] + 1) == (pc.NO_ANCHOR, at["far"], 1)


def test_every_rule_at_every_place(pv):
    """a line of depth 3 below an anchor; each own rule and each issuer rule broken at the leaf's k = 0, 1 and 2: what the leaf gets"""
    f = Forest()
    want = []

    def broken(k, what):
        issuers, anchor = pc.line(3)
        policy, status, ok, rev = pc.policy_rows(4), np.zeros(4, np.uint8), np.ones(4, np.uint8), np.zeros(4, np.uint8)
        i = 3 - k  # the certificate k steps above the leaf
        if what == pc.CERT:
            status[i] = 5
        elif what == pc.SIG:
            ok[i] = 0
        elif what == pc.POLICY:
            policy[i]["status"] = pc.EXT
        elif what == pc.NOT_YET:
            policy[i]["not_before"] = NOW + 1
        elif what == pc.EXPIRED:
            policy[i]["not_after"] = NOW - 1
        elif what == pc.REVOKED:
            rev[i] = cc.REVOKED
        elif what == pc.REVOCATION:
            rev[i] = cc.CRL_REFUSED
        elif what == pc.NOT_CA:
            policy[i]["flags"] = pc.V3 | pc.HAS_BC | pc.HAS_KU
        elif what == pc.KEY_USAGE:
            policy[i]["key_usage"] = 0x40  # cRLSign alone
        base = f.add(issuers, anchor, policy, status, ok, rev)
        as_issuer = what in (pc.NOT_CA, pc.KEY_USAGE)
        want.append((base + 3, (pc.TRUSTED, base, 3) if as_issuer and k == 0 else (what, base + i, k)))

    for k in (0, 1, 2):
        for what in range(pc.CERT, pc.KEY_USAGE + 1):
            broken(k, what)
    # the order of the rules: everything broken at once on one certificate, mended rule by rule
    for upto in range(pc.CERT, pc.KEY_USAGE + 1):
        issuers, anchor = pc.line(3)
        policy, status, ok, rev = pc.policy_rows(4), np.zeros(4, np.uint8), np.ones(4, np.uint8), np.zeros(4, np.uint8)
        status[2], ok[2], rev[2] = (upto <= pc.CERT) * 5, upto > pc.SIG, cc.REVOKED if upto <= pc.REVOKED else cc.SCOPE if upto <= pc.REVOCATION else 0
        policy[2]["status"] = pc.TIME if upto <= pc.POLICY else 0
        policy[2]["not_before"], policy[2]["not_after"] = (NOW + 1, NOW - 1) if upto <= pc.NOT_YET else (0, NOW - 1) if upto <= pc.EXPIRED else (0, NOW)
        policy[2]["flags"] = pc.V3 | pc.HAS_KU | pc.HAS_BC | (pc.IS_CA if upto > pc.NOT_CA else 0)
        policy[2]["key_usage"] = 1
        base = f.add(issuers, anchor, policy, status, ok, rev)
        want.append((base + 3, (upto, base + 2, 1)))
    # other flag bits do not make a CA: not v3, no basicConstraints
    for flags in (pc.HAS_BC | pc.IS_CA, pc.V3 | pc.IS_CA, pc.V3 | pc.HAS_BC, 0):
        policy = pc.policy_rows(2)
        policy[0]["flags"] = flags
        base = f.add([pc.NO_ISSUER, 0], [0, 0], policy)
        want.append((base + 1, (pc.NOT_CA, base, 1)))
    got = check_chain(pv, f.arrays())
    for i, w in want:
        assert (int(got[i]["verdict"]), int(got[i]["where"]), int(got[i]["depth"])) == w, (i, w)


def test_path_len_anchors_in_mid_chain_and_the_revocation_forms(pv):
    f = Forest()
    # pathLen 1 on certificate 1 of a line of depth 4: the certificate two steps below it is the last that passes
    issuers, anchor = pc.line(4)
    policy = pc.policy_rows(5)
    policy[1]["path_len"] = 1
    a = f.add(issuers, anchor, policy)
    # pathLen 0 on the anchor lends nothing; 300 and 2^31 - 1 saturate and never bite within the depth
    policy = pc.policy_rows(5)
    policy[0]["path_len"], policy[1]["path_len"], policy[2]["path_len"] = 0, 300, 2 ** 31 - 1
    b = f.add(issuers, anchor, policy)
    # an anchor in mid-chain: certificate 1 is expired and no CA, certificate 2 is an anchor; the leaf never sees certificate 1
    policy = pc.policy_rows(5)
    policy[1]["not_after"], policy[1]["flags"] = NOW - 1, pc.V3
    c = f.add(issuers, [1, 0, 1, 0, 0], policy)
    # revocation: every value a certificate can carry, on a leaf under an anchor
    revs = list(range(9))
    d = f.add([0] + [0] * len(revs), [1] + [0] * len(revs), rev=[0] + revs)
    arrays = f.arrays()
    got = check_chain(pv, arrays)
    v = lambda i: (int(got[i]["verdict"]), int(got[i]["where"]), int(got[i]["depth"]))  # noqa: E731
    assert [v(a + i)[0] for i in range(5)] == [0, 0, 0, 0, pc.PATH_LEN] and v(a + 4) == (pc.PATH_LEN, a + 1, 3) and v(a + 3) == (0, a, 3)
    assert [v(b + i)[0] for i in range(5)] == [0] * 5
    assert v(c + 4) == (pc.TRUSTED, c + 2, 2) and v(c + 1) == (pc.EXPIRED, c + 1, 0) and v(c + 2) == (pc.TRUSTED, c + 2, 0)
    assert [v(d + 1 + r)[0] for r in revs] == [0, pc.REVOKED] + [pc.REVOCATION] * 7
    # ALLOW_NO_CRL lets NO_CRL pass and nothing else; with revocation NULL no value is looked at
    got = check_chain(pv, arrays, flags=pc.ALLOW_NO_CRL)
    assert [int(got[d + 1 + r]["verdict"]) for r in revs] == [0, pc.REVOKED, 0] + [pc.REVOCATION] * 6
    got = check_chain(pv, arrays, with_revocation=False)
    assert [int(got[d + 1 + r]["verdict"]) for r in revs] == [0] * 9
    # the validity's ends are inside it
    for now, verdict in ((999, pc.NOT_YET), (1000, 0), (2000, 0), (2001, pc.EXPIRED), (-2 ** 63, pc.NOT_YET), (2 ** 63 - 1, pc.EXPIRED)):
        got = check_chain(pv, arrays, now=now)
        assert int(got[d + 1]["verdict"]) == verdict and int(got[d]["verdict"]) == 0, now


@pytest.mark.parametrize("n", (1, 64, 65, 257))
def test_chain_batch_sizes_and_the_scratch_check(pv, n):
    """n certificates as chains of depth 3 dealt round robin, every seventh certificate breaking a rule of its own"""
    roots = max(n // 4, 1)  # certificates [0, roots) are anchors, [roots, 2 roots) intermediates, the rest leaves
    issuers = np.array([i if i < roots else i - roots if i < 2 * roots else roots + i % roots for i in range(n)], dtype=np.uint32)
    assert n == 1 or int(issuers.max()) < min(2 * roots, n)
    policy = pc.policy_rows(n)
    anchor = np.array([1 if i < roots else 0 for i in range(n)], dtype=np.uint8)
    status, ok, rev = np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        if i % 7 == 3:
            ok[i] = 0
        if i % 11 == 5:
            policy[i]["not_after"] = NOW - 1
        if i % 13 == 6:
            rev[i] = cc.REVOKED
    got = check_chain(pv, (issuers, policy, status, ok, rev, anchor))
    assert got[0]["verdict"] == pc.TRUSTED and (n < 64 or len(set(got["verdict"].tolist())) >= 4)
    # a scratch one byte short is refused before anything is launched
    size = pv.lib.mldsa_path_scratch_bytes(n)
    results, scratch = guarded(n * 8, 8), guarded(size, 0)
    d = [rows_dev(np.zeros(n, dtype=_path_lib_cert_dtype())), rows_dev(policy), dev(status), dev(ok), dev(anchor)]  # kept alive
    rc = pv.lib.mldsa_path_chain(pv.hp._h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), None, _ptr(d[4]), n, NOW, 0, _ptr(results), _ptr(scratch),
                                 size - 1, _stream(pv.device))
    assert rc == _lib.ERR_PARAM and b"smaller than mldsa_path_scratch_bytes" in pv.lib.mldsa_path_last_error()
    assert (host(results) == CANARY).all() and (host(scratch) == CANARY).all()
    # the Python front gives the same rows
    certs_h = np.zeros(n, dtype=_path_lib_cert_dtype())
    certs_h["issuer"] = issuers
    front = pv.chain_device(rows_dev(certs_h), rows_dev(policy), dev(status), dev(ok), dev(rev), dev(anchor), NOW)
    differ(host(front).view(_path_lib.RESULT_DTYPE), got, "results")


# ------------------------------------------------------------------------------------------------------------------ end to end
YEAR = lambda y: calendar.timegm((y, 1, 1, 0, 0, 0))  # noqa: E731


@pytest.fixture(scope="module")
def pki():
    """Twelve ML-DSA-44 certificates signed by the oracle: two chains of root (valid to 2040), intermediate (to 2030) and four leaves (to
    2035) -- the last leaf of chain 1 issued by another leaf, which is no CA --, and two CRLs of root 0 that cover intermediate 0: one
    lists another serial, one lists its serial.  Both CRLs run from 2025-06-01 to 2025-07-01."""
    n = 12
    keys = [orc.keygen_from_seed(44, xc._bytes(b"path-e2e-xi", i, 32)) for i in range(n)]
    signer = [0, 0, 1, 1, 1, 1, 6, 6, 7, 7, 7, 10]
    cns = [b"path e2e %d" % i for i in range(n)]
    tail = lambda i: pc.CA_TAIL if i % 6 < 2 else pc.extensions([pc.basic(ca=False, critical=None), pc.key_usage(b"\x07\x80")])  # noqa: E731
    until = lambda i: 2040 if i % 6 == 0 else 2030 if i % 6 == 1 else 2035  # noqa: E731
    ders = []
    for i in range(n):
        body = xc.tlv(0x30, xc.VERSION + xc.tlv(0x02, bytes([0x10 + i])) + xc.alg_id(44) + xc.name(cns[signer[i]]) +
                      pc.validity(pc.utc(2025), pc.utc(until(i))) + xc.name(cns[i]) +
                      xc.tlv(0x30, xc.alg_id(44) + xc.tlv(0x03, b"\x00" + orc.pk_into_bytes(44, keys[i][0]))) + tail(i))
        sig = orc.sign_internal(44, keys[signer[i]][1], body, xc._bytes(b"path-e2e-rnd", i, 32), ctx=b"", mode=orc.MODE_PURE)
        ders.append(xc.cert(body, 44, sig))
    crls = []
    for k, serial in enumerate((b"\x7f", bytes([0x11]))):
        p = cc.parts(44, cns[0], [cc.entry(serial)], bytes(xc.SIG_LEN[44]))
        p.update(this=pc.utc(2025, 6, 1), next=pc.utc(2025, 7, 1))
        p["sig_bits"] = b"\x00" + orc.sign_internal(44, keys[0][1], cc.tbs_of(p), xc._bytes(b"path-e2e-crl", k, 32), ctx=b"", mode=orc.MODE_PURE)
        crls.append(cc.join(p))
    return dict(ders=ders, issuers=signer, anchors=[0, 6], crls=crls, cover=[None, 0] + [None] * 10)


def oracle_ok(blob, ops, status):
    raw = blob.tobytes()
    cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
    return np.array([st == 0 and bool(orc.verify_internal(44, orc.pk_try_from_bytes(44, cut(op["pk_off"], xc.PK_LEN[44])), cut(op["msg_off"], op["msg_len"]),
                                                          cut(op["sig_off"], xc.SIG_LEN[44]), ctx=b"", mode=orc.MODE_PURE))
                     for op, st in zip(ops, status)], dtype=np.uint8)


def restated(ders, issuers, anchors, now, crl=None, cover=None, pad=0):
    """the verdicts by the restatements of the three case files, run on the oracle's signature verdicts"""
    crl_entries = [] if crl is None else [(crl, len(crl))]
    blob, certs, items, cert_fields = cc.lay_out(ders, issuers, crl_entries, [0] * len(crl_entries), pad=pad)
    blob = blob[:-1]
    fields, ops, status = xc.expected(blob, certs)
    cert_ok = oracle_ok(blob, ops, status)
    policy = pc.expected_parse(blob, certs)
    revocation = None
    if crl is not None:
        f, e, crl_ops, crl_status, _ = cc.expected(blob, items, fields, cc.max_entries_of(items))
        crl_ok = oracle_ok(blob, crl_ops, crl_status)
        fresh = pc.expected_crl_times(blob, f, crl_status, crl_ok, now)[3]
        revocation = cc.expected_check(blob, certs, fields, [cc.NONE if c is None else c for c in cover], items, f, crl_status, fresh, e)
    anchor = np.zeros(len(ders), dtype=np.uint8)
    anchor[anchors] = 1
    return pc.expected_chain(certs["issuer"], policy, status, cert_ok, revocation, anchor, now, pc.ALLOW_NO_CRL), cert_ok, revocation


def test_validate_against_the_restatement_on_the_oracles_verdicts(pv, pki):
    ders, issuers, anchors, cover = pki["ders"], pki["issuers"], pki["anchors"], pki["cover"]
    flipped = list(ders)
    flipped[3] = ders[3][:-7] + bytes([ders[3][-7] ^ 0x20]) + ders[3][-6:]
    june = calendar.timegm((2025, 6, 15, 0, 0, 0))
    # name -> (certificates, now, CRL, what the certificates 0 ... 11 get)
    T, E, R, V = pc.TRUSTED, pc.EXPIRED, pc.REVOKED, pc.REVOCATION
    scenes = {
        "all good": (ders, june, pki["crls"][0], [T] * 11 + [pc.NOT_CA]),
        "no CRL at all": (ders, YEAR(2027), None, [T] * 11 + [pc.NOT_CA]),
        "intermediates expired": (ders, YEAR(2030) + 1, None, [T, E, E, E, E, E, T, E, E, E, E, pc.NOT_CA]),
        "intermediate revoked": (ders, june, pki["crls"][1], [T, R, R, R, R, R, T, T, T, T, T, pc.NOT_CA]),
        "one flipped signature byte": (flipped, june, pki["crls"][0], [T, T, T, pc.SIG] + [T] * 7 + [pc.NOT_CA]),
        "stale CRL": (ders, YEAR(2026), pki["crls"][0], [T, V, V, V, V, V, T, T, T, T, T, pc.NOT_CA]),
    }
    for name, (certs, now, crl, verdicts) in scenes.items():
        kw = {} if crl is None else dict(crl_ders=[crl], crl_issuers=[0], cert_crl=cover, allow_no_crl=True)
        verdict, where, depth, details = pv.validate(certs, issuers, anchors, now, pad=[3, 0, 9], **kw)
        want, cert_ok, revocation = restated(certs, issuers, anchors, now, crl, cover, pad=[3, 0, 9])
        assert np.array_equal(details["cert_ok"], cert_ok) and not details["cert_status"].any(), name
        if crl is not None:
            assert np.array_equal(details["revocation"], revocation), name
        assert (verdict.tolist(), where.tolist(), depth.tolist()) == (want["verdict"].tolist(), want["where"].tolist(), want["depth"].tolist()), name
        assert verdict.tolist() == verdicts, (name, verdict.tolist())
    # where and depth of the plain case; the leaf under a leaf is stopped at the leaf that issued it
    verdict, where, depth, details = pv.validate(ders, issuers, anchors, YEAR(2027))
    assert where.tolist() == [0, 0, 0, 0, 0, 0, 6, 6, 6, 6, 6, 10] and depth.tolist() == [0, 1, 2, 2, 2, 2, 0, 1, 2, 2, 2, 1]
    assert details["policy"]["flags"].tolist() == [15, 15, 11, 11, 11, 11] * 2
    # with CRLs and without allow_no_crl a certificate that no CRL covers is refused
    verdict, where, _, _ = pv.validate(ders, issuers, anchors, june, crl_ders=[pki["crls"][0]], crl_issuers=[0], cert_crl=cover)
    assert verdict.tolist() == [T, T] + [V] * 4 + [T] + [V] * 5 and where.tolist() == [0, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert pv.validate([], [], [], 0)[0].size == 0
