"""The certificate library on the device (include/mldsa_x509.h): the seam -- mldsa_x509_parse, mldsa_x509_link and mldsa_x509_ops -- byte
for byte against the restatement of tests/x509_cases.py, every defect and a sweep of single-byte changes among valid neighbours, the link
rules, and whole chains verified through mldsa_rec_verify against the oracle, in stream order and through the Python front."""
from gpu_common import *  # noqa: F401,F403

import x509_cases as xc
from fips204_amd import _rec_lib, _x509_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsaCertificates, certificates_blob

pytestmark = pytest.mark.gpu

CANARY = 0x77
ROWS = 3  # canary rows behind each output array


@pytest.fixture(scope="module")
def x5(hp):
    return MlDsaCertificates(hotpath=hp)


def blob_dev(blob, shift=0):
    """the blob on the device, `shift` bytes into its allocation (so its address is that far from 256-byte alignment)"""
    t = torch.full((blob.size + shift + 1,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + blob.size] = torch.from_numpy(blob.copy())
    return t[shift:shift + blob.size]


def run_seam(x5, blob, certs, flags=xc.CHECK_NAMES, shift=0, split=False):
    """(fields, ops, status) as numpy arrays from mldsa_x509_ops (split: from mldsa_x509_parse then mldsa_x509_link), after checking the
    canary rows behind each of the three output arrays"""
    n = len(certs)
    b, c = blob_dev(blob, shift), x5.certs_tensor(certs)
    fields = torch.full(((n + ROWS) * 56,), CANARY, dtype=torch.uint8, device="cuda")
    ops = torch.full(((n + ROWS) * 40,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((n + ROWS,), CANARY, dtype=torch.uint8, device="cuda")
    lib, h, s = x5.lib, x5.hp._h, _stream(x5.device)
    if split:
        _x509_lib.check(lib.mldsa_x509_parse(h, _ptr(b), b.numel(), _ptr(c), n, _ptr(fields), s))
        _x509_lib.check(lib.mldsa_x509_link(h, _ptr(b), b.numel(), _ptr(c), _ptr(fields), n, flags, _ptr(ops), _ptr(status), s))
    else:
        _x509_lib.check(lib.mldsa_x509_ops(h, _ptr(b), b.numel(), _ptr(c), n, flags, _ptr(fields), _ptr(ops), _ptr(status), s))
    f, o, st = host(fields), host(ops), host(status)
    assert (f[n * 56:] == CANARY).all() and (o[n * 40:] == CANARY).all() and (st[n:] == CANARY).all()
    return f[:n * 56].view(_x509_lib.FIELDS_DTYPE), o[:n * 40].view(_rec_lib.OP_DTYPE), st[:n]


def check_seam(got, want):
    for g, w, what in zip(got, want, ("fields", "ops", "status")):
        if not np.array_equal(g, w):
            bad = [i for i in range(len(w)) if g[i] != w[i]]
            raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], g[bad[0]], w[bad[0]]))


# ------------------------------------------------------------------------------------------------------------------ the seam
@pytest.mark.parametrize("mix", xc.MIXES)
@pytest.mark.parametrize("n", xc.SEAM_SIZES)
def test_seam_matches_the_restatement_byte_for_byte(x5, n, mix):
    shift = (0, 1, 3, 15)[xc.SEAM_SIZES.index(n) % 4]
    blob, certs = xc.seam_case(n, mix, seed=n % 7)
    want = xc.expected(blob, certs)
    if mix.startswith("only") or mix == "mod3":
        assert (want[2] == 0).all() and (want[1]["set"] != 0).all()
    elif mix == "all_defect":
        assert (want[2] != 0).sum() >= n - n // 3  # (a defective key leaves a root accepted; a defective issuer fails its child)
    else:
        assert (want[0]["status"] != 0).sum() == sum(1 for i in range(n) if i % 10 == 9 and xc.DEFECTS[list(xc.DEFECTS)[(i + n % 7) % len(xc.DEFECTS)]])
    check_seam(run_seam(x5, blob, certs, shift=shift), want)
    if n == 65:  # the two entry points on their own give what the one call gives, with and without the flag
        check_seam(run_seam(x5, blob, certs, shift=shift, split=True), want)
        check_seam(run_seam(x5, blob, certs, flags=0, shift=1, split=True), xc.expected(blob, certs, 0))


def test_seam_fan_out_and_coinciding_ranges(x5):
    # 64 leaves under one intermediate under one root; then the same leaf range named 5 times, and a root that overlaps nothing else
    root = xc.random_cert(65, 65, b"root", b"root", b"fan", 0)
    mid = xc.random_cert(65, 65, b"root", b"m" * 140, b"fan", 1)
    leaves = [xc.random_cert(65, (44, 65, 87, 0)[i % 4], b"m" * 140, b"leaf%d" % i, b"fan", 2 + i, tail=xc.extensions(i)) for i in range(64)]
    ders = [root, mid] + leaves
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [0, 0] + [1] * 64, pad=list(range(16)))
    certs = np.concatenate([certs, np.repeat(certs[7:8], 5)])
    want = xc.expected(blob, certs)
    assert (want[2] == 0).all() and len(set(int(x) for x in want[1]["pk_off"][2:])) == 1
    for shift in (0, 1, 3, 15):
        check_seam(run_seam(x5, blob, certs, shift=shift), want)


# ------------------------------------------------------------------------------------------------------------------ defects
def test_every_defect_among_valid_neighbours(x5):
    names = list(xc.DEFECTS)
    entries, issuers, at = [], [], {}
    for k, defect in enumerate(names):
        pset = xc.SETS[k % 3]
        good = [xc.random_cert(pset, pset, b"self", b"self", b"nb", 3 * k + j) for j in range(3)]
        at[defect] = len(entries) + 1
        entries += [(good[0], len(good[0])), xc.make_defect(good[1], defect), (good[2], len(good[2]))]
        # every certificate its own issuer, but the two whose key is useless: their left neighbour issues them
        issuers += [len(issuers), len(issuers) + (0 if defect in xc.KEY_SET_ZERO else 1), len(issuers) + 2]
    blob, certs = xc.lay_out(entries, issuers, pad=[0, 3, 8, 13], front=2)
    want = xc.expected(blob, certs)
    fields, ops, status = run_seam(x5, blob, certs, shift=3)
    check_seam((fields, ops, status), want)
    for defect, i in at.items():
        assert status[i] == xc.DEFECTS[defect], defect
        assert (ops[i].tobytes() == bytes(40)) == (status[i] != 0), defect
        assert (fields[i]["key_set"] == 0) == (status[i] == xc.DER or defect in xc.KEY_SET_ZERO), defect
        for j in (i - 1, i + 1):  # the neighbours are untouched
            assert status[j] == 0 and ops[j]["set"] in xc.SETS and ops[j]["pk_off"] == fields[j]["key_off"], defect
    # one byte short with the missing byte in the blob behind it: malformed, not accepted
    i = at["len_one_short"]
    assert blob[int(certs[i]["off"]) + int(certs[i]["len"])] == entries[i][0][-1] and status[i] == xc.DER
    # a certificate whose key is useless cannot be an issuer
    certs[at["key_one_short"] + 1]["issuer"] = at["key_one_short"]
    certs[at["spki_other_oid"] + 1]["issuer"] = at["spki_other_oid"]
    got = run_seam(x5, blob, certs)
    check_seam(got, xc.expected(blob, certs))
    assert got[2][at["key_one_short"] + 1] == got[2][at["spki_other_oid"] + 1] == xc.ISSUER


def test_range_rule_and_the_ends_of_the_blob(x5):
    good = xc.random_cert(44, 44, b"self", b"self", b"rng", 0)
    blob, certs = certificates_blob([good] * 8, list(range(8)), pad=0)  # flush against both ends of the blob
    assert int(certs[7]["off"]) + len(good) == blob.size
    certs[1]["off"], certs[1]["len"] = blob.size - 1, 2            # ends one byte behind the blob
    certs[2]["off"] = 2 ** 64 - 1                                  # no wrap gets past the test
    certs[3]["len"] = 1                                            # shorter than a header
    certs[4]["off"], certs[4]["len"] = blob.size, 0
    certs[5]["off"], certs[5]["len"] = blob.size - 2, 2            # the last two bytes: inside, and malformed
    certs[6]["len"] = 2 ** 32 - 1
    want = xc.expected(blob, certs)
    assert want[2].tolist() == [0, xc.RANGE, xc.RANGE, xc.RANGE, xc.RANGE, xc.DER, xc.RANGE, 0]
    for shift in (0, 1):
        check_seam(run_seam(x5, blob, certs, shift=shift), want)


def test_single_byte_mutation_sweep(x5):
    der = xc.random_cert(44, 44, b"root", b"root", b"mut", 0)
    blob, certs = xc.mutation_batch(der)
    assert len(certs) == xc.MUTATION_SPAN * len(xc.MUTATION_VALUES) == 910
    want = xc.expected(blob, certs)
    hist = np.bincount(want[2], minlength=8)
    # the sweep reaches the rules: headers (DER), the 11 bytes of the inner OID times seven values (ALG), the SPKI's OID (a useless key:
    # ISSUER, every copy being its own issuer), the two Names (NAME), and content nobody looks at (accepted)
    assert hist[xc.ALG] == 77 and min(hist[xc.DER], hist[xc.ISSUER], hist[xc.NAME], hist[xc.OK]) > 0 and hist.sum() == 910
    check_seam(run_seam(x5, blob, certs, shift=1), want)


# ------------------------------------------------------------------------------------------------------------------ the link
def test_link_rules(x5):
    # Names of 63, 64 and 65 bytes (one step of the comparison, and one byte more), 127, 128 and 129 (two steps), and of the 0x81 and 0x82 forms
    cn = {k: b"n" * k for k in (40, 50, 51, 52, 114, 115, 116, 117, 300)}
    assert [len(xc.name(c)) for c in cn.values()] == [53, 63, 64, 65, 127, 128, 129, 131, 321]
    last = lambda b: b[:-1] + b"N"   # noqa: E731
    first = lambda b: b"N" + b[1:]   # noqa: E731
    ders, issuers = [], []
    for k, name in cn.items():  # a root, a child that names it, one whose issuer Name differs in the last byte, one in the first
        base = len(ders)
        ders += [xc.random_cert(87, 87, name, name, b"ln", base), xc.random_cert(87, 87, name, b"c", b"ln", base + 1),
                 xc.random_cert(87, 87, last(name), b"c", b"ln", base + 2), xc.random_cert(87, 87, first(name), b"c", b"ln", base + 3)]
        issuers += [base, base, base, base]
    n0 = len(ders)
    ders += [xc.random_cert(87, 87, cn[51] + b"n", b"c", b"ln", 90),     # n0: an issuer Name one byte longer than the root's
             xc.random_cert(87, 87, cn[51][:-1], b"c", b"ln", 91),       # n0 + 1: one byte shorter
             xc.random_cert(44, 0, cn[51], b"rsa", b"ln", 92),           # n0 + 2: its own issuer, and its key is an RSA key
             xc.random_cert(44, 44, cn[51], b"c", b"ln", 93),            # n0 + 3: a 44 signature under the 87 root: cross-set
             xc.random_cert(44, 44, b"rsa", b"c", b"ln", 94),            # n0 + 4: under the RSA key
             xc.random_cert(87, 65, cn[51], b"c", b"ln", 95),            # n0 + 5: parse only
             xc.random_cert(87, 87, cn[51], b"c", b"ln", 96),            # n0 + 6: issuer out of range
             xc.random_cert(87, 87, cn[51], b"c", b"ln", 97)]            # n0 + 7: issuer out of range by far
    root64 = 4 * list(cn).index(51)
    n = len(ders) + 2
    issuers += [root64, root64, n0 + 2, root64, n0 + 2, xc.NO_ISSUER, n, 2 ** 32 - 2]
    broken = xc.make_defect(ders[root64], "wrong_tag_issuer")
    badsig = xc.make_defect(ders[root64], "sig_one_short")
    entries = [(d, len(d)) for d in ders] + [broken, badsig]
    issuers += [n - 2, n - 1]
    blob, certs = xc.lay_out(entries, issuers, pad=[1, 6, 11, 0], front=5)
    want = xc.expected(blob, certs)
    per_root = [0, 0, xc.NAME, xc.NAME]
    assert want[2].tolist() == per_root * len(cn) + [xc.NAME, xc.NAME, xc.ISSUER, xc.ISSUER, xc.ISSUER, xc.PARSE_ONLY, xc.ISSUER, xc.ISSUER,
                                                     xc.DER, xc.SIG]
    got = run_seam(x5, blob, certs, shift=3)
    check_seam(got, want)
    assert got[1][n0 + 5].tobytes() == bytes(40) and got[0][n0 + 5]["key_set"] == 65 and got[0][n0 + 5]["sig_off"] != 0  # fields filled
    # without the flag no Name is compared
    want0 = xc.expected(blob, certs, 0)
    assert want0[2].tolist()[:n0 + 2] == [0] * (n0 + 2)
    check_seam(run_seam(x5, blob, certs, flags=0), want0)
    # a malformed issuer refuses its children, one whose own signature field is bad still lends its key
    certs[1]["issuer"], certs[5]["issuer"] = n - 2, n - 1
    want = xc.expected(blob, certs)
    assert want[2][1] == xc.ISSUER and want[2][5] == xc.NAME and xc.expected(blob, certs, 0)[2][5] == xc.OK
    check_seam(run_seam(x5, blob, certs), want)
    check_seam(run_seam(x5, blob, certs, flags=0), xc.expected(blob, certs, 0))


def test_link_does_not_follow_a_fields_row_out_of_the_blob(x5):
    """mldsa_x509_link on rows a caller changed: a Name range that does not lie inside the blob is a mismatch and is not read"""
    ders = [xc.random_cert(44, 44, b"root", b"root", b"tamper", 0)] + [xc.random_cert(44, 44, b"root", b"c%d" % i, b"tamper", i) for i in (1, 2, 3)]
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], [0, 0, 0, 0], pad=3)
    fields, _, status = xc.expected(blob, certs)
    assert status.tolist() == [0, 0, 0, 0]
    fields[1]["issuer_off"] = blob.size - 3                       # ends behind the blob
    fields[2]["issuer_off"] = 2 ** 64 - 8                         # wraps
    fields[3]["issuer_len"] = fields[0]["subject_len"] + 1        # another length
    b, c = blob_dev(blob, 1), x5.certs_tensor(certs)
    f = torch.from_numpy(fields.view(np.uint8).copy()).cuda()
    ops = torch.full((4 * 40,), CANARY, dtype=torch.uint8, device="cuda")
    st = torch.full((4,), CANARY, dtype=torch.uint8, device="cuda")
    _x509_lib.check(x5.lib.mldsa_x509_link(x5.hp._h, _ptr(b), b.numel(), _ptr(c), _ptr(f), 4, xc.CHECK_NAMES, _ptr(ops), _ptr(st), _stream(x5.device)))
    assert host(st).tolist() == [0, xc.NAME, xc.NAME, xc.NAME] and not host(ops)[40:].any()


# ------------------------------------------------------------------------------------------------------------------ whole chains
@pytest.fixture(scope="module")
def chains():
    """four chains of depth 3 signed by the oracle -- one per parameter set and one that crosses them -- and a fan of leaves"""
    ders, issuers = [], []
    for psets, tag in (((44, 44, 44), b"g44"), ((65, 65, 65), b"g65"), ((87, 87, 87), b"g87"), ((87, 65, 44), b"gx")):
        d, iss = xc.signed_chain(psets, tag)
        issuers += [len(ders) + j for j in iss]
        ders += d
    return ders, issuers


def run_verify(x5, blob, certs, shift=0, check_names=True):
    n = len(certs)
    ok = torch.full((n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    status = x5.verify_device(blob_dev(blob, shift), x5.certs_tensor(certs), ok, check_names=check_names)
    got = host(ok)
    assert (got[n:] == CANARY).all() and set(got[:n].tolist()) <= {0, 1}
    return got[:n].astype(bool), host(status)


def oracle_ok(blob, certs, flags=xc.CHECK_NAMES):
    raw = blob.tobytes()
    _, ops, status = xc.expected(blob, certs, flags)
    out = []
    for op, st in zip(ops, status):
        pset = int(op["set"])
        cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
        out.append(st == 0 and bool(orc.verify_internal(pset, orc.pk_try_from_bytes(pset, cut(op["pk_off"], xc.PK_LEN[pset])),
                                                        cut(op["msg_off"], op["msg_len"]), cut(op["sig_off"], xc.SIG_LEN[pset]), ctx=b"",
                                                        mode=orc.MODE_PURE)))
    return np.array(out, dtype=bool), status


def test_chains_verify_and_single_flips_fail_exactly_their_certificates(x5, chains):
    ders, issuers = chains
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], issuers, pad=list(range(16)), front=1)
    fields = xc.expected(blob, certs)[0]
    for shift in (0, 3):
        ok, status = run_verify(x5, blob, certs, shift)
        assert ok.all() and not status.any()
    bad = blob.copy()
    bad[int(fields[1]["tbs_off"]) + 12] ^= 1      # the serial of the 44 intermediate: its own verdict, not its child's
    bad[int(fields[5]["sig_off"]) + 100] ^= 0x40  # the signature of the 65 leaf
    bad[int(fields[6]["key_off"]) + 500] ^= 2     # the key of the 87 root: itself and its child, not its grandchild
    bad[int(fields[10]["issuer_off"]) + 16] ^= 4  # the issuer Name of the crossing chain's intermediate: its TBS too
    want_ok, want_st = oracle_ok(bad, certs)
    assert [i for i in range(12) if not want_ok[i]] == [1, 5, 6, 7, 10] and want_st.tolist() == [0] * 10 + [xc.NAME, 0]
    ok, status = run_verify(x5, bad, certs, shift=1)
    assert np.array_equal(ok, want_ok) and np.array_equal(status, want_st)
    ok, status = run_verify(x5, bad, certs, check_names=False)  # without the flag the damaged Name is the signature's to refuse
    assert [i for i in range(12) if not ok[i]] == [1, 5, 6, 7, 10] and not status.any()
    # a key flip fails every child of that issuer: a fan of leaves, defective certificates and a parse-only one among them
    fan = np.concatenate([certs, np.repeat(certs[2:3], 3), certs[0:1], certs[4:5]])
    fan[15]["issuer"], fan[16]["len"] = xc.NO_ISSUER, fan[16]["len"] - 1
    bad = blob.copy()
    bad[int(fields[1]["key_off"])] ^= 0x80
    want_ok, want_st = oracle_ok(bad, fan)
    assert [i for i in range(17) if not want_ok[i]] == [1, 2, 12, 13, 14, 15, 16] and want_st.tolist()[12:] == [0, 0, 0, xc.PARSE_ONLY, xc.DER]
    ok, status = run_verify(x5, bad, fan)
    assert np.array_equal(ok, want_ok) and np.array_equal(status, want_st)


def test_back_to_back_calls_and_a_side_stream_are_ordered(x5, chains):
    ders, issuers = chains
    blob, certs = xc.lay_out([(d, len(d)) for d in ders], issuers, pad=[2, 5])
    bad = blob.copy()
    bad[int(xc.expected(blob, certs)[0][4]["sig_off"])] ^= 1
    scratch = x5.records.verify_scratch(12, 4 * blob.size, 4 * blob.size)
    da, db, c = blob_dev(blob), blob_dev(bad, 3), x5.certs_tensor(certs)
    ok_a = torch.full((12,), CANARY, dtype=torch.uint8, device="cuda")
    ok_b = torch.full((12,), CANARY, dtype=torch.uint8, device="cuda")
    st_b = torch.full((12,), CANARY, dtype=torch.uint8, device="cuda")
    x5.verify_device(da, c, ok_a, scratch=scratch)
    assert x5.verify_device(db, c, ok_b, status=st_b, scratch=scratch).data_ptr() == st_b.data_ptr()  # no wait in between
    assert host(ok_a).tolist() == [1] * 12 and host(ok_b).tolist() == [int(i != 4) for i in range(12)] and not host(st_b).any()
    # on a side stream the call runs behind the upload that precedes it there
    side = torch.cuda.Stream()
    pinned = torch.from_numpy(bad.copy()).pin_memory()
    target = torch.zeros(bad.size, dtype=torch.uint8, device="cuda")
    ok_s = torch.full((12,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        target.copy_(pinned, non_blocking=True)
        ops, st_s, _ = x5.ops_device(target, c)
        x5.records.verify_device(target, ops, ok_s, 12, scratch=scratch)
    side.synchronize()
    assert host(ok_s).tolist() == host(ok_b).tolist() and not host(st_s).any()


def test_python_front(x5, chains):
    ders, issuers = chains
    ok, status = x5.verify(ders, issuers, pad=[0, 5, 11])
    assert ok.all() and ok.dtype == bool and status.tolist() == [0] * 12
    # the leaf of the first chain under the wrong intermediate: same set, another key and another Name
    wrong = list(issuers)
    wrong[2] = 0
    ok, status = x5.verify(ders, wrong)
    assert [i for i in range(12) if not ok[i]] == [2] and status[2] == xc.NAME
    ok, status = x5.verify(ders, wrong, check_names=False)
    assert [i for i in range(12) if not ok[i]] == [2] and status[2] == 0  # the signature itself refuses it
    ok, status = x5.verify(ders, [None] * 12)
    assert not ok.any() and status.tolist() == [xc.PARSE_ONLY] * 12
    assert x5.verify([], [])[0].size == 0
    blob, certs = certificates_blob(ders, issuers, pad=7, front=3)
    ops, st, fields = x5.ops_device(blob_dev(blob), x5.certs_tensor(certs))
    check_seam((host(fields).view(_x509_lib.FIELDS_DTYPE), host(ops).view(_rec_lib.OP_DTYPE), host(st)), xc.expected(blob, certs))
