"""The certificate-issuing library on the device (include/mldsa_x509sign.h): mldsa_x509sign_plan, mldsa_x509sign_frame and
mldsa_x509sign_issue_ops byte for byte against the restatement of tests/x509sign_cases.py -- every size and mix, every defect, a sweep
of single-byte changes, the length edges, the SPACE rule and every alignment --, plan rows a caller tampered with, the whole pass
against the oracle's signatures, the round trip through the verifying libraries, stream order, and the Python front."""
from gpu_common import *  # noqa: F401,F403

import x509_cases as xc
import x509sign_cases as xs
from fips204_amd import _recsign_lib, _x509_lib, _x509sign_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsaCertificateIssuer, MlDsaCertificates

pytestmark = pytest.mark.gpu

CANARY = 0x77
ROWS = 3      # canary rows behind each output array
GUARD = 64    # canary bytes on both sides of the output buffer


@pytest.fixture(scope="module")
def issuer(hp, sets):
    """an issuer that serves xs.N_KEYS rows per set (the seam cases sign nothing: any keys will do)"""
    s = MlDsaCertificateIssuer(hotpath=hp)
    for c, pset in enumerate(xs.SETS):
        _, sk = sets[pset].keygen_from_seed([shake(b"x509sign-key%d" % pset, j) for j in range(xs.N_KEYS[c])])
        s.set_keys(pset, sets[pset].private_keys_from_bytes(sk))
    return s


@pytest.fixture(scope="module")
def signing(hp, sets):
    """an issuer over the two oracle keys per set of the signing cases"""
    s = MlDsaCertificateIssuer(hotpath=hp)
    for pset, seeds in xs.key_seeds().items():
        _, sk = sets[pset].keygen_from_seed(seeds)
        s.set_keys(pset, sets[pset].private_keys_from_bytes(sk))
    return s


def placed(data, shift=0, guard=GUARD):
    """(allocation, view, where the view begins): `data` (uint8 array) on the device behind `guard` + `shift` canary bytes and in front of
    `guard` more; guard + shift decides the view's alignment (allocations are 256-byte aligned)"""
    at = guard + shift
    t = torch.full((at + data.size + guard,), CANARY, dtype=torch.uint8, device="cuda")
    t[at:at + data.size] = torch.from_numpy(data.copy())
    return t, t[at:at + data.size], at


def run_seam(issuer, blob, reqs, out_len, shift=0, out_shift=0, split=False):
    """dict(status, out_certs, ops, totals, out) from mldsa_x509sign_issue_ops (split: from mldsa_x509sign_plan then
    mldsa_x509sign_frame), after checking the canary rows behind each output array and the guard bands around the output buffer"""
    n = len(reqs)
    _, b, _ = placed(blob, shift)
    alloc, o, at = placed(np.full(out_len, CANARY, dtype=np.uint8), out_shift)
    r = issuer.requests_tensor(reqs)
    out_certs = torch.full(((n + ROWS) * 16,), CANARY, dtype=torch.uint8, device="cuda")
    ops = torch.full(((n + ROWS) * 48,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((n + ROWS,), CANARY, dtype=torch.uint8, device="cuda")
    totals = torch.full((3 + ROWS,), -1, dtype=torch.int64, device="cuda")
    plan = torch.full((issuer.lib.mldsa_x509sign_plan_bytes(n),), CANARY, dtype=torch.uint8, device="cuda")
    lib, h, s, nk = issuer.lib, issuer.hp._h, _stream(issuer.device), issuer.signer._n_keys()
    if split:
        _x509sign_lib.check(lib.mldsa_x509sign_plan(h, _ptr(b), b.numel(), _ptr(r), n, nk, out_len, _ptr(out_certs), _ptr(ops), _ptr(status),
                                                    _ptr(totals), _ptr(plan), plan.numel(), s))
        assert (host(alloc) == CANARY).all()  # the plan does not touch the output buffer
        _x509sign_lib.check(lib.mldsa_x509sign_frame(h, _ptr(b), b.numel(), _ptr(r), n, _ptr(o), out_len, _ptr(out_certs), _ptr(status), s))
    else:
        _x509sign_lib.check(lib.mldsa_x509sign_issue_ops(h, _ptr(b), b.numel(), _ptr(r), n, nk, _ptr(o), out_len, _ptr(out_certs), _ptr(ops),
                                                         _ptr(status), _ptr(totals), _ptr(plan), plan.numel(), s))
    c, p, st, tot, whole = host(out_certs), host(ops), host(status), host(totals), host(alloc)
    assert (c[n * 16:] == CANARY).all() and (p[n * 48:] == CANARY).all() and (st[n:] == CANARY).all() and (tot[3:] == -1).all()
    assert (whole[:at] == CANARY).all() and (whole[at + out_len:] == CANARY).all()
    return dict(status=st[:n], out_certs=c[:n * 16].view(_x509_lib.CERT_DTYPE), ops=p[:n * 48].view(_recsign_lib.OP_DTYPE),
                totals=tuple(int(x) for x in tot[:3]), out=whole[at:at + out_len])


def check_seam(got, want, out_len):
    for what in ("status", "out_certs", "ops"):
        g, w = got[what], want[what]
        if not np.array_equal(g, w):
            bad = [i for i in range(len(w)) if g[i] != w[i]]
            raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], g[bad[0]], w[bad[0]]))
    assert got["totals"] == want["totals"]
    # every frame byte; the sentinel outside the accepted ranges and inside the holes
    want_out = xs.framed(np.full(out_len, CANARY, dtype=np.uint8), want)
    if not np.array_equal(got["out"], want_out):
        raise AssertionError("out differs at %s" % np.nonzero(got["out"] != want_out)[0][:8].tolist())


def seam(issuer, blob, reqs, out_len=None, **kw):
    want = xs.expected(blob, reqs, xs.N_KEYS, 2 ** 62)
    out_len = (want["totals"][2] or 33) if out_len is None else out_len  # (nothing accepted: a buffer all the same, to stay untouched)
    want = xs.expected(blob, reqs, xs.N_KEYS, out_len)
    got = run_seam(issuer, blob, reqs, out_len, **kw)
    check_seam(got, want, out_len)
    return got, want


# ------------------------------------------------------------------------------------------------------------------ the seam
@pytest.mark.parametrize("mix", xs.MIXES)
@pytest.mark.parametrize("n", xs.SEAM_SIZES)
def test_seam_matches_the_restatement_byte_for_byte(issuer, n, mix):
    k = xs.SEAM_SIZES.index(n)
    blob, reqs = xs.seam_case(n, mix, seed=n % 7, front=k)
    got, want = seam(issuer, blob, reqs, shift=(0, 1, 3, 15)[k % 4], out_shift=(5, 0, 15, 8, 2)[k])
    if mix in ("mod3", "only44", "only87"):
        assert want["totals"][:2] == (n, 0)
    elif mix == "all_defect":
        assert want["totals"] == (0, n, 0) and (got["out"] == CANARY).all()
    else:
        assert want["totals"][1] == n // 10
    if n == 65:  # the two entry points on their own give what the one call gives
        out_len = want["totals"][2] or 33
        check_seam(run_seam(issuer, blob, reqs, out_len, shift=2, out_shift=9, split=True), xs.expected(blob, reqs, xs.N_KEYS, out_len), out_len)


CARRY_N = 64 * 256 + 1  # 65 workgroups of the scan: the one-wave offsets kernel goes round its carry loop a second time
CARRY_AT = (0, 255, 256, 16127, 16128, 16383, 16384)  # the accepted few: both ends of the first and the 64th workgroup, and the 65th


def test_placement_scan_carries_past_64_workgroups(issuer):
    """16 385 requests of which seven are accepted; every other one is a RANGE refusal (no length, or an offset behind the blob's end),
    so the blob stays seven TBSs long.  Then the same with one byte too few: the first certificate that does not fit is the one behind
    the carry, and it corrects the totals."""
    tbss = [xs.good_tbs(xs.SETS[j % 3], b"carry", j, tail=xc.extensions(3 * j)) for j in range(len(CARRY_AT))]
    blob, few = xs.lay_out([(xs.SETS[j % 3], j % 4, t, len(t), xc._bytes(b"crnd", j, 32) if j % 2 else None, j) for j, t in enumerate(tbss)],
                           pad=[0, 3, 8, 13, 5], front=1)
    reqs = np.zeros(CARRY_N, dtype=few.dtype)
    reqs["set"], reqs["key"], reqs["issuer"] = 44, 1, xs.NO_ISSUER
    reqs["off"][1::2], reqs["len"][1::2] = blob.size + 1, 100  # behind the end; the even ones have no length
    reqs[list(CARRY_AT)] = few
    got, want = seam(issuer, blob, reqs, shift=1, out_shift=3)
    assert np.nonzero(want["status"] == xs.OK)[0].tolist() == list(CARRY_AT) and (want["status"] == xs.RANGE).sum() == CARRY_N - len(CARRY_AT)
    need = want["totals"][2]
    assert want["totals"] == (len(CARRY_AT), CARRY_N - len(CARRY_AT), need) and int(got["out_certs"][CARRY_AT[-1]]["off"]) > 6 * 2400
    got, short = seam(issuer, blob, reqs, out_len=need - 1, shift=1, out_shift=3)
    assert np.nonzero(short["status"] == xs.SPACE)[0].tolist() == [CARRY_AT[-1]]
    assert got["totals"] == (len(CARRY_AT) - 1, CARRY_N - len(CARRY_AT) + 1, need)


def test_every_defect_among_valid_neighbours(issuer):
    blob, reqs, at = xs.defect_batch()
    got, want = seam(issuer, blob, reqs, shift=3, out_shift=1)
    for name, i in at.items():
        assert got["status"][i] == xs.DEFECTS[name], name
        assert got["ops"][i].tobytes() == bytes(48) and got["out_certs"][i].tobytes() == bytes(12) + b"\xff" * 4, name
        for j in (i - 1, i + 1):  # the neighbours are untouched
            assert got["status"][j] == 0 and got["ops"][j]["set"] in xs.SETS, name
    # an unserved set: every request of it is KEY, its neighbours of other sets are as they were
    held = issuer.signer._keys[65]
    issuer.set_keys(65, None)
    try:
        want = xs.expected(blob, reqs, (4, 0, 4), 2 ** 62)
        want = xs.expected(blob, reqs, (4, 0, 4), want["totals"][2])
        assert (want["status"] == xs.KEY).sum() > 20
        check_seam(run_seam(issuer, blob, reqs, want["totals"][2]), want, want["totals"][2])
    finally:
        issuer.set_keys(65, held)


def test_single_byte_mutation_sweep(issuer):
    blob, reqs = xs.mutation_batch(xs.good_tbs(44, b"mut", 0))
    assert len(reqs) == 910
    got, want = seam(issuer, blob, reqs, shift=1, out_shift=3)
    hist = np.bincount(got["status"], minlength=12)
    assert hist[xs.ALG] == 77 and hist[xs.DER] > 0 and hist[xs.OK] > 0


def test_length_edges(issuer):
    blob, reqs, status = xs.edge_batch()
    got, want = seam(issuer, blob, reqs, shift=7, out_shift=11)
    assert got["status"].tolist() == status and sorted(int(c["len"]) for c in got["out_certs"])[-3:] == [65539] * 3


def test_space_rule(issuer):
    blob, reqs = xs.seam_case(65, "tenth_defect", seed=3)
    free = xs.expected(blob, reqs, xs.N_KEYS, 2 ** 62)
    need = free["totals"][2]
    mid = sorted(free["frames"])[len(free["frames"]) // 2]
    for out_len in (need, need - 1, int(free["out_certs"][mid]["off"]) + 100, 1):
        got, want = seam(issuer, blob, reqs, out_len=out_len, out_shift=out_len % 16)
        assert got["totals"][2] == need and got["totals"][0] + got["totals"][1] == 65
        assert (got["status"] == xs.SPACE).sum() == {need: 0, need - 1: 1, 1: len(free["frames"])}.get(out_len, len([i for i in free["frames"] if i >= mid]))


@pytest.mark.parametrize("front", range(16))
def test_every_alignment_of_blob_and_output(issuer, front):
    blob, reqs = xs.alignment_batch(front=front)
    # allocations are 256-byte aligned and GUARD is a multiple of 16: `front` is the blob's first TBS's and the output buffer's residue
    got, want = seam(issuer, blob, reqs, shift=0, out_shift=front)
    assert not got["status"].any()
    assert {(GUARD + int(r["off"])) % 16 for r in reqs} == set(range(16)) == {(GUARD + front + int(c["off"])) % 16 for c in got["out_certs"]}


def test_frame_does_not_follow_tampered_rows(issuer):
    """mldsa_x509sign_frame on out_certs / status rows a caller changed: a row that points outside the output buffer, or whose length is
    not its request's, writes nothing; neither does a request that points outside the blob"""
    n = 8
    tbss = [xs.good_tbs(44, b"tamper", i) for i in range(n)]
    blob, reqs = xs.lay_out([(44, 0, t, len(t), None, i) for i, t in enumerate(tbss)], pad=3)
    want = xs.expected(blob, reqs, xs.N_KEYS, 2 ** 62)
    out_len = want["totals"][2]
    assert not want["status"].any()
    rows, status, treqs = want["out_certs"].copy(), want["status"].copy(), reqs.copy()
    clen = int(rows[0]["len"])
    rows[0]["off"] = out_len - clen + 1          # ends one byte behind the buffer
    rows[1]["off"] = 2 ** 64 - 8                 # wraps
    rows[2]["len"] = clen - 1                    # not the length of its request
    rows[3]["off"], rows[3]["len"] = out_len, 0
    status[4] = xs.DER                           # refused: not framed, whatever its row says
    treqs[5]["off"] = blob.size - 10             # the TBS would be read behind the blob
    treqs[6]["set"] = 66                         # no set: no frame
    _, b, _ = placed(blob, 1)
    alloc, o, at = placed(np.full(out_len, CANARY, dtype=np.uint8), 5)
    _x509sign_lib.check(issuer.lib.mldsa_x509sign_frame(issuer.hp._h, _ptr(b), b.numel(), _ptr(issuer.requests_tensor(treqs)), n, _ptr(o), out_len,
                                                        _ptr(dev(rows.view(np.uint8))), _ptr(dev(status)), _stream(issuer.device)))
    only7 = dict(want, frames={7: want["frames"][7]})
    want_alloc = np.full(alloc.numel(), CANARY, dtype=np.uint8)
    want_alloc[at:at + out_len] = xs.framed(np.full(out_len, CANARY, dtype=np.uint8), only7)
    assert np.array_equal(host(alloc), want_alloc)  # certificate 7 alone; the guard bands on both sides at the sentinel


# ------------------------------------------------------------------------------------------------------------------ the whole pass
def issue(signing, requests, shift=0, out_shift=0, pad=None, slack=0):
    """issue_device on the requests: (whole output buffer, out_certs, status, sig_status, totals, blob, reqs)"""
    blob, reqs = xs.tbs_blob(requests, pad=list(range(16)) if pad is None else pad)
    out_len = xs.expected(blob, reqs, xs.SIGN_N_KEYS, 2 ** 62)["totals"][2] + slack
    _, b, _ = placed(blob, shift)
    alloc, o, at = placed(np.full(out_len, CANARY, dtype=np.uint8), out_shift)
    sig_status = torch.full((len(reqs) + ROWS,), 0x77777777, dtype=torch.int32, device="cuda")
    out_certs, status, totals = signing.issue_device(b, signing.requests_tensor(reqs), o, sig_status, len(reqs))
    whole = host(alloc)
    assert (whole[:at] == CANARY).all() and (whole[at + out_len:] == CANARY).all() and (host(sig_status)[len(reqs):] == 0x77777777).all()
    return dict(out=whole[at:at + out_len], out_certs=host(out_certs).view(_x509_lib.CERT_DTYPE), status=host(status),
                sig_status=host(sig_status)[:len(reqs)], totals=tuple(host(totals).tolist()), blob=blob, reqs=reqs, dev_out=o, dev_certs=out_certs)


@pytest.mark.parametrize("name", ["pass65", "pass257"])
def test_whole_pass_equals_the_oracles_certificates(signing, name):
    requests = xs.signing_cases()[name]
    sigs, iters = xs.oracle_signed(name)
    got = issue(signing, requests, shift=len(requests) % 4, out_shift=len(requests) % 5, slack=7)
    assert not got["status"].any() and not got["sig_status"].any() and got["totals"] == (len(requests), 0, got["out"].size - 7)
    at = 0
    for i, (pset, key, tbs, rnd, issuer_i) in enumerate(requests):  # deterministic and with rnd, every other one
        der = xc.cert(tbs, pset, sigs[i])
        assert tuple(got["out_certs"][i]) == (at, len(der), issuer_i)
        assert got["out"][at:at + len(der)].tobytes() == der, i
        at += len(der)
    assert (got["out"][at:] == CANARY).all()


def test_round_trip_through_the_verifying_libraries(signing, hp):
    """roots, intermediates and leaves issued in ONE call, the issuer's index copied through: mldsa_x509_ops with CHECK_NAMES and
    mldsa_rec_verify on out / out_certs accept every one; a certificate signed with the wrong key row is framed and fails verification"""
    requests = xs.signing_cases()["chains"]
    got = issue(signing, requests, shift=3, out_shift=9)
    assert not got["status"].any() and not got["sig_status"].any()
    assert [int(c["issuer"]) for c in got["out_certs"]] == [r[4] for r in requests]
    x5 = MlDsaCertificates(hotpath=hp)
    ok = torch.full((12 + ROWS,), CANARY, dtype=torch.uint8, device="cuda")
    st = x5.verify_device(got["dev_out"], got["dev_certs"], ok)
    assert host(st).tolist() == [0] * 12 and host(ok).tolist() == [1] * 12 + [CANARY] * ROWS
    sigs, _ = xs.oracle_signed("chains")
    assert got["out"].tobytes() == b"".join(xc.cert(r[2], r[0], s) for r, s in zip(requests, sigs))
    # the 65 intermediate (request 4) under the other key row of its issuer's set: a certificate, but not one its issuer's key verifies;
    # its own child, signed by the right key, still verifies
    wrong = xs.signing_cases()["chains_wrong_row"]
    assert [i for i in range(12) if wrong[i] != requests[i]] == [4] and wrong[4][1] == 1 - requests[4][1]
    got = issue(signing, wrong, out_shift=2)
    assert not got["status"].any() and not got["sig_status"].any()
    st = x5.verify_device(got["dev_out"], got["dev_certs"], ok)
    assert host(st).tolist() == [0] * 12 and host(ok)[:12].tolist() == [int(i != 4) for i in range(12)]


def test_back_to_back_calls_into_one_plan_memory_on_a_side_stream(issuer):
    """a caller-owned stream: a second call into the same plan memory, then a stream-ordered copy of the first call's outputs -- they are
    what the first call alone gives"""
    blob_a, reqs_a = xs.seam_case(257, "tenth_defect", seed=1)
    blob_b, reqs_b = xs.seam_case(65, "all_defect", seed=4)
    want = xs.expected(blob_a, reqs_a, xs.N_KEYS, 2 ** 62)
    out_len = want["totals"][2]
    _, ba, _ = placed(blob_a, 1)
    _, bb, _ = placed(blob_b, 2)
    ra, rb = issuer.requests_tensor(reqs_a), issuer.requests_tensor(reqs_b)
    plan = issuer.plan_memory(257)
    out_a = torch.full((out_len,), CANARY, dtype=torch.uint8, device="cuda")
    out_b = torch.full((out_len,), CANARY, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = issuer.issue_ops_device(ba, ra, out_a, 257, plan=plan)
        second = issuer.issue_ops_device(bb, rb, out_b, 65, plan=plan)
        copies = [t.clone() for t in first] + [out_a.clone()]
    side.synchronize()
    got = dict(out_certs=host(copies[0]).view(_x509_lib.CERT_DTYPE), ops=host(copies[1]).view(_recsign_lib.OP_DTYPE), status=host(copies[2]),
               totals=tuple(host(copies[3]).tolist()), out=host(copies[4]))
    check_seam(got, want, out_len)
    assert host(second[3]).tolist() == [0, 65, 0] and (host(out_b) == CANARY).all()


def test_python_front(signing):
    requests = xs.signing_cases()["front"]
    sigs, _ = xs.oracle_signed("front")
    certs, status, sig_status = signing.issue(requests, pad=[0, 5, 11])
    assert status.tolist() == [0] * 7 and sig_status.tolist() == [0] * 7
    assert certs == [xc.cert(r[2], r[0], s) for r, s in zip(requests, sigs)]
    got = issue(signing, requests, pad=[0, 5, 11])  # issue_device gives the same bytes
    assert got["out"].tobytes() == b"".join(certs)
    # a refused request yields no certificate and leaves the others as they were
    bad = list(requests)
    bad[2] = (bad[2][0], 2, bad[2][2], bad[2][3], bad[2][4])  # key row 2 of 2
    bad[5] = (87 if bad[5][0] != 87 else 44,) + bad[5][1:]   # a TBS that names another set
    c2, st2, sst2 = signing.issue(bad)
    assert st2.tolist() == [0, 0, xs.KEY, 0, 0, xs.ALG, 0] and [c is None for c in c2] == [s != 0 for s in st2]
    assert [c for c in c2 if c is not None] == [c for i, c in enumerate(certs) if i not in (2, 5)]
    assert sst2[2] == sst2[5] == -1 and not sst2[[0, 1, 3, 4, 6]].any()  # the signer refuses an all-zero op by its own rule 1
    assert signing.issue([])[0] == []
    blob, reqs = signing.tbs_blob(requests, pad=7, front=3)
    assert blob[:10].tolist() == [0xC3] * 10 and int(reqs[0]["off"]) == 10 and reqs.dtype == _x509sign_lib.REQ_DTYPE
