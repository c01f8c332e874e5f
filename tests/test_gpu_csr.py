"""The certification-request library on the device (include/mldsa_csr.h): mldsa_csr_parse, mldsa_csr_tbs_plan, mldsa_csr_tbs_write and
mldsa_csr_tbs byte for byte against the restatement of tests/csr_cases.py -- every size and mix, every defect of both stages, a sweep of
single-byte changes, every pair of alignments, the length edges and the SPACE rule, the untouched bytes of the output buffer --, rows a
caller tampered with, and the five calls end to end against the oracle and through the verifying libraries."""
from gpu_common import *  # noqa: F401,F403

import csr_cases as cs
import x509_cases as xc
from fips204_amd import _csr_lib, _rec_lib, _x509_lib, _x509sign_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsaCertificateRequests, MlDsaCertificates

pytestmark = pytest.mark.gpu

CANARY = 0x77
ROWS = 3      # canary rows behind each output array
GUARD = 64    # canary bytes on both sides of the output buffer


@pytest.fixture(scope="module")
def front(hp):
    return MlDsaCertificateRequests(hotpath=hp)


def placed(data, shift=0, fill=CANARY):
    """(allocation, view, where the view begins): `data` (uint8 array) on the device behind GUARD + `shift` bytes of `fill` and in front of
    GUARD more; GUARD + shift decides the view's alignment (allocations are 256-byte aligned)"""
    at = GUARD + shift
    t = torch.full((at + data.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    t[at:at + data.size] = torch.from_numpy(data.copy())
    return t, t[at:at + data.size], at


def rows(n, size):
    return torch.full(((n + ROWS) * size,), CANARY, dtype=torch.uint8, device="cuda")


def run_parse(front, blob_d, items):
    """(fields, ops, status) of mldsa_csr_parse, after checking the canary rows behind each output array"""
    n = len(items)
    fields, ops, status, items_d = rows(n, 56), rows(n, 40), rows(n, 1), front.items_tensor(items)
    _csr_lib.check(front.lib.mldsa_csr_parse(front.hp._h, _ptr(blob_d), blob_d.numel(), _ptr(items_d), n, _ptr(fields), _ptr(ops), _ptr(status),
                                             _stream(front.device)))
    f, o, s = host(fields), host(ops), host(status)
    assert (f[n * 56:] == CANARY).all() and (o[n * 40:] == CANARY).all() and (s[n:] == CANARY).all()
    return f[:n * 56].view(_csr_lib.FIELDS_DTYPE), o[:n * 40].view(_rec_lib.OP_DTYPE), s[:n]


def run_tbs(front, blob_d, fields, entries, ok, out_len, out_shift=0, split=False):
    """dict(status, reqs, totals, out) from mldsa_csr_tbs (split: from mldsa_csr_tbs_plan then mldsa_csr_tbs_write) into a buffer filled
    with cs.FILL, after checking the canary rows behind each output array and the guard bands around the output buffer"""
    n = len(entries)
    alloc, o, at = placed(np.full(out_len, cs.FILL, dtype=np.uint8), out_shift)
    f, e, k = dev(fields.view(np.uint8)), front.issue_tensor(entries), dev(np.asarray(ok, dtype=np.uint8))
    reqs, status = rows(n, 32), rows(n, 1)
    totals = torch.full((3 + ROWS,), -1, dtype=torch.int64, device="cuda")
    plan = torch.full((front.lib.mldsa_csr_plan_bytes(n),), CANARY, dtype=torch.uint8, device="cuda")
    lib, h, s = front.lib, front.hp._h, _stream(front.device)
    if split:
        _csr_lib.check(lib.mldsa_csr_tbs_plan(h, _ptr(blob_d), blob_d.numel(), _ptr(f), _ptr(e), _ptr(k), n, out_len, _ptr(reqs), _ptr(status),
                                              _ptr(totals), _ptr(plan), plan.numel(), s))
        assert (host(alloc)[at:at + out_len] == cs.FILL).all()  # the plan does not touch the output buffer
        _csr_lib.check(lib.mldsa_csr_tbs_write(h, _ptr(blob_d), blob_d.numel(), _ptr(f), _ptr(e), n, _ptr(o), out_len, _ptr(reqs), _ptr(status), s))
    else:
        _csr_lib.check(lib.mldsa_csr_tbs(h, _ptr(blob_d), blob_d.numel(), _ptr(f), _ptr(e), _ptr(k), n, _ptr(o), out_len, _ptr(reqs), _ptr(status),
                                         _ptr(totals), _ptr(plan), plan.numel(), s))
    q, st, tot, whole = host(reqs), host(status), host(totals), host(alloc)
    assert (q[n * 32:] == CANARY).all() and (st[n:] == CANARY).all() and (tot[3:] == -1).all()
    assert (whole[:at] == CANARY).all() and (whole[at + out_len:] == CANARY).all()
    return dict(status=st[:n], reqs=q[:n * 32].view(_x509sign_lib.REQ_DTYPE), totals=tuple(int(x) for x in tot[:3]), out=whole[at:at + out_len])


def same(what, g, w):
    """two arrays of rows, byte for byte"""
    if g.tobytes() != w.tobytes():
        bad = [i for i in range(len(w)) if g[i].tobytes() != w[i].tobytes()]
        raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], g[bad[0]], w[bad[0]]))


def check_tbs(got, want, out_len):
    same("status", got["status"], want["status"])
    same("reqs", got["reqs"], want["reqs"])
    assert got["totals"] == want["totals"]
    want_out = cs.written(np.full(out_len, cs.FILL, dtype=np.uint8), want)  # every byte; the fill outside the accepted ranges
    if not np.array_equal(got["out"], want_out):
        raise AssertionError("out differs at %s" % np.nonzero(got["out"] != want_out)[0][:8].tolist())


def seam(front, batch, shift=0, out_shift=0, out_len=None, split=False):
    """both stages of a batch against the restatement: stage 1 from the items, stage 2 from the batch's rows, entries and verdicts"""
    _, blob_d, _ = placed(batch["blob"], shift)
    fields, ops, status = run_parse(front, blob_d, batch["items"])
    for what, g, w in zip(("fields", "ops", "parse status"), (fields, ops, status), batch["parse"]):
        same(what, g, w)
    b = (batch["blob"], batch["fields"], batch["entries"], batch["ok"])
    if out_len is None:
        out_len = cs.expected_tbs(*b, 2 ** 62)["totals"][2] or 33  # (nothing accepted: a buffer all the same, to stay untouched)
    want = cs.expected_tbs(*b, out_len)
    got = run_tbs(front, blob_d, batch["fields"], batch["entries"], batch["ok"], out_len, out_shift, split)
    check_tbs(got, want, out_len)
    return got, want


# ------------------------------------------------------------------------------------------------------------------ the seams
@pytest.mark.parametrize("mix", cs.MIXES)
@pytest.mark.parametrize("n", cs.SEAM_SIZES)
def test_both_stages_match_the_restatement_byte_for_byte(front, n, mix):
    k = cs.SEAM_SIZES.index(n)
    batch = cs.seam_case(n, mix, seed=n % 7, front=(0, 5)[k % 2])
    got, want = seam(front, batch, shift=(0, 1, 3, 15)[k % 4], out_shift=(5, 0, 15, 8, 2)[k])
    if mix in ("mod3", "only44", "only87"):
        assert want["totals"][:2] == (n, 0)
    elif mix == "all_defect":
        assert want["totals"] == (0, n, 0) and (got["out"] == cs.FILL).all()
    else:
        assert want["totals"][1] == n // 10
    if n == 65:  # the two entry points on their own give what the one call gives
        seam(front, batch, shift=2, out_shift=9, split=True)


CARRY_N = 64 * 256 + 1  # 65 workgroups of the scan: the one-wave offsets kernel goes round its carry loop a second time
CARRY_AT = (0, 255, 256, 16127, 16128, 16383, 16384)  # the accepted few: both ends of the first and the 64th workgroup, and the 65th


def test_placement_scan_carries_past_64_workgroups(front):
    """stage 2 over 16 385 rows of which seven are accepted; every other one is refused for its verdict (ok = 0: POP), so the blob stays
    seven requests long.  Then the same with one byte too few: the first TBSCertificate that does not fit is the one behind the carry,
    and it corrects the totals."""
    small = cs.seam_case(len(CARRY_AT), "mod3", seed=4, front=1)
    assert not small["parse"][2].any()
    fields = np.zeros(CARRY_N, dtype=small["fields"].dtype)
    entries = np.zeros(CARRY_N, dtype=small["entries"].dtype)
    ok = np.zeros(CARRY_N, dtype=np.uint8)
    entries["set"], entries["serial_len"] = 44, 1
    fields[list(CARRY_AT)], entries[list(CARRY_AT)], ok[list(CARRY_AT)] = small["fields"], small["entries"], 1
    _, blob_d, _ = placed(small["blob"], 3)
    free = cs.expected_tbs(small["blob"], fields, entries, ok, 2 ** 62)
    need = free["totals"][2]
    assert np.nonzero(free["status"] == cs.OK)[0].tolist() == list(CARRY_AT) and (free["status"] == cs.POP).sum() == CARRY_N - len(CARRY_AT)
    assert free["totals"] == (len(CARRY_AT), CARRY_N - len(CARRY_AT), need)
    for out_len in (need, need - 1):
        want = cs.expected_tbs(small["blob"], fields, entries, ok, out_len)
        got = run_tbs(front, blob_d, fields, entries, ok, out_len, out_shift=5)
        check_tbs(got, want, out_len)
    assert np.nonzero(want["status"] == cs.SPACE)[0].tolist() == [CARRY_AT[-1]]
    assert got["totals"] == (len(CARRY_AT) - 1, CARRY_N - len(CARRY_AT) + 1, need)


def test_every_defect_of_both_stages_among_valid_neighbours(front):
    batch, at = cs.defect_batch()
    got, want = seam(front, batch, shift=3, out_shift=1)
    for name, i in ((name, i) for name, three in at.items() for i in three):  # every defect once per parameter set
        assert got["status"][i] == cs.DEFECTS[name], name
        assert got["reqs"][i].tobytes() == bytes(32), name
        for j in (i - 1, i + 1):  # the neighbours are untouched
            assert got["status"][j] == 0 and got["reqs"][j]["set"] in cs.SETS, name


def test_single_byte_mutation_sweep(front):
    batch = cs.mutation_batch()
    assert len(batch["items"]) == 170 * 7
    got, want = seam(front, batch, shift=1, out_shift=3)
    assert set(batch["parse"][2].tolist()) == {cs.OK, cs.DER, cs.VERSION, cs.ALG, cs.KEY, cs.SIG}


@pytest.mark.parametrize("shift", (0, 5))
def test_every_pair_of_alignments(front, shift):
    # allocations are 256-byte aligned and GUARD is a multiple of 16: the generator's `front` is the residue it planned the blob for
    batch = cs.alignment_batch(shift)
    got, want = seam(front, batch, shift=0, out_shift=0)
    assert not got["status"].any()
    pairs = {(int(r["spki_off"]) % 16, (int(q["off"]) + 24 + int(e["serial_len"]) + int(e["issuer_len"]) + int(e["validity_len"]) +
                                       int(r["subject_len"])) % 16) for r, q, e in zip(batch["fields"], got["reqs"], batch["entries"])}
    assert len(pairs) == 256 and {int(e["serial_len"]) for e in batch["entries"]} == set(range(1, 21))


def test_length_edges(front):
    batch, status = cs.edge_batch()
    got, want = seam(front, batch, shift=7, out_shift=11)
    assert got["status"].tolist() == status and sorted(int(q["len"]) for q in got["reqs"])[-3:] == sorted(cs.MAX_TBS.values())


def test_space_rule(front):
    batch = cs.seam_case(65, "tenth_defect", seed=3)
    free = cs.expected_tbs(batch["blob"], batch["fields"], batch["entries"], batch["ok"], 2 ** 62)
    need = free["totals"][2]
    mid = sorted(free["tbs"])[len(free["tbs"]) // 2]
    for out_len in (need, need - 1, int(free["reqs"][mid]["off"]) + 100, 0):
        got, want = seam(front, batch, out_len=out_len, out_shift=out_len % 16)
        assert got["totals"][2] == need and got["totals"][0] + got["totals"][1] == 65
        assert (got["status"] == cs.SPACE).sum() == {need: 0, need - 1: 1, 0: len(free["tbs"])}.get(out_len, len([i for i in free["tbs"] if i >= mid]))
        first = np.nonzero(got["status"] == cs.SPACE)[0]
        if first.size:  # once one request is SPACE, every later accepted one is too
            assert all(got["status"][i] == cs.SPACE for i in free["tbs"] if i >= first[0])


def test_write_does_not_follow_tampered_rows(front):
    """mldsa_csr_tbs_write on rows a caller changed: a request row that points outside the output buffer or whose length is not the
    pieces', a fields row or an entry that points outside the blob, an unknown set, a refused status -- none writes a byte"""
    n = 10
    cases = [cs._case(44, b"tamper", i)[0] for i in range(n)]
    blob, items, entries = cs.lay_out(cases, pad=3)
    fields, _, st1 = cs.expected_parse(blob, items)
    want = cs.expected_tbs(blob, fields, entries, np.ones(n, dtype=np.uint8), 2 ** 62)
    out_len = want["totals"][2]
    assert not st1.any() and not want["status"].any()
    reqs, status, f, e = want["reqs"].copy(), want["status"].copy(), fields.copy(), entries.copy()
    tlen = int(reqs[0]["len"])
    reqs[0]["off"] = out_len - tlen + 1            # ends one byte behind the buffer
    reqs[1]["off"] = 2 ** 64 - 8                   # wraps
    reqs[2]["len"] = int(reqs[2]["len"]) - 1       # not the length of its pieces
    status[3] = cs.POP                             # refused: not written, whatever its rows say
    f[4]["spki_off"] = blob.size - 10              # the SPKI would be read behind the blob
    f[5]["subject_off"] = 2 ** 64 - 4
    e[6]["issuer_off"] = blob.size - 3             # the issuer Name would be read behind the blob
    e[7]["set"] = 66                               # no set: no bytes
    e[8]["serial_len"] = 21
    _, b, _ = placed(blob, 1)
    alloc, o, at = placed(np.full(out_len, cs.FILL, dtype=np.uint8), 5, fill=cs.FILL)
    f_d, e_d, q_d, st_d = dev(f.view(np.uint8)), front.issue_tensor(e), dev(reqs.view(np.uint8)), dev(status)  # (alive until the call is over)
    args = [front.hp._h, _ptr(b), b.numel(), _ptr(f_d), _ptr(e_d), n, _ptr(o), out_len, _ptr(q_d), _ptr(st_d), _stream(front.device)]
    _csr_lib.check(front.lib.mldsa_csr_tbs_write(*args))
    only9 = dict(want, tbs={9: want["tbs"][9]})
    want_alloc = np.full(alloc.numel(), cs.FILL, dtype=np.uint8)
    want_alloc[at:at + out_len] = cs.written(np.full(out_len, cs.FILL, dtype=np.uint8), only9)
    assert np.array_equal(host(alloc), want_alloc)  # request 9 alone
    # and with that one refused too the whole buffer, guard bands included, stays at the fill value
    status[9] = cs.SPACE
    alloc, o, at = placed(np.full(out_len, cs.FILL, dtype=np.uint8), 5, fill=cs.FILL)
    st_d = dev(status)
    args[6], args[9] = _ptr(o), _ptr(st_d)
    _csr_lib.check(front.lib.mldsa_csr_tbs_write(*args))
    assert (host(alloc) == cs.FILL).all()


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("pset", cs.SETS)
def test_five_calls_end_to_end_against_the_oracle(front, sets, hp, pset):
    """a CA key and certificate from the oracle, two requests signed by the oracle, one with a damaged signature: the five calls,
    deterministic; the possessed request's certificate is the restatement's bytes around the oracle's signature and verifies under the
    CA certificate with the names checked; the damaged one is POP and nothing is written for it"""
    s = cs.signed_case(pset)
    _, sk = sets[pset].keygen_from_seed([s["ca_seed"]])
    front.set_keys(pset, sets[pset].private_keys_from_bytes(sk))
    try:
        blob, items, entries = cs.lay_out([(d, len(d), t) for d, t in zip(s["ders"], s["templates"])], pad=[3, 0, 7])
        fields, _, st1 = cs.expected_parse(blob, items)
        want = cs.expected_tbs(blob, fields, entries, [1, 0], 2 ** 62)
        tbs = want["tbs"][0]
        der = xc.cert(tbs, pset, orc.sign_internal(pset, s["ca_sk"], tbs, bytes(32), ctx=b"", mode=orc.MODE_PURE))
        _, b, _ = placed(blob, 1)
        tbs_alloc, tbs_d, tbs_at = placed(np.full(len(tbs) + 9, cs.FILL, dtype=np.uint8), 3)
        out_alloc, out_d, out_at = placed(np.full(len(der) + 9, cs.FILL, dtype=np.uint8), 5)
        sig_status = torch.full((2 + ROWS,), 0x77777777, dtype=torch.int32, device="cuda")
        out_certs, status, issue_status, totals = front.issue_device(b, front.items_tensor(items), front.issue_tensor(entries), tbs_d, out_d,
                                                                     sig_status)
        assert host(status).tolist() == [0, cs.POP] and host(totals).tolist() == [1, 1, len(tbs)]
        assert host(issue_status).tolist() == [0, _x509sign_lib.ENTRY] and host(sig_status).tolist()[:2] == [0, -1]
        want_tbs = np.full(tbs_alloc.numel(), CANARY, dtype=np.uint8)
        want_tbs[tbs_at:tbs_at + len(tbs) + 9] = cs.FILL
        want_tbs[tbs_at:tbs_at + len(tbs)] = np.frombuffer(tbs, dtype=np.uint8)
        assert np.array_equal(host(tbs_alloc), want_tbs)
        want_out = np.full(out_alloc.numel(), CANARY, dtype=np.uint8)
        want_out[out_at:out_at + len(der) + 9] = cs.FILL
        want_out[out_at:out_at + len(der)] = np.frombuffer(der, dtype=np.uint8)
        assert np.array_equal(host(out_alloc), want_out)  # the restatement's bytes around the oracle's signature; nothing for the damaged one
        c = host(out_certs).view(_x509_lib.CERT_DTYPE)
        assert tuple(c[0]) == (0, len(der), 2) and tuple(c[1]) == (0, 0, _x509_lib.NO_ISSUER)
        # the issued certificate, the refused one's empty row and the CA certificate as one batch of the verifying libraries
        ca = np.frombuffer(s["ca_der"], dtype=np.uint8)
        chain = torch.cat([out_d, dev(ca)])
        c = np.concatenate([c, np.array([(out_d.numel(), ca.size, 2)], dtype=_x509_lib.CERT_DTYPE)])
        x5 = MlDsaCertificates(hotpath=hp)
        ok = torch.full((3 + ROWS,), CANARY, dtype=torch.uint8, device="cuda")
        st = x5.verify_device(chain, x5.certs_tensor(c), ok)
        assert host(st).tolist() == [0, _x509_lib.RANGE, 0] and host(ok).tolist() == [1, 0, 1] + [CANARY] * ROWS
        # the subject Name and key the verifying side finds are the request's bytes, the issuer Name the template's
        _, _, vf = x5.ops_device(chain, x5.certs_tensor(c))
        row = host(vf).view(_x509_lib.FIELDS_DTYPE)[0]
        got = host(out_d).tobytes()
        raw = blob.tobytes()
        cut = lambda buf, off, n: buf[int(off):int(off) + int(n)]  # noqa: E731
        assert cut(got, row["subject_off"], row["subject_len"]) == cut(raw, fields[0]["subject_off"], fields[0]["subject_len"])
        assert cut(got, row["key_off"], cs.PK_LEN[s["req_set"]]) == s["pks"][0] and int(row["key_set"]) == s["req_set"]
        assert cut(got, row["issuer_off"], row["issuer_len"]) == s["ca_name"]
    finally:
        front.set_keys(pset, None)


def test_python_front(front, sets):
    s = cs.signed_case(65)
    ok, status = front.verify(s["ders"] + [s["ders"][0][:-1]], pad=[1, 6])
    assert ok.tolist() == [True, False, False] and status.tolist() == [0, 0, cs.DER]
    _, sk = sets[65].keygen_from_seed([s["ca_seed"]])
    front.set_keys(65, sets[65].private_keys_from_bytes(sk))
    try:
        hedged = [t[:6] + (shake(b"csr-front", j),) + t[7:] for j, t in enumerate(s["templates"])]
        certs, st, sst = front.issue(s["ders"], hedged, pad=5)
        assert st.tolist() == [0, cs.POP] and sst.tolist() == [0, -1] and certs[1] is None
        blob, items, entries = cs.lay_out([(d, len(d), t) for d, t in zip(s["ders"], hedged)])
        tbs = cs.expected_tbs(blob, cs.expected_parse(blob, items)[0], entries, [1, 0], 2 ** 62)["tbs"][0]
        assert certs[0] == xc.cert(tbs, 65, orc.sign_internal(65, s["ca_sk"], tbs, hedged[0][6], ctx=b"", mode=orc.MODE_PURE))
        assert front.issue([], [])[0] == [] and front.verify([])[0].size == 0
    finally:
        front.set_keys(65, None)
    blob, items, entries = front.csr_blob(s["ders"], s["templates"], pad=7, front=3)
    assert blob[:10].tolist() == [0xC3] * 10 and int(items[0]["off"]) == 10 and entries.dtype == _csr_lib.ISSUE_DTYPE
    assert int(entries[0]["issuer_off"]) == int(entries[1]["issuer_off"]) and int(entries[0]["serial_off"]) != int(entries[1]["serial_off"])
