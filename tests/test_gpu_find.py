"""The path-building library on the device (include/mldsa_find.h): mldsa_find_ids, mldsa_find_table, mldsa_find_issuers, mldsa_find_build,
mldsa_find_crl_issuers and mldsa_find_cert_crls byte for byte against the restatement of tests/find_cases.py -- batch sizes around the
wave and the workgroup, every blob alignment, Names at the edges of the 64-byte compare step, every rule of the two identifiers, the
matching rules, a flood of one Name, forced hash collisions up to a table that runs over, tampered rows, CRLs -- and whole signed chains
through MlDsaPathValidator.validate with no issuer arrays against the same call with the arrays."""
import calendar

from gpu_common import *  # noqa: F401,F403

import crl_cases as cc
import find_cases as fc
import path_cases as pc
import x509_cases as xc
from fips204_amd import _crl_lib, _find_lib, _lib, _path_lib, _x509_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MlDsaPathBuilder, MlDsaPathValidator

pytestmark = pytest.mark.gpu

CANARY = 0x77
SEED = bytes(range(16))


@pytest.fixture(scope="module")
def pb(hp):
    return MlDsaPathBuilder(hotpath=hp, seed=SEED)


def blob_dev(blob, shift=0):
    """the blob on the device between canary bytes, `shift` bytes into its (256-byte aligned) allocation"""
    t = torch.full((blob.size + shift + 1,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + blob.size] = torch.from_numpy(blob.copy())
    return t, t[shift:shift + blob.size]


def rows_dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).cuda()


def differ(got, want, what):
    if not np.array_equal(got, want):
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        raise AssertionError("%s differ at %s: got %s, want %s" % (what, bad[:5], got[bad[0]], want[bad[0]]))


def lay_out(ders, pad=None, lens=None):
    blob, certs = xc.lay_out([(d, len(d) if lens is None else lens[i]) for i, d in enumerate(ders)], [None] * len(ders),
                             pad=list(range(16)) if pad is None else pad)
    return blob[:-1], certs


def run(pb, blob, certs, shift=0, hash_bits=64, seed=SEED, use_ids=True, tamper=None, in_group=None):
    """ids, table and issuers as three calls on rows the device wrote (changed by `tamper` on the way), each compared with the restatement
    run on the same rows.  Returns the host arrays by name."""
    n = len(certs)
    whole, b = blob_dev(blob, shift)
    assert (b.data_ptr() - shift) % 256 == 0
    d_certs = rows_dev(certs)
    fields, policy = pb.parse_device(b, d_certs)
    fields_h, policy_h = host(fields).view(_x509_lib.FIELDS_DTYPE).copy(), host(policy).view(_path_lib.FIELDS_DTYPE).copy()
    builder = MlDsaPathBuilder(hotpath=pb.hp, seed=seed, hash_bits=hash_bits)
    if tamper is not None and tamper.__code__.co_argcount == 3:
        tamper(certs, fields_h, policy_h)
        d_certs, fields, policy = rows_dev(certs), rows_dev(fields_h), rows_dev(policy_h)
    ids = builder.ids_device(b, d_certs, policy if use_ids else None)
    ids_h = host(ids).view(_find_lib.ID_DTYPE).copy()
    differ(ids_h, fc.expected_ids(blob, certs, policy_h if use_ids else None), "ids")
    if tamper is not None and tamper.__code__.co_argcount == 1:
        tamper(ids_h)
        ids = rows_dev(ids_h)
    totals, scratch = builder.table_device(b, d_certs, fields, ids)
    certs_out, results = builder.issuers_device(b, d_certs, fields, ids, totals, scratch)
    res, out = host(results).view(_find_lib.RESULT_DTYPE), host(certs_out).view(_x509_lib.CERT_DTYPE)
    want_res, want_out = fc.expected_issuers(blob, certs, fields_h, ids_h, in_group)
    differ(res, want_res, "results")
    differ(out, want_out, "certs_out")
    tot = host(totals).view(_find_lib.TOTALS_DTYPE)[0]
    table = fc.candidates(blob, certs, fields_h, ids_h)
    n_cand = len({j for js in table.values() for j in js})
    assert (int(tot["candidates"]), int(tot["keys"])) == (n_cand, 2 * n_cand) and 0 <= int(tot["slots"]) <= 2 * n_cand
    if hash_bits == 64:
        assert int(tot["overflow"]) == 0 and int(tot["slots"]) == len(table)  # one slot per distinct key, a 64-bit collision aside
    w = host(whole)
    assert (w[:shift] == CANARY).all() and w[-1] == CANARY and np.array_equal(w[shift:shift + blob.size], blob)
    return dict(res=res, out=out, ids=ids_h, fields=fields_h, policy=policy_h, totals=tot, n=n, dev=dict(
        blob=b, certs=d_certs, fields=fields, policy=policy, ids=ids, totals=totals, scratch=scratch, certs_out=certs_out, builder=builder))


# ------------------------------------------------------------------------------------------------------------------ sizes, alignments
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_shuffled_chains_match_the_restatement_byte_for_byte(pb, n):
    ders, issuers = fc.shuffled_chains(n, seed=n)
    blob, certs = lay_out(ders)
    got = run(pb, blob, certs, shift=n % 16)
    assert (got["res"]["status"] == fc.FOUND).all()
    # where only one certificate matches it is the one that the chain was built with
    one = got["res"]["candidates"] == 1
    assert one.sum() >= n // 2 and np.array_equal(got["res"]["issuer"][one], np.array(issuers, dtype=np.uint32)[one])
    # by Name alone: the same issuers wherever the Name is one certificate's
    by_name = run(pb, blob, certs, shift=n % 16, use_ids=False)
    one = by_name["res"]["candidates"] == 1
    assert not by_name["ids"]["ski_len"].any() and one.sum() >= n // 2 and np.array_equal(by_name["res"]["issuer"][one], got["res"]["issuer"][one])


def test_every_start_alignment_of_the_blob(pb):
    ders, issuers = fc.shuffled_chains(9, seed=77)
    for shift in range(16):
        blob, certs = lay_out(ders, pad=[shift, 3, 0])
        got = run(pb, blob, certs, shift=shift)
        assert got["res"]["issuer"].tolist() == issuers, shift


def test_build_is_the_three_calls_writes_nothing_else_and_may_alias(pb):
    n = 65
    ders, _ = fc.shuffled_chains(n, seed=5)
    blob, certs = lay_out(ders)
    got = run(pb, blob, certs, shift=3)
    d = got["dev"]
    need = pb.lib.mldsa_find_scratch_bytes(n)
    ids, totals, results = (torch.full((size + 48,), CANARY, dtype=torch.uint8, device="cuda") for size in (n * 24, 16, n * 12))
    certs_io = torch.cat([d["certs"], torch.full((48,), CANARY, dtype=torch.uint8, device="cuda")])
    scratch = torch.full((need + 256,), CANARY, dtype=torch.uint8, device="cuda")
    call = lambda size: pb.lib.mldsa_find_build(pb.hp._h, _ptr(d["blob"]), d["blob"].numel(), _ptr(certs_io), _ptr(d["fields"]), _ptr(d["policy"]), n,  # noqa: E731
                                                SEED, 64, _ptr(ids), _ptr(totals), _ptr(certs_io), _ptr(results), _ptr(scratch), size, _stream(pb.device))
    assert call(need - 1) == _lib.ERR_PARAM and b"smaller than mldsa_find_scratch_bytes" in pb.lib.mldsa_find_last_error()
    assert all((host(t) == CANARY).all() for t in (ids, totals, results, scratch))
    _find_lib.check(call(need))
    differ(host(ids)[:n * 24].view(_find_lib.ID_DTYPE), got["ids"], "ids")
    differ(host(results)[:n * 12].view(_find_lib.RESULT_DTYPE), got["res"], "results")
    differ(host(certs_io)[:n * 16].view(_x509_lib.CERT_DTYPE), got["out"], "certs_out in place")
    differ(host(totals)[:16].view(_find_lib.TOTALS_DTYPE), host(d["totals"]).view(_find_lib.TOTALS_DTYPE), "totals")
    for t, size in ((ids, n * 24), (totals, 16), (results, n * 12), (certs_io, n * 16), (scratch, need)):
        assert (host(t)[size:] == CANARY).all()
    # the Python front, and the calls behind it run on certs_out unchanged
    found = pb.build_device(d["blob"], d["certs"])
    differ(host(found["results"]).view(_find_lib.RESULT_DTYPE), got["res"], "results")
    issuers, candidates, cert_crl, details = pb.build(ders, pad=list(range(16)))
    assert np.array_equal(issuers, got["res"]["issuer"]) and np.array_equal(candidates, got["res"]["candidates"]) and (cert_crl == fc.CRL_NONE).all()
    assert pb.build([])[0].size == 0


# ------------------------------------------------------------------------------------------------------------------ Names, identifiers
def test_name_lengths_at_the_edges_of_the_compare_step_and_of_the_length_forms(pb):
    ders, want = [], []
    for k, length in enumerate(fc.NAME_LENGTHS):
        nm = fc.name_of_len(length, b"edge%d" % k)
        ders.append(fc.cert(44, 44, nm, nm, b"nl", 3 * k))  # a root
        want.append(len(ders) - 1)
        if length > 2:
            last = nm[:-1] + bytes([nm[-1] ^ 0x01])  # the same but for the last byte: another root, and a leaf under each
            ders.append(fc.cert(44, 44, last, last, b"nl", 3 * k + 1))
            want.append(len(ders) - 1)
            ders += [fc.cert(44, 0, nm, xc.name(b"leaf"), b"nl", 3 * k + 2), fc.cert(44, 0, last, xc.name(b"leaf"), b"nl", 3 * k + 2)]
            want += [len(ders) - 4, len(ders) - 3]
    # Names that differ in length alone: one is the other's beginning, as bytes
    short, long_ = fc.name_of_len(64, b"q"), fc.name_of_len(65, b"q")
    assert long_[4:-1] != short[4:] and len(short) + 1 == len(long_)
    ders += [fc.cert(44, 44, short, short, b"nl", 90), fc.cert(44, 44, long_, long_, b"nl", 91), fc.cert(44, 0, long_, xc.name(b"leaf"), b"nl", 92)]
    want += [len(ders) - 3, len(ders) - 2, len(ders) - 2]
    blob, certs = lay_out(ders)
    got = run(pb, blob, certs, shift=7)
    assert got["res"]["issuer"].tolist() == want and (got["res"]["candidates"] == 1).all()
    assert sorted(set(got["fields"]["subject_len"].tolist()) - {xc.walk(ders[-1])["subject_len"]}) == sorted(fc.NAME_LENGTHS)


def test_identifier_lengths_and_the_members_of_the_aki(pb):
    nm = xc.name(b"one name for all")
    ders, want = [], []
    for k, length in enumerate((1, 20, 32, 64)):
        kid = bytes([0x50 + k]) * length
        ders.append(fc.cert(44, 44, nm, nm, b"il", 4 * k, [fc.ski_ext(kid), fc.aki_ext(kid)]))
        ders.append(fc.cert(44, 0, nm, xc.name(b"leaf"), b"il", 4 * k + 1, [fc.aki_ext(kid, nm, b"\x05")]))       # A1 and 82 behind the identifier
        ders.append(fc.cert(44, 0, nm, xc.name(b"leaf"), b"il", 4 * k + 2, [fc.aki_ext(kid[:-1] + b"\x00")]))      # another last byte
        ders.append(fc.cert(44, 0, nm, xc.name(b"leaf"), b"il", 4 * k + 3, [fc.aki_ext(None, nm, b"\x05")]))       # no identifier: by Name
        want += [(4 * k, 1), (4 * k, 1), (fc.NO_ISSUER, 0), (0, 4)]
    ders.append(fc.cert(44, 44, nm, nm, b"il", 90, [fc.ski_ext(bytes(65))]))   # refused with EXT: it takes no part
    ders.append(fc.cert(44, 0, nm, nm, b"il", 91, [fc.aki_ext(bytes(65))]))
    want += [(fc.NO_ISSUER, 0), (fc.NO_ISSUER, 0)]
    blob, certs = lay_out(ders)
    got = run(pb, blob, certs, shift=1)
    assert list(zip(got["res"]["issuer"].tolist(), got["res"]["candidates"].tolist())) == want
    assert got["ids"]["status"].tolist() == [0] * 16 + [fc.EXT] * 2 and got["res"]["status"].tolist()[-2:] == [fc.CERT, fc.CERT]
    assert got["ids"]["ski_len"][0::4][:4].tolist() == [1, 20, 32, 64] and got["ids"]["aki_len"][1::4][:4].tolist() == [1, 20, 32, 64]


def test_every_defect_class_of_the_two_values_and_a_mutation_sweep(pb):
    nm = xc.name(b"defects")
    cases = fc.value_cases()
    ders = [fc.cert(44, 44, nm, nm, b"vc", i, tail=xc.tlv(0xA3, xc.tlv(0x30, content))) for i, (content, _) in enumerate(cases)]
    # one certificate's extensions with every byte set to each of the mutation values
    base_exts = pc.basic() + fc.ski_ext(fc.KID) + fc.aki_ext(fc.KID, nm, b"\x12\x34")
    base = fc.cert(44, 44, nm, nm, b"vc", 999, tail=xc.tlv(0xA3, xc.tlv(0x30, base_exts)))
    at = base.index(base_exts)
    for pos in range(at - 4, at + len(base_exts)):
        ders += [base[:pos] + bytes([v]) + base[pos + 1:] for v in xc.MUTATION_VALUES]
    blob, certs = lay_out(ders, pad=[5, 0, 11])
    got = run(pb, blob, certs, shift=2)
    walked = [(i, want) for i, (content, want) in enumerate(cases) if content and got["policy"][i]["status"] not in (pc.RANGE, pc.DER)]
    assert len(walked) > 40
    for i, want in walked:  # the frames that mldsa_path_parse refuses as DER never get here; the others give the documented status
        assert got["ids"][i]["status"] == want, (i, cases[i][0].hex())
    # (a frame that walk_ids would call DER is DER for mldsa_path_parse too, whose row is then not followed: the tampered rows below get there)
    assert set(got["ids"]["status"].tolist()) == {fc.OK, fc.EXT} and set(got["res"]["status"].tolist()) >= {fc.FOUND, fc.CERT}


# ------------------------------------------------------------------------------------------------------------------ matching
def test_the_matching_rules(pb):
    root, other_root, ca = xc.name(b"root"), xc.name(b"rooT"), xc.name(b"ca")
    x, y = xc.name(b"cross x"), xc.name(b"cross y")
    k1, k2 = bytes([1] * 20), bytes([2] * 20)
    ders = [fc.cert(44, 44, root, root, b"t", 0, [fc.ski_ext(k1), fc.aki_ext(k1)]),      # 0 a self-signed root
            fc.cert(44, 44, root, root, b"t", 1, [fc.ski_ext(k2)]),                      # 1 the same Name, rolled over to another key
            fc.cert(44, 44, root, ca, b"t", 2, [fc.aki_ext(k2)]),                        # 2 issued under the new key
            fc.cert(44, 44, root, ca, b"t", 3),                                          # 3 no AKI: the lowest of the Name
            fc.cert(65, 44, root, ca, b"t", 4),                                          # 4 signed with another parameter set
            fc.cert(44, 44, other_root, ca, b"t", 5),                                    # 5 a Name that differs in its last byte
            fc.cert(44, 0, ca, xc.name(b"leaf"), b"t", 6, [fc.aki_ext(k1)]),             # 6 under 2 ... 5, which carry no SKI
            fc.cert(44, 44, root, root, b"t", 7, [fc.aki_ext(k2)]),                      # 7 self-issued, its AKI is not its own SKI
            fc.cert(87, 87, y, x, b"t", 8), fc.cert(87, 87, x, y, b"t", 9),              # 8, 9 a cross-signed pair
            fc.cert(65, 65, xc.name(b"r65"), xc.name(b"r65"), b"t", 10)]                 # 10 a root of the set that 4 is signed with, another Name
    blob, certs = lay_out(ders, pad=[5, 0, 11])
    got = run(pb, blob, certs)
    assert got["res"]["status"].tolist() == [0, 0, 0, 0, fc.NONE, fc.NONE, 0, 0, 0, 0, 0]
    assert got["res"]["issuer"].tolist() == [0, 0, 1, 0, fc.NO_ISSUER, fc.NO_ISSUER, 2, 1, 9, 8, 10]
    assert got["res"]["candidates"].tolist() == [2, 3, 2, 3, 0, 0, 4, 2, 1, 1, 1]
    # key rollover alone: with the rolled-over root carrying an SKI and no third certificate of the Name, the AKI picks exactly one
    got = run(pb, *lay_out(ders[:3] + ders[3:4]))
    assert got["res"]["issuer"].tolist() == [0, 0, 1, 0] and got["res"]["candidates"].tolist() == [1, 2, 1, 2]


def test_defective_issuers_and_certificates_whose_own_row_is_not_ok(pb):
    nms = [xc.name(b"issuer %d" % k) for k in range(6)]
    good = [fc.cert(44, 44, nms[k], nms[k], b"d", k) for k in range(6)]
    roots = [good[0], xc.make_defect(good[1], "alg_sets_differ")[0], xc.make_defect(good[2], "sig_unused_bits")[0],
             xc.make_defect(good[3], "wrong_tag_validity")[0], good[4], good[5]]
    leaves = [fc.cert(44, 0, nms[k], xc.name(b"leaf %d" % k), b"d", 10 + k) for k in range(6)]
    ders = roots + leaves
    lens = [len(d) for d in ders]
    lens[4] = 2 ** 32 - 1  # RANGE
    blob, certs = lay_out(ders, lens=lens)
    got = run(pb, blob, certs)
    st = got["fields"]["status"].tolist()
    assert st[:6] == [0, xc.ALG, xc.SIG, xc.DER, xc.RANGE, 0]
    # roots: ALG, SIG, DER and RANGE rows are no seekers; leaves: the ALG and SIG roots still lend their keys, the DER and RANGE ones do not
    assert got["res"]["status"].tolist() == [0, fc.CERT, fc.CERT, fc.CERT, fc.CERT, 0, 0, 0, 0, fc.NONE, fc.NONE, 0]
    assert got["res"]["issuer"].tolist()[6:] == [0, 1, 2, fc.NO_ISSUER, fc.NO_ISSUER, 5]


def test_a_flood_of_one_subject_name(pb):
    n = 1000
    nm = xc.name(b"everybody")
    kid = lambda i: xc._bytes(b"flood", i, 20)  # noqa: E731
    ders = [fc.cert(44, 44, nm, nm, b"fl", i, [fc.ski_ext(kid(i))] + ([fc.aki_ext(kid((7 * i + 3) % n))] if i % 4 else [])) for i in range(n)]
    blob, certs = lay_out(ders)
    got = run(pb, blob, certs)
    res = got["res"]
    assert (res["status"] == fc.FOUND).all()
    assert all(int(r["issuer"]) == ((7 * i + 3) % n if i % 4 else 0) and int(r["candidates"]) == (1 if i % 4 else n) for i, r in enumerate(res))
    assert int(got["totals"]["slots"]) == n + 1 and int(got["totals"]["overflow"]) == 0  # one ANY key, n SKI keys


# ------------------------------------------------------------------------------------------------------------------ collisions
def test_forced_collisions_change_nothing(pb):
    ders, _ = fc.shuffled_chains(300, seed=300)
    blob, certs = lay_out(ders)
    base = run(pb, blob, certs)
    for bits, seed in ((1, SEED), (2, SEED), (4, SEED), (64, bytes(16)), (4, bytes([0xA5] * 16))):
        got = run(pb, blob, certs, hash_bits=bits, seed=seed)
        differ(got["res"], base["res"], "results at %d bits" % bits)
        differ(got["out"], base["out"], "certs_out at %d bits" % bits)
        assert int(got["totals"]["overflow"]) <= fc.OVERFLOW_MAX and int(got["totals"]["slots"]) <= 2 ** min(bits, 12)
        if bits < 64:
            assert int(got["totals"]["overflow"]) >= 600 - 2 * 2 ** bits * 3  # nearly every key lost its slot to another


def test_a_table_that_runs_over_answers_space_and_nothing_wrong(pb):
    n = 2000
    root = xc.name(b"the first entry")
    ders = [fc.cert(44, 44, root, root, b"ov", 0)]
    for i in range(1, n):
        issuer = root if i % 5 == 0 else xc.name(b"absent %d" % i)  # nobody carries these Names
        ders.append(fc.cert(44, 44, issuer, xc.name(b"subject %d" % i), b"ov", i))
    lens = [len(d) for d in ders]
    lens[7] -= 1  # a DER row: CERT
    blob, certs = lay_out(ders, lens=lens)
    first = (fc.ANY, 44, root, b"")  # entry 0 owns its slot whatever the hash: the lowest index of its tag
    got = run(pb, blob, certs, hash_bits=1, in_group={first})
    assert int(got["totals"]["overflow"]) > fc.OVERFLOW_MAX and int(got["totals"]["slots"]) <= 2
    want = [fc.CERT if i == 7 else fc.FOUND if i % 5 == 0 else fc.SPACE for i in range(n)]
    assert got["res"]["status"].tolist() == want and (got["res"]["issuer"][::5] == 0).all() and (got["res"]["candidates"][::5] == 1).all()
    # the same batch with the whole hash: nothing runs over, the absent issuers are NONE
    got = run(pb, blob, certs)
    assert got["res"]["status"].tolist() == [fc.NONE if w == fc.SPACE else w for w in want]


# ------------------------------------------------------------------------------------------------------------------ tampered rows
def test_ranges_that_point_outside_the_certificate_are_not_followed(pb):
    ders, _ = fc.shuffled_chains(24, seed=24)
    blob, certs = lay_out(ders)
    end = blob.size

    def rows(c, f, p):
        f[1]["subject_off"] = int(c[1]["off"]) - 1            # begins in front of its certificate
        f[2]["subject_len"] = int(c[2]["len"]) + 1            # ends behind it
        f[3]["issuer_off"] = int(c[4]["off"])                 # lies in a neighbour
        f[5]["issuer_off"], f[5]["issuer_len"] = end - 1, 2   # ends behind the blob
        f[6]["subject_off"] = 2 ** 64 - 1
        p[7]["ext_off"] = int(c[7]["off"]) + int(c[7]["len"]) - 1  # the extensions end behind the certificate (where it has any)
        p[8]["ext_off"], p[8]["ext_len"] = 2 ** 64 - 4, 8
        c[9]["off"], c[10]["len"] = end, 2 ** 32 - 1           # the certificate itself outside the blob
        assert p[11]["ext_len"] > 8
        p[11]["ext_off"] += 1                                  # inside the certificate, but no extension begins there
        p[11]["ext_len"] -= 1

    got = run(pb, blob, certs.copy(), shift=5, tamper=rows)
    assert got["res"]["status"][3] == got["res"]["status"][5] == fc.CERT
    assert got["ids"]["status"][7:12].tolist() == [fc.RANGE, fc.RANGE, fc.RANGE, fc.RANGE, fc.DER]

    def identifiers(d):
        has_ski, has_aki = [i for i in range(24) if d[i]["ski_len"]], [i for i in range(24) if d[i]["aki_len"]]
        d[has_ski[0]]["ski_off"] = end - 1
        d[has_ski[1]]["ski_len"] = 65
        d[has_ski[2]]["ski_off"] = 0
        d[has_aki[0]]["aki_off"] = 2 ** 64 - 8
        d[has_aki[1]]["aki_len"] = 200
        d[has_aki[2]]["status"] = fc.DER

    got = run(pb, blob, certs.copy(), shift=5, tamper=identifiers)
    assert (got["res"]["status"] == fc.CERT).sum() >= 3


# ------------------------------------------------------------------------------------------------------------------ CRLs
@pytest.mark.parametrize("n_crls", [1, 2, 65])
def test_crl_issuers_and_the_crl_of_every_certificate(pb, n_crls):
    ders, _ = fc.shuffled_chains(40, seed=40 + n_crls)
    blob_c, certs = lay_out(ders)
    fields, _, _ = xc.expected(blob_c, certs)
    ids0 = fc.expected_ids(blob_c, certs, pc.expected_parse(blob_c, certs))
    named = set(fc.expected_issuers(blob_c, certs, fields, ids0)[0]["issuer"].tolist())  # the CRLs' CAs are certificates that issued something
    cas = [j for j in range(40) if fields[j]["subject_len"] > 2 and j in named]
    raw = blob_c.tobytes()
    crls = []
    for c in range(n_crls):
        j = cas[(c // 2) % len(cas)] if n_crls > 1 else cas[0]  # two CRLs of every CA, in turn
        nm = raw[int(fields[j]["subject_off"]):int(fields[j]["subject_off"]) + int(fields[j]["subject_len"])]
        kid = raw[int(ids0[j]["ski_off"]):int(ids0[j]["ski_off"]) + int(ids0[j]["ski_len"])]
        ext = (fc.aki_ext(kid) if kid and c % 3 == 0 else b"") + cc.crl_number()
        crls.append(fc.crl(int(fields[j]["key_set"]), nm, b"crl%d" % n_crls, c, ext=None if c % 7 == 6 else ext))
    if n_crls > 2:
        crls[-1] = fc.crl(44, xc.name(b"an issuer nobody has"), b"crl", 0)
    if n_crls == 65:
        crls[10] = fc.crl(44, xc.name(b"x"), b"crl", 1, ext=fc.aki_ext(bytes(65)))  # an AKI that is refused: no seeker
        crls[11] = crls[11][:-1]                                                      # DER
    blob, rows = xc.lay_out([(d, len(d)) for d in ders + crls], [None] * (40 + n_crls), pad=list(range(16)))
    blob, certs, items = blob[:-1], rows[:40], rows[40:].astype(_crl_lib.ITEM_DTYPE)
    got = run(pb, blob, certs, shift=9)
    d = got["dev"]
    d_items = rows_dev(items)
    crl_fields = d["builder"].crl_parse_device(d["blob"], d_items)
    crl_fields_h = host(crl_fields).view(_crl_lib.FIELDS_DTYPE)
    found = dict(certs=d["certs"], fields=d["fields"], ids=d["ids"], totals=d["totals"], scratch=d["scratch"])
    items_out, results = d["builder"].crl_issuers_device(d["blob"], d_items, crl_fields, found)
    want_res, want_items = fc.expected_crl_issuers(blob, items, crl_fields_h, certs, got["fields"], got["ids"])
    differ(host(results).view(_find_lib.RESULT_DTYPE), want_res, "crl results")
    differ(host(items_out).view(_crl_lib.ITEM_DTYPE), want_items, "crls_out")
    assert want_res["status"][0] == fc.FOUND and (n_crls <= 2 or want_res["status"][-1] == fc.NONE)
    if n_crls == 65:
        assert want_res["status"][10] == want_res["status"][11] == fc.CERT and (want_res["status"] == fc.FOUND).sum() >= 60
    cert_crl = d["builder"].cert_crls_device(d["certs_out"], items_out, d["scratch"])
    want_cover = fc.expected_cert_crls(got["out"]["issuer"], want_items["issuer"])
    differ(host(cert_crl).view(np.uint32), want_cover, "cert_crl")
    assert (want_cover != fc.CRL_NONE).any() and (want_cover == fc.CRL_NONE).any()
    if n_crls > 1:  # two CRLs of one CA: the lower index
        assert want_items["issuer"][0] == want_items["issuer"][1] and 1 not in want_cover.tolist() and 0 in want_cover.tolist()
    # the table is as it was: the same lookups give the same answers afterwards
    again, _ = d["builder"].issuers_device(d["blob"], d["certs"], d["fields"], d["ids"], d["totals"], d["scratch"])
    differ(host(again).view(_x509_lib.CERT_DTYPE), got["out"], "certs_out behind mldsa_find_cert_crls")
    # without CRLs nobody is covered
    none = d["builder"].cert_crls_device(d["certs_out"], None, d["scratch"])
    assert (host(none).view(np.uint32) == fc.CRL_NONE).all()


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_validate_without_issuer_arrays_is_validate_with_them(hp):
    pv = MlDsaPathValidator(hotpath=hp)
    tag = b"find-e2e"
    psets = (44, 65, 87)
    ders, issuers = xc.signed_chain(psets, tag)
    root_key = orc.keygen_from_seed(44, xc._bytes(tag + b"xi", 0, 32))
    p = cc.parts(44, tag + b"-0", [cc.entry(b"\x7f")], bytes(xc.SIG_LEN[44]))
    p.update(this=pc.utc(2025, 6, 1), next=pc.utc(2025, 7, 1))
    p["sig_bits"] = b"\x00" + orc.sign_internal(44, root_key[1], cc.tbs_of(p), xc._bytes(tag + b"crl", 0, 32), ctx=b"", mode=orc.MODE_PURE)
    crl = cc.join(p)
    now = calendar.timegm((2025, 6, 15, 0, 0, 0))
    for perm in ([2, 0, 1], [1, 2, 0], [0, 1, 2]):  # position q holds certificate perm[q]
        where = {c: q for q, c in enumerate(perm)}
        shuffled = [ders[c] for c in perm]
        named = [where[issuers[c]] for c in perm]
        cover = [0 if named[q] == where[0] else None for q in range(3)]
        for flip in (None, 1):
            batch = list(shuffled)
            if flip is not None:
                q = where[flip]
                batch[q] = batch[q][:-9] + bytes([batch[q][-9] ^ 0x04]) + batch[q][-8:]
            kw = dict(crl_ders=[crl], pad=[3, 0, 9], allow_no_crl=True)
            v0, w0, d0, det0 = pv.validate(batch, named, [where[0]], now, crl_issuers=[where[0]], cert_crl=cover, **kw)
            v1, w1, d1, det1 = pv.validate(batch, None, [where[0]], now, crl_issuers=None, cert_crl=None, **kw)
            assert (v1.tolist(), w1.tolist(), d1.tolist()) == (v0.tolist(), w0.tolist(), d0.tolist()), (perm, flip)
            assert det1["issuers"].tolist() == named and det1["candidates"].tolist() == [1, 1, 1] and det1["crl_issuers"].tolist() == [where[0]]
            assert det1["cert_crl"].tolist() == [fc.CRL_NONE if c is None else c for c in cover]
            for name in ("cert_ok", "cert_status", "revocation", "crl_ok", "crl_status", "fresh_ok"):
                assert np.array_equal(det0[name], det1[name]), name
            # the oracle's verdicts on the signatures, after undoing the permutation
            oracle_ok = []
            for c in range(3):
                der, up = batch[where[c]], xc.walk(batch[where[issuers[c]]])
                w = xc.walk(der)
                pk = batch[where[issuers[c]]][up["key_off"]:up["key_off"] + xc.PK_LEN[psets[issuers[c]]]]
                sig_set = psets[issuers[c]]
                oracle_ok.append(int(bool(orc.verify_internal(sig_set, orc.pk_try_from_bytes(sig_set, pk), der[w["tbs_off"]:w["tbs_off"] + w["tbs_len"]],
                                                              der[w["sig_off"]:w["sig_off"] + xc.SIG_LEN[sig_set]], ctx=b"", mode=orc.MODE_PURE))))
            assert [int(det1["cert_ok"][where[c]]) for c in range(3)] == oracle_ok == [1, 0 if flip == 1 else 1, 1], (perm, flip)
            assert det1["crl_ok"].tolist() == [1] and det1["revocation"].tolist() == [_crl_lib.GOOD if c == 0 else _crl_lib.NO_CRL for c in
                                                                                     [0 if x is not None else 1 for x in cover]]
    # cert_issuers given and the CRL's issuer found; and a batch without CRLs
    kw = dict(crl_ders=[crl], pad=[3, 0, 9], allow_no_crl=True)
    v0, w0, d0, det0 = pv.validate(shuffled, named, [where[0]], now, crl_issuers=[where[0]], cert_crl=cover, **kw)
    v2, w2, d2, det2 = pv.validate(shuffled, named, [where[0]], now, crl_issuers=None, cert_crl=cover, **kw)
    assert (v2.tolist(), w2.tolist(), d2.tolist()) == (v0.tolist(), w0.tolist(), d0.tolist())
    assert np.array_equal(det2["revocation"], det0["revocation"]) and np.array_equal(det2["crl_status"], det0["crl_status"])
    assert det2["crl_issuers"].tolist() == [where[0]] and "cert_crl" not in det2
    v3, _, _, det3 = pv.validate(shuffled, None, [where[0]], now)
    v4, _, _, _ = pv.validate(shuffled, named, [where[0]], now)
    assert v3.tolist() == v4.tolist() and det3["issuers"].tolist() == named
