"""The wire-record library on the device (include/mldsa_rec.h): the seam -- mldsa_rec_plan and mldsa_rec_pack -- byte for byte against the
numpy restatement of tests/rec_cases.py, refusals of single ops, mldsa_rec_verify against mldsa_verify_pk per parameter set on arrays
packed on the host and against the oracle, the scratch sizes, stream order, and the Python front."""
from gpu_common import *  # noqa: F401,F403

import rec_cases as rc
from fips204_amd import _lib, _rec_lib
from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PREHASH, MODE_PURE, MlDsaRecords, hash_message, records_blob

pytestmark = pytest.mark.gpu

CANARY = 0x77


@pytest.fixture(scope="module")
def recs(hp):
    return MlDsaRecords(hotpath=hp)


def blob_dev(blob, shift=0):
    """the blob on the device, `shift` bytes into its allocation (so its address is that far from 256-byte alignment)"""
    t = torch.full((blob.size + shift + 1,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + blob.size] = torch.from_numpy(blob.copy())
    return t[shift:shift + blob.size]


def signed(sets, n, mode, tag, n_keys=4):
    """n valid records (pset, pk, message, sig, ctx) signed on the device, sets dealt i mod 3, n_keys keys per set dealt round-robin,
    message and context lengths cycling through rc.MSG_LENS and rc.CTX_LENS"""
    out = [None] * n
    for c, pset in enumerate(rc.SETS):
        idx = list(range(c, n, 3))
        if not idx:
            continue
        m = sets[pset]
        pk, sk = m.keygen_from_seed([shake(tag + b"key%d" % pset, j) for j in range(n_keys)])
        pk_h = host(pk)
        msgs = [shake(tag + b"msg", i, rc.MSG_LENS[(i // 3) % len(rc.MSG_LENS)]) for i in idx]
        if mode == MODE_PREHASH:
            msgs = [hash_message(x, "SHA256") for x in msgs]
        ctxs = [shake(tag + b"ctx", i, rc.CTX_LENS[(i // 3) % len(rc.CTX_LENS)]) for i in idx]
        kidx = np.arange(len(idx), dtype=np.uint32) % n_keys
        sig = host(m.try_sign_with_seed(m.private_keys_from_bytes(sk), msgs, [shake(tag + b"rnd", i) for i in idx], ctxs=ctxs, key_idx=kidx,
                                        mode=mode))
        for j, i in enumerate(idx):
            out[i] = (pset, pk_h[kidx[j]].tobytes(), msgs[j], sig[j].tobytes(), ctxs[j])
    return out


@pytest.fixture(scope="module")
def pool(sets):
    """signed records, made once: 1 100 in pure mode, 65 in each of the other two"""
    return {MODE_PURE: signed(sets, 1100, MODE_PURE, b"rec-pure"), MODE_INTERNAL: signed(sets, 65, MODE_INTERNAL, b"rec-int"),
            MODE_PREHASH: signed(sets, 65, MODE_PREHASH, b"rec-ph")}


def reference_ok(sets, blob, ops, mode):
    """one verdict per op from mldsa_verify_pk per parameter set on the arrays the restatement packs on the host; 0 for a refused op"""
    want = rc.expected(blob, ops)
    per_class = {}
    for c, pset in enumerate(rc.SETS):
        r = rc.records_of(want["packed"][pset])
        if r:
            per_class[c] = sets[pset].verify_pk([x[0] for x in r], [x[1] for x in r], [x[2] for x in r], ctxs=[x[3] for x in r], mode=mode)
    cs = want["class_slot"]
    return np.array([bool(per_class[int(w) >> 30][int(w) & 0x3FFFFFFF]) if int(w) >> 30 != 3 else False for w in cs], dtype=bool), want


def run_verify(recs, blob, ops, mode=MODE_PURE, shift=0, scratch=None, info=None):
    ok = torch.full((len(ops) + 64,), CANARY, dtype=torch.uint8, device="cuda")
    recs.verify_device(blob_dev(blob, shift), recs.ops_tensor(ops), ok, len(ops), mode, scratch=scratch, info=info)
    got = host(ok)
    assert (got[len(ops):] == CANARY).all() and set(got[:len(ops)].tolist()) <= {0, 1}
    return got[:len(ops)].astype(bool)


# ------------------------------------------------------------------------------------------------------------------ the seam
def run_seam(recs, blob, ops, shift=0):
    b, o = blob_dev(blob, shift), recs.ops_tensor(ops)
    class_slot, totals, plan = recs.plan_device(b, o, len(ops))
    packed = recs.pack_device(b, o, class_slot, totals, plan, len(ops))
    return host(class_slot).view(np.uint32), [int(x) for x in host(totals)], packed


def check_seam(got, want):
    class_slot, totals, packed = got
    assert np.array_equal(class_slot, want["class_slot"])
    assert totals == want["totals"]
    for pset in rc.SETS:
        g, w = packed[pset], want["packed"][pset]
        assert g["n"] == w["n"], pset
        assert np.array_equal(host(g["pk"]), w["pk"]) and np.array_equal(host(g["sigs"]), w["sigs"]), pset
        assert np.array_equal(host(g["msg_off"]).view(np.uint64), w["msg_off"]) and np.array_equal(host(g["ctx_off"]).view(np.uint64), w["ctx_off"]), pset
        assert np.array_equal(host(g["msgs"])[:w["msgs"].size], w["msgs"]) and np.array_equal(host(g["ctxs"])[:w["ctxs"].size], w["ctxs"]), pset


@pytest.mark.parametrize("mix", rc.MIXES)
@pytest.mark.parametrize("n", rc.SEAM_SIZES)
def test_seam_matches_the_restatement_byte_for_byte(recs, n, mix):
    blob, ops = rc.seam_case(n, mix, seed=n % 7)
    want = rc.expected(blob, ops)
    if mix.startswith("only"):  # two classes are empty
        assert sorted(want["totals"][:3]) == [0, 0, n]
    elif mix == "all_refused":
        assert want["totals"][:4] == [0, 0, 0, n]
    elif mix == "tenth_refused":
        assert want["totals"][3] == n // 10
    check_seam(run_seam(recs, blob, ops, shift=n % 4), want)


def test_seam_shared_and_overlapping_ranges(recs):
    blob, ops = rc.seam_case(12, "mod3", seed=3)
    assert ops[2]["msg_off"] == ops[1]["msg_off"] and ops[6]["pk_off"] == ops[3]["pk_off"] == ops[9]["pk_off"]
    assert ops[4]["sig_off"] < ops[5]["msg_off"] < ops[4]["sig_off"] + rc.SIG_LEN[int(ops[4]["set"])]
    ops = ops.copy()
    ops[10]["msg_off"], ops[10]["msg_len"] = blob.size, 0  # the empty range at the very end of the blob
    ops[11]["pk_off"] = 0  # a key range flush against offset 0, across other records' bytes
    want = rc.expected(blob, ops)
    assert want["totals"][3] == 0
    for shift in (0, 1, 2, 3, 15):
        check_seam(run_seam(recs, blob, ops, shift=shift), want)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("defect", rc.DEFECTS)
def test_one_refused_op_in_a_valid_batch(recs, sets, pool, defect):
    records = pool[MODE_PURE][:24]
    blob, ops = records_blob(records, pad=[3, 0, 7, 1, 12], front=1)
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, rc.PATTERN, dtype=np.uint8)])
    blob[int(ops[5]["sig_off"]) + 9] ^= 2  # one invalid signature among the valid ones
    base = run_verify(recs, blob, ops)
    assert base.tolist() == [i != 5 for i in range(24)]
    bad = ops.copy()
    rc.make_refused(bad, 13, defect, blob.size, region)
    got = run_verify(recs, blob, bad, shift=1)
    assert got.tolist() == [i not in (5, 13) for i in range(24)]
    class_slot, totals, packed = run_seam(recs, blob, bad)
    assert totals[3] == 1 and class_slot[13] >> 30 == 3
    check_seam((class_slot, totals, packed), rc.expected(blob, bad))
    for pset in rc.SETS:  # nothing of the region the refused op points into
        for name in ("pk", "sigs", "msgs", "ctxs"):
            assert bytes([rc.PATTERN]) * 8 not in host(packed[pset][name]).tobytes(), (pset, name)


# ------------------------------------------------------------------------------------------------------------------ op level
def damaged(records):
    """the records with, where the batch is long enough, a damaged signature (op 1), message (op 5), key (op 9) and a wrong context
    (op 13)"""
    out = list(records)
    flip = lambda b, at, bit: b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]  # noqa: E731
    if len(out) > 13:
        p, k, m, s, c = out[1]
        out[1] = (p, k, m, flip(s, len(s) // 2, 0x20), c)
        p, k, m, s, c = out[5]
        out[5] = (p, k, flip(m, 0, 1) if m else b"x", s, c)
        p, k, m, s, c = out[9]
        out[9] = (p, flip(k, 700, 8), m, s, c)
        p, k, m, s, c = out[13]
        out[13] = (p, k, m, s, c + b"!" if len(c) < 255 else c[:-1])
    return out


@pytest.mark.parametrize("n,mode", [(1, MODE_PURE), (65, MODE_PURE), (65, MODE_INTERNAL), (65, MODE_PREHASH), (1100, MODE_PURE)])
def test_verdicts_equal_verify_pk_per_set_and_the_oracle(recs, sets, pool, n, mode):
    records = damaged(pool[mode][:n])
    blob, ops = records_blob(records, pad=list(range(16)), front=0)
    want, _ = reference_ok(sets, blob, ops, mode)
    info = {}
    got = run_verify(recs, blob, ops, mode, info=info)
    assert np.array_equal(got, want)
    assert (info["n44"], info["n65"], info["n87"], info["refused"]) == ((n + 2) // 3, (n + 1) // 3, n // 3, 0)
    assert info["msg_bytes"] == sum(len(r[2]) for r in records) and info["ctx_bytes"] == sum(len(r[4]) for r in records)
    if n > 13:
        # a wrong context changes nothing where mu does not cover the context
        assert [i for i in range(n) if not want[i]] == ([1, 5, 9] if mode == MODE_INTERNAL else [1, 5, 9, 13])
    else:
        assert want.all()
    for i in sorted(set(range(min(n, 16))) | {n - 1}):  # a sample against the oracle, the damaged ops among it
        pset, pk, msg, sig, ctx = records[i]
        assert got[i] == orc.verify_internal(pset, orc.pk_try_from_bytes(pset, pk), msg, sig, ctx=ctx, mode=mode), i
    if n <= 65:  # the same verdicts wherever the blob lies
        for shift in (1, 2, 3):
            assert np.array_equal(run_verify(recs, blob, ops, mode, shift=shift), want), shift


# ------------------------------------------------------------------------------------------------------------------ scratch
def need_of(recs, ops, want):
    t = want["totals"]
    return recs.rec.mldsa_rec_front_bytes(len(ops)) + recs.rec.mldsa_rec_scratch_bytes(t[0], t[1], t[2], sum(t[4:7]), sum(t[7:10]))


def test_exact_scratch_passes_and_one_byte_less_is_refused(recs, sets, pool):
    records = pool[MODE_PURE][:30]
    blob, ops = records_blob(records, pad=5)
    want_ok, want = reference_ok(sets, blob, ops, MODE_PURE)
    need = need_of(recs, ops, want)
    assert need == rc.front_bytes(30) + rc.arena_bytes(10, 10, 10, sum(want["totals"][4:7]), sum(want["totals"][7:10]))
    info = {}
    exact = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert np.array_equal(run_verify(recs, blob, ops, scratch=exact, info=info), want_ok) and want_ok.all()
    assert info["scratch_needed"] == need
    # one byte less: MLDSA_ERR_NOMEM, nothing written to ok, the need named
    ok = torch.full((30,), CANARY, dtype=torch.uint8, device="cuda")
    info = {}
    with pytest.raises(_lib.MldsaError) as e:
        recs.verify_device(blob_dev(blob), recs.ops_tensor(ops), ok, 30, MODE_PURE, scratch=exact[:need - 1], info=info)
    assert e.value.code == _lib.ERR_NOMEM and "needs %d" % need in str(e.value)
    assert info["scratch_needed"] == need and (info["n44"], info["n65"], info["n87"]) == (10, 10, 10)
    assert (host(ok) == CANARY).all()
    # the bound for an unknown mix covers it
    assert recs.rec.mldsa_rec_front_bytes(30) + recs.rec.mldsa_rec_scratch_bytes_max(30, info["msg_bytes"], info["ctx_bytes"]) >= need


def test_shared_messages_count_once_per_op(recs, sets):
    m = sets[44]
    pk, sk = m.keygen_from_seed([shake(b"rec-shared", 0)])
    msg = shake(b"rec-shared-msg", 0, 20000)
    sig = host(m.try_sign_with_seed(m.private_keys_from_bytes(sk), [msg], [shake(b"rec-shared-rnd", 0)]))[0].tobytes()
    blob, one = records_blob([(44, host(pk)[0].tobytes(), msg, sig, b"")], pad=3)
    ops = np.repeat(one, 8)  # eight ops on one record: the messages alone exceed the blob
    ops[3]["msg_len"] -= 1   # (one of them on a shorter message: it fails)
    info = {}
    need = recs.rec.mldsa_rec_front_bytes(8) + recs.rec.mldsa_rec_scratch_bytes(8, 0, 0, 8 * 20000 - 1, 0)
    got = run_verify(recs, blob, ops, scratch=torch.empty(need, dtype=torch.uint8, device="cuda"), info=info)
    assert got.tolist() == [i != 3 for i in range(8)]
    assert info["msg_bytes"] == 8 * 20000 - 1 > blob.size and info["scratch_needed"] == need


# ------------------------------------------------------------------------------------------------------------------ stream order
def test_back_to_back_calls_share_a_scratch_and_a_side_stream_is_ordered(recs, sets, pool):
    a = damaged(pool[MODE_PURE][:40])
    b = pool[MODE_PURE][40:75]
    blob_a, ops_a = records_blob(a, pad=[1, 2, 3])
    blob_b, ops_b = records_blob(b, pad=[9, 0, 4], front=2)
    scratch = recs.verify_scratch(40, blob_a.size + blob_b.size, blob_a.size + blob_b.size)
    da, db, oa, ob = blob_dev(blob_a), blob_dev(blob_b, 3), recs.ops_tensor(ops_a), recs.ops_tensor(ops_b)
    ok_a = torch.full((40,), CANARY, dtype=torch.uint8, device="cuda")
    ok_b = torch.full((35,), CANARY, dtype=torch.uint8, device="cuda")
    recs.verify_device(da, oa, ok_a, 40, scratch=scratch)
    recs.verify_device(db, ob, ok_b, 35, scratch=scratch)  # no wait in between: the second call reuses the scratch in stream order
    assert host(ok_a).tolist() == [int(i not in (1, 5, 9, 13)) for i in range(40)] and host(ok_b).tolist() == [1] * 35
    # on a side stream the call runs behind the upload that precedes it there
    side = torch.cuda.Stream()
    pinned = torch.from_numpy(blob_a.copy()).pin_memory()
    target = torch.zeros(blob_a.size, dtype=torch.uint8, device="cuda")
    ok_s = torch.full((40,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        target.copy_(pinned, non_blocking=True)
        recs.verify_device(target, oa, ok_s, 40, scratch=scratch)
    side.synchronize()
    assert host(ok_s).tolist() == host(ok_a).tolist()


# ------------------------------------------------------------------------------------------------------------------ the Python front
def test_python_front_agrees_with_verify_pk_per_set(recs, sets, pool):
    records = damaged(pool[MODE_PURE][:60])  # four keys per set: every key repeats five times
    plain = recs.verify(records, pad=[0, 5, 11])
    dedup = recs.verify(records, dedup=True, pad=7)
    per_set = np.zeros(60, dtype=bool)
    for c, pset in enumerate(rc.SETS):
        mine = [r for r in records if r[0] == pset]
        per_set[c::3] = sets[pset].verify_pk([r[1] for r in mine], [r[2] for r in mine], [r[3] for r in mine], ctxs=[r[4] for r in mine])
    assert np.array_equal(plain, per_set) and np.array_equal(dedup, per_set)
    assert [i for i in range(60) if not per_set[i]] == [1, 5, 9, 13]
    assert recs.verify([]).size == 0
    # the seam of a mixed list: the arrays a caller feeds to MlDsa(pset) calls
    blob, ops = records_blob(records, pad=2)
    _, totals, packed = run_seam(recs, blob, ops)
    assert totals[:4] == [20, 20, 20, 0] and all(packed[p]["pk"].data_ptr() % 16 == 0 for p in rc.SETS)
