"""The request-signing library on the device (include/mldsa_recsign.h): the seam -- mldsa_recsign_plan, mldsa_recsign_pack and
mldsa_recsign_scatter -- byte for byte against the numpy restatement of tests/recsign_cases.py, mldsa_recsign_sign against mldsa_sign
per parameter set on arrays packed on the host and against the oracle, the round trip through the wire-record verifier in place,
refusals of single ops, the rnd rows' clearing, the scratch sizes, stream order, and the Python front."""
from gpu_common import *  # noqa: F401,F403

import rec_cases as rc
import recsign_cases as rs
from fips204_amd import _lib, _rec_lib, _recsign_lib
from fips204_amd.ml_dsa import (MODE_INTERNAL, MODE_PREHASH, MODE_PURE, MlDsaRecords, MlDsaRecordSigner, hash_message, sign_requests_blob)

pytestmark = pytest.mark.gpu

CANARY = 0x77
ST_CANARY = 0x77777777


@pytest.fixture(scope="module")
def keys(sets):
    """{pset: dict(pk: wire public keys (numpy), sks: the expanded private keys on the device)}: rs.N_KEYS keys per set"""
    out = {}
    for c, pset in enumerate(rs.SETS):
        pk, sk = sets[pset].keygen_from_seed([shake(b"recsign-key%d" % pset, j) for j in range(rs.N_KEYS[c])])
        out[pset] = dict(pk=host(pk), sks=sets[pset].private_keys_from_bytes(sk))
    return out


@pytest.fixture(scope="module")
def signer(hp, keys):
    s = MlDsaRecordSigner(hotpath=hp)
    for pset in rs.SETS:
        s.set_keys(pset, keys[pset]["sks"])
    return s


def placed(data, shift=0, tail=33):
    """(allocation, view): `data` (uint8 array) on the device, `shift` bytes into a canary-filled allocation with `tail` canary bytes
    behind it"""
    t = torch.full((data.size + shift + tail,), CANARY, dtype=torch.uint8, device="cuda")
    t[shift:shift + data.size] = torch.from_numpy(data.copy())
    return t, t[shift:shift + data.size]


def requests(n, tag, mode=MODE_PURE, sets_of=None):
    """n requests (pset, key, message, ctx, rnd or None), sets dealt i mod 3, four keys per set dealt round-robin, message and context
    lengths cycling through rc.MSG_LENS and rc.CTX_LENS, every third without rnd"""
    out = []
    for i in range(n):
        pset = rs.SETS[i % 3] if sets_of is None else sets_of[i]
        msg = shake(tag + b"msg", i, rc.MSG_LENS[(i // 3) % len(rc.MSG_LENS)])
        if mode == MODE_PREHASH:
            msg = hash_message(msg, "SHA256")
        out.append((pset, (i // 3) % 4, msg, shake(tag + b"ctx", i, rc.CTX_LENS[(i // 3) % len(rc.CTX_LENS)]),
                    None if i % 3 == 2 else shake(tag + b"rnd", i)))
    return out


def core_signed(sets, table, want, mode=MODE_PURE):
    """{pset: sigs [n_c, SIG_LEN]}, {pset: status [n_c]}: the restated packed arrays signed by MlDsa(pset).try_sign_with_seed"""
    sigs, status = {}, {}
    for pset in rs.SETS:
        r = rs.requests_of(want["packed"][pset])
        status[pset] = np.zeros(len(r), dtype=np.int32)
        if not r:
            sigs[pset] = np.zeros((0, rs.SIG_LEN[pset]), dtype=np.uint8)
            continue
        sigs[pset] = host(sets[pset].try_sign_with_seed(table[pset], [x[1] for x in r], [x[3] for x in r], ctxs=[x[2] for x in r],
                                                        key_idx=np.array([x[0] for x in r], dtype=np.uint32), mode=mode))
    return sigs, status


def run_sign(signer, blob, ops, out_len, mode=MODE_PURE, in_place=False, shift=0, scratch=None, info=None):
    """mldsa_recsign_sign with the blob `shift` bytes into its allocation and (unless in_place) the output buffer `shift + 1` bytes into
    a canary-filled one: (the output buffer's whole allocation, where the buffer begins in it, status)"""
    alloc_b, b = placed(blob, shift)
    alloc_o, o = (alloc_b, b) if in_place else placed(np.full(out_len, CANARY, dtype=np.uint8), shift + 1)
    status = torch.full((len(ops) + 8,), ST_CANARY, dtype=torch.int32, device="cuda")
    signer.sign_device(b, signer.ops_tensor(ops), o, status, len(ops), mode, scratch=scratch, info=info)
    st = host(status)
    assert (st[len(ops):] == ST_CANARY).all()
    return host(alloc_o), (shift if in_place else shift + 1), st[:len(ops)]


def expected_sign(sets, table, blob, ops, out_len, n_keys, mode=MODE_PURE, in_place=False, shift=0):
    """what run_sign must return, from the restatement fed with the core's signatures of the host-packed arrays"""
    want = rs.expected(blob, ops, n_keys, out_len)
    before = blob if in_place else np.full(out_len, CANARY, dtype=np.uint8)
    out, st = rs.scattered(before, ops, want, *core_signed(sets, table, want, mode))
    at = shift if in_place else shift + 1
    alloc = np.full(out.size + at + 33, CANARY, dtype=np.uint8)
    alloc[at:at + out.size] = out
    return alloc, st, want


def table_of(keys):
    return {pset: keys[pset]["sks"] for pset in rs.SETS}


# ------------------------------------------------------------------------------------------------------------------ the pack seam
def run_pack(signer, blob, ops, out_len, shift=0, arena=None):
    _, b = placed(blob, shift)
    o = signer.ops_tensor(ops)
    class_slot, totals, plan = signer.plan_device(o, blob.size, out_len, len(ops))
    packed = signer.pack_device(b, o, out_len, class_slot, totals, plan, len(ops), arena=arena)
    return host(class_slot).view(np.uint32), [int(x) for x in host(totals)], packed, class_slot, o


def check_pack(got, want):
    class_slot, totals, packed = got[:3]
    assert np.array_equal(class_slot, want["class_slot"])
    assert totals == want["totals"]
    for pset in rs.SETS:
        g, w = packed[pset], want["packed"][pset]
        assert g["n"] == w["n"], pset
        assert np.array_equal(host(g["key_idx"]).view(np.uint32), w["key_idx"]) and np.array_equal(host(g["rnd"]), w["rnd"]), pset
        assert np.array_equal(host(g["msg_off"]).view(np.uint64), w["msg_off"]) and np.array_equal(host(g["ctx_off"]).view(np.uint64), w["ctx_off"]), pset
        assert np.array_equal(host(g["msgs"])[:w["msgs"].size], w["msgs"]) and np.array_equal(host(g["ctxs"])[:w["ctxs"].size], w["ctxs"]), pset


@pytest.mark.parametrize("mix", rs.MIXES)
@pytest.mark.parametrize("n", rc.SEAM_SIZES)
def test_pack_seam_matches_the_restatement_byte_for_byte(signer, n, mix):
    blob, ops, out_len = rs.seam_case(n, mix, seed=n % 7)
    want = rs.expected(blob, ops, rs.N_KEYS, out_len)
    if mix.startswith("only"):  # two classes are empty
        assert sorted(want["totals"][:3]) == [0, 0, n]
    elif mix == "all_refused":
        assert want["totals"][:4] == [0, 0, 0, n]
    elif mix == "tenth_refused":
        assert want["totals"][3] == n // 10
    got = run_pack(signer, blob, ops, out_len, shift=n % 4)
    check_pack(got, want)
    for pset in rs.SETS:  # nothing of the region the refused ops point into
        for name in ("rnd", "msgs", "ctxs"):
            assert bytes([rs.PATTERN]) * 8 not in host(got[2][pset][name]).tobytes(), (pset, name)


# ------------------------------------------------------------------------------------------------------------------ the scatter seam
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 15])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_scatter_seam_on_arbitrary_bytes(signer, n, shift):
    blob, ops, out_len = rs.seam_case(n, "tenth_refused", seed=(n + shift) % 7)
    want = rs.expected(blob, ops, rs.N_KEYS, out_len)
    _, _, packed, class_slot, o = run_pack(signer, blob, ops, out_len)
    sigs, status = {}, {}
    for pset in rs.SETS:  # no signing: rows of arbitrary bytes, made-up codes
        n_c = want["packed"][pset]["n"]
        sigs[pset] = np.frombuffer(shake(b"rs-sig%d" % pset, n, n_c * rs.SIG_LEN[pset]), dtype=np.uint8).reshape(n_c, rs.SIG_LEN[pset])
        status[pset] = ((np.arange(n_c) * 7 - 5) * (1 if pset != 65 else -3)).astype(np.int32)
        if n_c:
            packed[pset]["sigs"].copy_(dev(sigs[pset]))
            packed[pset]["status"].copy_(dev(status[pset]))
    alloc, out = placed(np.full(out_len, CANARY, dtype=np.uint8), shift)
    st = torch.full((n + 8,), ST_CANARY, dtype=torch.int32, device="cuda")
    signer.scatter_device(o, blob.size, out, class_slot, packed, st, n)
    want_out, want_st = rs.scattered(np.full(out_len, CANARY, dtype=np.uint8), ops, want, sigs, status)
    want_alloc = np.full(alloc.numel(), CANARY, dtype=np.uint8)
    want_alloc[shift:shift + out_len] = want_out
    assert np.array_equal(host(alloc), want_alloc)  # the canary everywhere outside the accepted holes
    assert np.array_equal(host(st)[:n], want_st) and (host(st)[n:] == ST_CANARY).all()
    if n >= 10:
        assert (want_st[9::10] < 0).all() and want["totals"][3] == n // 10


# ------------------------------------------------------------------------------------------------------------------ the whole pass
def with_refusals(blob, ops, out_len, every=10):
    """the blob with a pattern region behind it and every `every`th op damaged with one of rs.DEFECTS in turn"""
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, rs.PATTERN, dtype=np.uint8)])
    ops = ops.copy()
    for r, i in enumerate(range(every - 1, len(ops), every)):
        rs.make_refused(ops, i, r % len(rs.DEFECTS), blob.size, out_len, region)
    return blob, ops


@pytest.mark.parametrize("n,mode,refuse", [(257, MODE_PURE, True), (3, MODE_PURE, False), (12, MODE_INTERNAL, False), (12, MODE_PREHASH, False)])
def test_whole_pass_equals_the_core_on_host_packed_arrays(signer, sets, keys, n, mode, refuse):
    reqs = requests(n, b"rs-pass%d" % mode, mode)
    blob, ops, out_len = sign_requests_blob(reqs, pad=list(range(16)), front=0)
    if refuse:
        blob, ops = with_refusals(blob, ops, out_len)
    want_alloc, want_st, want = expected_sign(sets, table_of(keys), blob, ops, out_len, rs.N_KEYS, mode, shift=n % 4)
    info = {}
    alloc, _, st = run_sign(signer, blob, ops, out_len, mode, shift=n % 4, info=info)
    assert np.array_equal(st, want_st) and np.array_equal(alloc, want_alloc)
    assert [info["n44"], info["n65"], info["n87"], info["refused"]] == want["totals"][:4]
    assert info["msg_bytes"] == sum(want["totals"][4:7]) and info["ctx_bytes"] == sum(want["totals"][7:10])
    if refuse:
        assert info["refused"] == n // 10 and sorted(set(st.tolist())) == [rs.ERR_CTX_LEN, rs.ERR_PARAM, 0]
    else:
        assert not st.any()


def test_the_oracles_signatures_byte_for_byte(hp, sets):
    q = rs.oracle_requests()
    s = MlDsaRecordSigner(hotpath=hp)
    for pset, seeds in rs.oracle_key_seeds().items():
        _, sk = sets[pset].keygen_from_seed(seeds)
        s.set_keys(pset, sets[pset].private_keys_from_bytes(sk))
    for in_place in (False, True):
        blob, ops, out_len = sign_requests_blob(q["requests"], pad=list(range(16)), front=1, in_place=in_place)
        alloc, at, st = run_sign(s, blob, ops, out_len, in_place=in_place, shift=2)
        assert not st.any()
        for i, (pset, key, msg, ctx, rnd) in enumerate(q["requests"]):
            lo = at + int(ops[i]["sig_off"])
            assert alloc[lo:lo + rs.SIG_LEN[pset]].tobytes() == q["sigs"][i], (in_place, i)


def test_round_trip_in_place_through_the_record_verifier(signer, hp, keys):
    """65 records, each holding key, signature hole, message, context and rnd, signed with out == blob: mldsa_rec_verify then accepts
    every one, and one flipped message byte refuses that record alone"""
    n = 65
    reqs = requests(n, b"rs-trip")
    sign_ops = np.zeros(n, dtype=_recsign_lib.OP_DTYPE)
    vfy_ops = np.zeros(n, dtype=_rec_lib.OP_DTYPE)
    parts, at, k = [], 0, 0
    for i, (pset, key, msg, ctx, rnd) in enumerate(reqs):
        fields = [("pk", keys[pset]["pk"][key].tobytes()), ("sig", bytes([0xC3]) * rs.SIG_LEN[pset]), ("msg", msg), ("ctx", ctx)]
        if rnd is not None:
            fields.append(("rnd", rnd))
        off = {}
        for name, field in fields:
            gap = (k * 5 + 3) % 16
            k += 1
            parts += [bytes([0xC3]) * gap, field]
            off[name] = at + gap
            at += gap + len(field)
        sign_ops[i] = (off["msg"], off["ctx"], off.get("rnd", 0), off["sig"], len(msg), key, len(ctx), pset, 0 if rnd is None else 1, 0)
        vfy_ops[i] = (off["pk"], off["sig"], off["msg"], off["ctx"], len(msg), len(ctx), pset, 0)
    blob_h = np.frombuffer(b"".join(parts), dtype=np.uint8)
    _, blob = placed(blob_h, 3)
    status = torch.full((n,), ST_CANARY, dtype=torch.int32, device="cuda")
    signer.sign_device(blob, signer.ops_tensor(sign_ops), blob, status, n)
    assert not host(status).any()
    after = host(blob)
    hole = np.zeros(blob_h.size, dtype=bool)
    for i in range(n):
        hole[int(sign_ops[i]["sig_off"]):int(sign_ops[i]["sig_off"]) + rs.SIG_LEN[reqs[i][0]]] = True
    assert np.array_equal(after[~hole], blob_h[~hole])  # nothing but the holes changed
    recs = MlDsaRecords(hotpath=hp)
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    recs.verify_device(blob, recs.ops_tensor(vfy_ops), ok, n)
    assert host(ok).tolist() == [1] * n
    victim = 16  # a record with a message of at least one byte
    assert int(sign_ops[victim]["msg_len"]) > 0
    blob[int(sign_ops[victim]["msg_off"])] ^= 0x04
    recs.verify_device(blob, recs.ops_tensor(vfy_ops), ok, n)
    assert host(ok).tolist() == [int(i != victim) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def undamaged(signer):
    reqs = requests(12, b"rs-refuse")
    blob, ops, out_len = sign_requests_blob(reqs, pad=[3, 0, 7, 1, 12], front=1)
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, rs.PATTERN, dtype=np.uint8)])
    alloc, at, st = run_sign(signer, blob, ops, out_len)
    assert not st.any() and (alloc[:at] == CANARY).all()
    return dict(blob=blob, ops=ops, out_len=out_len, region=region, alloc=alloc, at=at)


def holes_of(ops, at, total):
    """one mask per op over an allocation of `total` bytes whose output buffer begins at `at`"""
    masks = []
    for op in ops:
        m = np.zeros(total, dtype=bool)
        m[at + int(op["sig_off"]):at + int(op["sig_off"]) + rs.SIG_LEN[int(op["set"])]] = True
        masks.append(m)
    return masks


@pytest.mark.parametrize("defect", rs.DEFECTS)
def test_each_defect_refuses_its_op_alone(signer, undamaged, defect):
    u = undamaged
    bad = u["ops"].copy()
    rs.make_refused(bad, 4, defect, u["blob"].size, u["out_len"], u["region"])
    alloc, at, st = run_sign(signer, u["blob"], bad, u["out_len"])
    assert st.tolist() == [rs.DEFECT_STATUS[defect] if i == 4 else 0 for i in range(12)]
    mine = holes_of(u["ops"], at, alloc.size)[4]
    assert (alloc[mine] == CANARY).all()                       # its hole keeps the canary
    assert np.array_equal(alloc[~mine], u["alloc"][~mine])     # every other byte is the undamaged call's


def test_an_unserved_set_refuses_all_its_ops(hp, keys, undamaged):
    u = undamaged
    s = MlDsaRecordSigner(hotpath=hp)
    s.set_keys(44, keys[44]["sks"])
    s.set_keys(87, keys[87]["sks"])
    alloc, at, st = run_sign(s, u["blob"], u["ops"], u["out_len"])
    assert st.tolist() == [rs.ERR_PARAM if i % 3 == 1 else 0 for i in range(12)]
    masks = holes_of(u["ops"], at, alloc.size)
    mine = np.logical_or.reduce([masks[i] for i in range(1, 12, 3)])
    assert (alloc[mine] == CANARY).all() and np.array_equal(alloc[~mine], u["alloc"][~mine])


def test_no_rnd_flag_is_thirty_two_zero_bytes(signer):
    reqs = [(pset, 1, b"deterministic", b"ctx", None) for pset in rs.SETS]
    zero = [(pset, 1, b"deterministic", b"ctx", bytes(32)) for pset in rs.SETS]
    a, sa = signer.sign(reqs)
    b, sb = signer.sign(zero)
    c, _ = signer.sign([(pset, 1, b"deterministic", b"ctx", bytes([1]) * 32) for pset in rs.SETS])
    assert not sa.any() and not sb.any() and a == b and all(x != y for x, y in zip(a, c))


# ------------------------------------------------------------------------------------------------------------------ scratch
def need_of(signer, n, want):
    t = want["totals"]
    return signer.lib.mldsa_recsign_front_bytes(n) + signer.lib.mldsa_recsign_arena_bytes(t[0], t[1], t[2], sum(t[4:7]), sum(t[7:10]))


def test_rnd_does_not_outlive_the_call(signer):
    reqs = requests(30, b"rs-rnd")
    rnds = [r[4] for r in reqs if r[4] is not None]
    blob, ops, out_len = sign_requests_blob(reqs, pad=5)
    want = rs.expected(blob, ops, rs.N_KEYS, out_len)
    scratch = filled(need_of(signer, 30, want) + 512)
    _, _, st = run_sign(signer, blob, ops, out_len, scratch=scratch)
    assert not st.any()
    left = host(scratch).tobytes()
    assert len(rnds) == 20 and not any(r in left for r in rnds)
    assert bytes([0x5A]) * 64 in left  # (the scratch is not cleared wholesale: rnd is its one secret)
    # positive control: after the pack alone every rnd row is there
    arena = filled(signer.lib.mldsa_recsign_arena_bytes_max(30, blob.size, blob.size))
    packed = run_pack(signer, blob, ops, out_len, arena=arena)[2]
    there = host(arena).tobytes()
    assert all(r in there for r in rnds) and all(r in host(packed["rnd_region"]).tobytes() for r in rnds)
    packed["rnd_region"].zero_()
    assert not any(r in host(arena).tobytes() for r in rnds)


def test_exact_scratch_passes_and_one_byte_less_is_refused(signer, sets, keys):
    reqs = requests(30, b"rs-scratch")
    blob, ops, out_len = sign_requests_blob(reqs, pad=5)
    want_alloc, want_st, want = expected_sign(sets, table_of(keys), blob, ops, out_len, rs.N_KEYS)
    need = need_of(signer, 30, want)
    assert need == rs.front_bytes(30) + rs.arena_bytes(10, 10, 10, sum(want["totals"][4:7]), sum(want["totals"][7:10]))
    exact = torch.empty(need, dtype=torch.uint8, device="cuda")
    # one byte less: MLDSA_ERR_NOMEM, out and status untouched, the need named
    info = {}
    with pytest.raises(_lib.MldsaError) as e:
        alloc_o, o = placed(np.full(out_len, CANARY, dtype=np.uint8), 1)
        status = torch.full((30,), ST_CANARY, dtype=torch.int32, device="cuda")
        signer.sign_device(placed(blob)[1], signer.ops_tensor(ops), o, status, 30, scratch=exact[:need - 1], info=info)
    assert e.value.code == _lib.ERR_NOMEM and "needs %d" % need in str(e.value)
    assert info["scratch_needed"] == need and (info["n44"], info["n65"], info["n87"]) == (10, 10, 10)
    assert (host(alloc_o) == CANARY).all() and (host(status) == ST_CANARY).all()
    # a scratch of exactly that size succeeds
    info = {}
    alloc, _, st = run_sign(signer, blob, ops, out_len, scratch=exact, info=info)
    assert np.array_equal(alloc, want_alloc) and np.array_equal(st, want_st) and info["scratch_needed"] == need
    # the bound for an unknown mix covers it
    assert signer.lib.mldsa_recsign_front_bytes(30) + signer.lib.mldsa_recsign_arena_bytes_max(30, info["msg_bytes"], info["ctx_bytes"]) >= need


# ------------------------------------------------------------------------------------------------------------------ stream order
def test_a_side_stream_is_ordered(signer, sets, keys):
    reqs = requests(24, b"rs-stream")
    blob, ops, out_len = sign_requests_blob(reqs, pad=[1, 2, 3], in_place=True)
    want_alloc, want_st, _ = expected_sign(sets, table_of(keys), blob, ops, out_len, rs.N_KEYS, in_place=True)
    side = torch.cuda.Stream()
    pinned = torch.from_numpy(blob.copy()).pin_memory()
    target = torch.zeros(blob.size, dtype=torch.uint8, device="cuda")
    status = torch.full((24,), ST_CANARY, dtype=torch.int32, device="cuda")
    o = signer.ops_tensor(ops)
    back = torch.empty(blob.size, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        target.copy_(pinned, non_blocking=True)  # the upload right before the call, on the call's stream
        signer.sign_device(target, o, target, status, 24)
        back.copy_(target, non_blocking=True)    # and the result read behind it
    side.synchronize()
    assert np.array_equal(back.numpy(), want_alloc[:blob.size]) and np.array_equal(host(status), want_st)


# ------------------------------------------------------------------------------------------------------------------ the Python front
@pytest.mark.parametrize("in_place", [False, True])
def test_python_front_agrees_with_the_core_per_set(signer, sets, keys, in_place):
    reqs = requests(30, b"rs-front")
    sigs, st = signer.sign(reqs, in_place=in_place)
    assert not st.any() and st.dtype == np.int32 and len(sigs) == 30
    for c, pset in enumerate(rs.SETS):
        mine = [r for r in reqs if r[0] == pset]
        ref = host(sets[pset].try_sign_with_seed(keys[pset]["sks"], [r[2] for r in mine], [r[4] or bytes(32) for r in mine],
                                                 ctxs=[r[3] for r in mine], key_idx=np.array([r[1] for r in mine], dtype=np.uint32)))
        assert [s for s, r in zip(sigs, reqs) if r[0] == pset] == [row.tobytes() for row in ref], pset
    none, st0 = signer.sign([])
    assert none == [] and st0.size == 0
    bad, st = signer.sign([(65, 4, b"m", b"", None), (65, 0, b"m", b"x" * 256, None)], in_place=in_place)  # key = n_keys; ctx too long
    assert st.tolist() == [rs.ERR_PARAM, rs.ERR_CTX_LEN]
