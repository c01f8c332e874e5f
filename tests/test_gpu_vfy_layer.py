"""GPU parity of the large-batch verify library (include/mldsa_vfy.h) with the core's mldsa_verify and with the oracle: the ExpandA
seam on the folded Keccak round, whole verdicts over parts of 64 ops, damaged signatures, stream order, profiling and routing.
Every call is small: the part size is forced to 64 through mldsa_vfy_set_part_ops, so 257 ops are five parts with a one-op tail."""
import json

import rare_sampler_cases as rc
import sig_cases
from fips204_amd import _lib, _vfy_lib
from fips204_amd.ml_dsa import MODE_PREHASH, MODE_PURE, _cat_with_offsets
from gpu_common import *
from vfy_calls import core_verify, gathered, verdicts, vfy_expand_a, vfy_verify

pytestmark = pytest.mark.gpu

PART = 64
SIZES = (1, 63, 64, 65, 257)
N, NK = 257, 7
STAGES = ("expand_a", "verify_main", "ctilde_hash", "mu", "sample_in_ball")
# fixed sites of the 257-op batch, all inside its first 63 ops
OP_CTX256, OP_OOR, OP_BAD_PAIR, OP_5K = 5, 9, 20, 30


@pytest.fixture(scope="module")
def vfy():
    lib = _vfy_lib.load()
    lib.mldsa_vfy_set_part_ops(PART)
    yield lib
    lib.mldsa_vfy_set_part_ops(0)


def stale(n):
    return torch.full((max(n, 1),), 0x5A, dtype=torch.uint8, device="cuda")


def both(lib, m, n, *a, **kw):
    """the verdicts of the library and of the core on the same arguments, as bool arrays"""
    return verdicts(vfy_verify(lib, m, *a[:4], stale(n), n, *a[4:], **kw), n), verdicts(core_verify(m, *a[:4], stale(n), n, *a[4:], **kw), n)


# ------------------------------------------------------------------------------------------------------------- the batch
def _msg_len(i, clen):
    """message lengths: tr | M' = 64 + 2 + clen + mlen ends one before, on and one after a 136-byte boundary for ops 0 ... 8"""
    if i < 9:
        return 136 * (2 + i // 3 + (clen + 66) // 136) - 66 - clen + (i % 3 - 1)
    if i == OP_5K:
        return 5 * 1024
    return (0, 1, 31, 32, 70, 200, 207)[i % 7]


_batches = {}


def batch(m):
    """257 signed ops over 7 keys, built once per parameter set.  Op OP_CTX256 is verified under a ctx of 256 bytes, op OP_OOR under a
    key index outside the table; the message of op OP_BAD_PAIR + 1 is the bytes of ops OP_BAD_PAIR - 1, OP_BAD_PAIR and its own tail, so
    the table whose entry OP_BAD_PAIR + 1 points back to the start of op OP_BAD_PAIR - 1 is malformed for op OP_BAD_PAIR alone."""
    if m.pset in _batches:
        return _batches[m.pset]
    pset = m.pset
    xi = [shake(b"vfy-key%d" % pset, i) for i in range(NK)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    ctxs = [(b"", shake(b"vfy-ctx", i, 255), shake(b"vfy-ctx", i, 17))[i % 3] for i in range(N)]
    laid = [shake(b"vfy-msg%d" % pset, i, _msg_len(i, len(ctxs[i]))) for i in range(N)]  # the bytes in each op's slot of the buffer
    msgs = list(laid)
    k = OP_BAD_PAIR
    msgs[k + 1] = laid[k - 1] + laid[k] + laid[k + 1]
    rnd = [shake(b"vfy-rnd", i) for i in range(N)]
    kidx = (np.arange(N) * 3 % NK).astype(np.uint32)
    sig = m.try_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, key_idx=kidx, mode=MODE_PURE)
    torch.cuda.synchronize()
    # what the verifier is shown
    vctx = list(ctxs)
    vctx[OP_CTX256] = shake(b"vfy-ctx", OP_CTX256, 256)
    mbuf, moff = table(laid)
    moff_bad = moff.copy()
    moff_bad[k + 1] = moff[k - 1]
    cbuf, coff = table(vctx)
    vkidx = kidx.copy()
    vkidx[OP_OOR] = NK + 5
    want = np.ones(N, dtype=bool)
    want[[OP_CTX256, OP_OOR, k]] = False
    okeys = [orc.pk_try_from_bytes(pset, host(pk)[i].tobytes()) for i in range(NK)]
    b = dict(pks=pks, sks=sks, okeys=okeys, sig=sig, kidx=kidx, vkidx=vkidx, msgs=msgs, vctx=vctx, want=want, mb=dev(mbuf), mo=dev_off(moff_bad),
             mo_good=dev_off(moff), cb=dev(cbuf), co=dev_off(coff), moff=moff, moff_bad=moff_bad, per_op=gathered(pks, kidx))
    _batches[pset] = b
    return b


def oracle_verdict(pset, b, i, sig=None):
    """the oracle on what the verifier is shown for op i (a valid key index; the message as the malformed table delimits it)"""
    msg = b["msgs"][i]
    return orc.verify_internal(pset, b["okeys"][int(b["kidx"][i])], msg, bytes(host(b["sig"])[i]) if sig is None else sig, ctx=b["vctx"][i],
                               mode=MODE_PURE)


# ---------------------------------------------------------------------------------------------------------- 1: ExpandA seam
@pytest.mark.parametrize("n", [1, 2, 3, 13])
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_expand_a_seam_is_the_cores_and_the_oracles(vfy, hp, sets, pset, n):
    """n x K x L streams: 16 ... 728, so the 64-stream wave boundary and the 256-stream block boundary fall inside ops"""
    m = sets[pset]
    k, l = m.params.k, m.params.l
    seeds = [shake(b"vfy-rho%d" % pset, 100 * n + i) for i in range(n)]
    rho = dev(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n, 32))
    got = vfy_expand_a(vfy, m, rho)
    core = hp.expand_a(pset, rho).flatten(1, 2)
    torch.cuda.synchronize()
    assert torch.equal(got, core)
    want = np.stack([orc.expand_a(k, l, s).reshape(k * l, 256) for s in seeds])
    assert np.array_equal(host(got), want)
    assert int(got.min()) >= 0 and int(got.max()) < 8380417


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_expand_a_seam_on_the_rejection_path_seeds(vfy, hp, sets, pset):
    """the rho of every ExpandA entry of tests/golden/rare_sampler_seeds.json.gz: candidates equal to q and q - 1 in each position of a
    group of four, two rejections in one group, the polynomial filled on the last candidate of a block"""
    fx = rc.load_fixture()
    m = sets[pset]
    seeds = []
    for cat in ("ea_boundary", "ea_shape"):
        for e in fx[cat][str(pset)]:
            if bytes.fromhex(e["rho"]) not in seeds:
                seeds.append(bytes.fromhex(e["rho"]))
    assert len(seeds) >= 12
    rho = dev(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(len(seeds), 32))
    got = vfy_expand_a(vfy, m, rho)
    core = hp.expand_a(pset, rho).flatten(1, 2)
    torch.cuda.synchronize()
    assert torch.equal(got, core)
    k, l = m.params.k, m.params.l
    for i, s in enumerate(seeds):
        want = orc.expand_a(k, l, s).reshape(k * l, 256)
        assert np.array_equal(rc.expand_a(pset, s)[0].reshape(-1, 256), want)
        assert np.array_equal(host(got[i]), want), s.hex()


# -------------------------------------------------------------------------------------------------------- 2: verdict parity
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verdicts_are_the_cores_and_the_oracles(vfy, sets, pset, n):
    m = sets[pset]
    b = batch(m)
    sig = b["sig"][:n].contiguous()
    assert vfy.mldsa_vfy_set_part_ops(PART) == PART
    parts = (n + PART - 1) // PART
    assert parts == {1: 1, 63: 1, 64: 1, 65: 2, 257: 5}[n]
    # ---- a key table: the 256-byte ctx, the index outside the table and the malformed pair are refused alone
    if n > OP_BAD_PAIR + 1:
        got, ref = both(vfy, m, n, b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), sig, b["cb"], b["co"][:n + 1].contiguous(), kidx_dev(b["vkidx"][:n]))
        want = b["want"][:n]
        assert got.tolist() == ref.tolist() == want.tolist()
        assert not got[OP_CTX256] and not got[OP_OOR] and not got[OP_BAD_PAIR] and got[OP_BAD_PAIR + 1] and got[OP_BAD_PAIR - 1]
        check = sorted({0, 1, 2, 3, 4, OP_CTX256, 6, 7, 8, OP_BAD_PAIR - 1, OP_BAD_PAIR + 1, OP_5K, n - 1} - {OP_OOR, OP_BAD_PAIR})
        assert len(check) >= 8
        for i in check:
            assert oracle_verdict(pset, b, i) == bool(want[i]), i
        assert len(b["msgs"][OP_5K]) == 5120 and {(66 + len(b["vctx"][i]) + len(b["msgs"][i])) % 136 for i in (0, 1, 2, 6, 7, 8)} == {135, 0, 1}
    else:
        # one op: alone, then under an index outside the table, then under a malformed pair of its own
        args = (b["pks"], b["mb"], b["mo_good"][:2].contiguous(), sig, b["cb"], b["co"][:2].contiguous())
        got, ref = both(vfy, m, 1, *args, kidx_dev(b["kidx"][:1]))
        assert got.tolist() == ref.tolist() == [True] and oracle_verdict(pset, b, 0)
        got, ref = both(vfy, m, 1, *args, kidx_dev(np.array([NK], dtype=np.uint32)))
        assert got.tolist() == ref.tolist() == [False]
        bad = dev_off(np.array([int(b["moff"][1]), 0], dtype=np.uint64))
        got, ref = both(vfy, m, 1, b["pks"], b["mb"], bad, sig, b["cb"], b["co"][:2].contiguous(), kidx_dev(b["kidx"][:1]))
        assert got.tolist() == ref.tolist() == [False]
    # ---- no key_idx: op i uses key i of a table of one key per op; no ctx table: every ctx empty, so only the ops signed under one pass
    mo = (b["mo"] if n > OP_BAD_PAIR + 1 else b["mo_good"])[:n + 1].contiguous()
    got, ref = both(vfy, m, n, b["per_op"], b["mb"], mo, sig)
    want = np.array([len(b["vctx"][i]) == 0 for i in range(n)])
    want[OP_BAD_PAIR:n] &= b["want"][OP_BAD_PAIR:n]
    assert got.tolist() == ref.tolist() == want.tolist()
    # ---- no key_idx, with the ctx table: the key of op OP_OOR is its own again
    got, ref = both(vfy, m, n, b["per_op"], b["mb"], mo, sig, b["cb"], b["co"][:n + 1].contiguous())
    want = b["want"][:n].copy()
    want[OP_OOR:OP_OOR + 1] = True
    assert got.tolist() == ref.tolist() == want.tolist()


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_prehash_mode(vfy, sets, pset):
    """MODE_PREHASH: the message is OID | PH(M), M' = 0x01 | len(ctx) | ctx | OID | PH(M); 65 ops = two parts"""
    m = sets[pset]
    b = batch(m)
    n = 65
    ctxs = [shake(b"vfy-phctx", i, (0, 9, 255)[i % 3]) for i in range(n)]
    phm = []
    for i in range(n):
        oid, d = orc.hash_message(shake(b"vfy-phmsg", i, 100 + i), ("SHA256", "SHA512", "SHAKE128")[i % 3])
        phm.append(oid + d)
    rnd = [shake(b"vfy-phrnd", i) for i in range(n)]
    kidx = (np.arange(n) % NK).astype(np.uint32)
    sig = m.try_sign_with_seed(b["sks"], phm, rnd, ctxs=ctxs, key_idx=kidx, mode=MODE_PREHASH)
    mb, mo = _cat_with_offsets(phm, m.device)
    cb, co = _cat_with_offsets(ctxs, m.device)
    got, ref = both(vfy, m, n, b["pks"], mb, mo, sig, cb, co, kidx_dev(kidx), mode=MODE_PREHASH)
    assert got.tolist() == ref.tolist() == [True] * n
    sigs = host(sig)
    for i in (0, 1, 2, 30, 31, 62, 63, 64):
        assert orc.verify_internal(pset, b["okeys"][int(kidx[i])], phm[i], bytes(sigs[i]), ctx=ctxs[i], mode=MODE_PREHASH)
    # the same bytes under the pure prefix are another message
    got, ref = both(vfy, m, n, b["pks"], mb, mo, sig, cb, co, kidx_dev(kidx), mode=MODE_PURE)
    assert got.tolist() == ref.tolist() == [False] * n


# --------------------------------------------------------------------------------------------------- 3: damaged signatures
def damaged(m, good):
    """name -> a damaged copy of the signature `good` (numpy uint8): one flipped bit in c~, in each z polynomial and in the hint section,
    and the three malformed hint shapes"""
    p = m.params
    cb, z0, h0 = sig_cases.sections(p)
    total = int(sig_cases.hint_limits(p, good)[-1])
    assert 2 <= total < p.omega, total  # room for every shape below: positions to swap, padding to dirty
    sites = {"ctilde_bit": (z0 // 2, 3), **{f"z{j}_bit": (z0 + j * 32 * cb + 11 * (j + 1), j % 8) for j in range(p.l)},
             "hint_bit": (h0, 0),  # the first position moves: another w1, or a position that no longer increases
             "hint_positions_not_increasing": None, "hint_limit_above_omega": None, "hint_padding_not_zero": None}
    return {name: sig_cases.damage(p, good, name, 0, site) for name, site in sites.items()}


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_damaged_signatures(vfy, sets, pset):
    m = sets[pset]
    b = batch(m)
    first = 56  # ops 56 ... : good signatures of the batch, each damaged one way, across the boundary of the first two parts
    sig = host(b["sig"]).copy()
    names = []
    for j, (name, s) in enumerate(damaged(m, sig[first]).items()):
        op = first + j
        for nm, s2 in damaged(m, sig[op]).items():
            if nm == name:
                sig[op] = s2
        names.append(name)
    assert len(names) == 1 + m.params.l + 1 + 3
    n = first + len(names) + 10  # the last ten ops are good again
    assert PART < n <= N
    got, ref = both(vfy, m, n, b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), dev(sig[:n]), b["cb"], b["co"][:n + 1].contiguous(),
                    kidx_dev(b["vkidx"][:n]))
    want = b["want"][:n].copy()
    want[first:first + len(names)] = False
    assert got.tolist() == ref.tolist() == want.tolist(), [nm for j, nm in enumerate(names) if got[first + j]]
    for j, name in enumerate(names):
        assert not oracle_verdict(pset, b, first + j, sig=bytes(sig[first + j])), name
    assert want[first + len(names):].all() and oracle_verdict(pset, b, n - 1)


# ----------------------------------------------------------------------------------------- 4: stream order and profiling
def test_two_calls_back_to_back_on_one_stream_share_a_scratch(vfy, sets):
    m = sets[65]
    b = batch(m)
    n = N
    scratch = filled(vfy.mldsa_vfy_scratch_bytes(65, n))
    ok_a, ok_b = stale(n), stale(n)
    sig_b = host(b["sig"]).copy()
    sig_b[::2, 7] ^= 0x10  # the second call: every other signature damaged in c~
    sig_b = dev(sig_b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        args = (b["pks"], b["mb"], b["mo"])
        tail = (b["cb"], b["co"], kidx_dev(b["vkidx"]))
        vfy_verify(vfy, m, *args, b["sig"], ok_a, n, *tail, scratch=scratch)
        vfy_verify(vfy, m, *args, sig_b, ok_b, n, *tail, scratch=scratch)
    s.synchronize()
    want_b = b["want"].copy()
    want_b[::2] = False
    assert ok_a.cpu().numpy().astype(bool).tolist() == b["want"].tolist()
    assert ok_b.cpu().numpy().astype(bool).tolist() == want_b.tolist()


def test_profile_stages_carry_the_cores_names_once_per_part(vfy, hp, sets):
    m = sets[65]
    b = batch(m)
    buf = C.create_string_buffer(8192)
    _vfy_lib.check(vfy.mldsa_vfy_profile_enable(hp._h, 1))
    try:
        for n, parts in ((N, 5), (64, 1)):
            ok = vfy_verify(vfy, m, b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), b["sig"][:n].contiguous(), stale(n), n, b["cb"],
                            b["co"][:n + 1].contiguous(), kidx_dev(b["vkidx"][:n]))
            _vfy_lib.check(vfy.mldsa_vfy_profile_report(hp._h, buf, len(buf)))
            rep = json.loads(buf.value.decode())
            assert sorted(rep) == sorted(STAGES)
            for st in STAGES:
                assert rep[st]["calls"] == parts and rep[st]["ms"] > 0, (st, rep[st])
            assert host(ok)[:n].astype(bool).tolist() == b["want"][:n].tolist()
        _vfy_lib.check(vfy.mldsa_vfy_profile_report(hp._h, buf, len(buf)))
        assert json.loads(buf.value.decode()) == {}  # a report starts the record afresh
    finally:
        _vfy_lib.check(vfy.mldsa_vfy_profile_enable(hp._h, 0))


# ------------------------------------------------------------------------------------------------------------ 5: routing
def test_routing(vfy, hp, sets, monkeypatch):
    from fips204_amd import ml_dsa
    m = sets[44]
    assert sorted(ml_dsa.VFY_MIN_OPS) == [44, 65, 87]
    for pset, lo in ml_dsa.VFY_MIN_OPS.items():  # per set
        assert sets[pset].verify_route(lo - 1) == "core" and sets[pset].verify_route(lo) == "vfy"
    lo = ml_dsa.VFY_MIN_OPS[44]
    assert lo >= 1024  # far above the core's single-launch limit
    assert m.verify_route(lo - 1) == "core" and m.verify_route(lo) == "vfy" and m.verify_route(_vfy_lib.MAX_OPS) == "vfy"
    assert m.verify_route(lo, a_hat=object()) == "core" and m.verify_route(_vfy_lib.MAX_OPS + 1) == "core" and m.verify_route(0) == "core"
    # the routes run what they name: with the threshold lowered for the test, the stages of a call show up in one record only
    b = batch(m)
    monkeypatch.setattr(ml_dsa, "VFY_MIN_OPS", {44: 64, 65: 64, 87: 64})
    a_hat = m.expand_a_for_keys(b["pks"])
    stats = hp.stats()
    hp.profile_enable(True)
    core_buf, vfy_buf = C.create_string_buffer(8192), C.create_string_buffer(8192)

    def records():
        _lib.check(hp.lib.mldsa_profile_report(hp._h, core_buf, len(core_buf)))
        _vfy_lib.check(vfy.mldsa_vfy_profile_report(hp._h, vfy_buf, len(vfy_buf)))
        return json.loads(core_buf.value.decode()), json.loads(vfy_buf.value.decode())

    try:
        records()
        for n, kw, route in ((63, {}, "core"), (64, {}, "vfy"), (65, {}, "vfy"), (65, dict(a_hat=a_hat), "core")):
            assert m.verify_route(n, kw.get("a_hat")) == route
            ok = m.verify_device(b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), b["sig"][:n].contiguous(), stale(n), n, b["cb"],
                                 b["co"][:n + 1].contiguous(), kidx_dev(b["vkidx"][:n]), **kw)
            assert host(ok)[:n].astype(bool).tolist() == b["want"][:n].tolist(), (n, route)
            core_rec, vfy_rec = records()
            # either route counts as one more directly launched call in hp.stats(), and changes nothing else of it
            after = hp.stats()
            assert after["direct_calls"] + after["graph_replays"] == stats["direct_calls"] + stats["graph_replays"] + 1, (n, route)
            if route == "vfy":  # (a core call may also grow the context's workspace)
                assert {k: v for k, v in after.items() if k != "direct_calls"} == {k: v for k, v in stats.items() if k != "direct_calls"}
            stats = after
            if route == "vfy":
                assert not core_rec and sorted(vfy_rec) == sorted(STAGES) and vfy_rec["expand_a"]["calls"] == (n + PART - 1) // PART
            else:
                assert core_rec and not vfy_rec
        # HotPath's report is the sum of the two records, under one set of names
        n = 65
        m.verify_device(b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), b["sig"][:n].contiguous(), stale(n), n, b["cb"],
                        b["co"][:n + 1].contiguous(), kidx_dev(b["vkidx"][:n]))
        m.verify_device(b["pks"], b["mb"], b["mo"][:n + 1].contiguous(), b["sig"][:n].contiguous(), stale(n), n, b["cb"],
                        b["co"][:n + 1].contiguous(), kidx_dev(b["vkidx"][:n]), a_hat=a_hat)
        rep = hp.profile_report()
        # (the core runs a call of 65 ops as its single launch, stage verify_small)
        assert rep["verify_main"]["calls"] == 2 and rep["expand_a"]["calls"] == 2 and rep["verify_small"]["calls"] == 1
    finally:
        hp.profile_enable(False)
    # one scratch per MlDsa, grown on demand
    assert m._vfy_buf.numel() >= vfy.mldsa_vfy_scratch_bytes(44, 65)
    ptr = m._vfy_buf.data_ptr()
    m.verify_device(b["pks"], b["mb"], b["mo"][:65].contiguous(), b["sig"][:64].contiguous(), stale(64), 64, b["cb"], b["co"][:65].contiguous(),
                    kidx_dev(b["vkidx"][:64]))
    torch.cuda.synchronize()
    assert m._vfy_buf.data_ptr() == ptr
    assert hp.stats()["direct_calls"] + hp.stats()["graph_replays"] == stats["direct_calls"] + stats["graph_replays"] + 3
