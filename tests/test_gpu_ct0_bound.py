"""The signer's ||c t0||inf < gamma2 test (FIPS 204 Algorithm 7, ml_dsa.rs:312) on every device route, with keys whose t0 makes it DECIDE
signatures (tests/ct0_cases.py; the inputs themselves are checked by tests/test_ct0_cases_cpu.py).

The device has the test four times: tail_attempt (k_sign_tail / k_resolve, csrc/kernels_sign.hip) works from d = c t0 - c s2, accepts on
max|d| + beta < gamma2 and only otherwise transforms c t0 itself (an out-of-range s2 gives c t0 directly, no beta); resolve_coop4 is the
same on four waves inside k_sign_back_small (small calls, in rounds planned at <= 2 560 candidate slots); small calls with
MLDSA_OPT_SMALL_FUSED = 0 run the batch kernels at small sizes; k_accept
(mu/mu.hip) compares |c t0| itself.  For ML-DSA-65 / 87 it is compiled out on tau * 2^12 < gamma2.  On honest keys it fires in ~1e-7
of the attempts: a wrong comparison, a dropped beta or an exact branch that always rejects changed no test result before this file.

Every assertion is byte equality with the oracle's signature on EVERY op of the route's batch, together with the class-size conditions
(ct0_cases.CONDITIONS) on the ops that route signs."""
from gpu_common import *  # noqa: F401,F403
from gpu_common import dev, host, np, orc, pytest, torch

import ct0_cases as cc
from fips204_amd import _lib
from fips204_amd.ml_dsa import MODE_PURE, _cat_with_offsets, external_mu

pytestmark = pytest.mark.gpu

_DEV = {}


def device_batch(m, pset):
    """the set's batch resident on the device (shared by the tests of this module; nothing in it is written)"""
    if pset not in _DEV:
        b = cc.batch(pset)
        sk = np.frombuffer(b"".join(b["keys"]), dtype=np.uint8).reshape(len(b["keys"]), -1)
        sks = m.private_keys_from_bytes(dev(sk))
        mb, mo = _cat_with_offsets(b["msgs"], m.device)
        rn = dev(np.frombuffer(b"".join(b["rnd"]), dtype=np.uint8).reshape(b["n"], 32))
        kidx = dev(b["kidx"].view(np.int32))
        tr = host(sks.tr)
        mus = np.frombuffer(b"".join(external_mu(tr[k].tobytes(), x) for k, x in zip(b["kidx"], b["msgs"])), dtype=np.uint8).reshape(b["n"], 64)
        _DEV[pset] = dict(b, sk=sk, sks=sks, mb=mb, mo=mo, rn=rn, kidx_dev=kidx, mus=dev(mus))
    return _DEV[pset]


def check(pset, got, ops, route):
    """got[j] is the route's signature of op ops[j]: byte equality with the oracle on every one of them, and the class-size conditions
    on what the route signed"""
    want = cc.traced(pset)[0]
    ops = np.asarray(ops, dtype=np.int64)
    got = np.asarray(got)
    assert got.shape == (ops.size, want.shape[1]), route
    bad = ops[(got != want[ops]).any(axis=1)]
    if bad.size:
        cl = cc.classes(pset)
        names = {int(i): [c for c in cc.CLASSES if cl[c][i]] for i in bad[:12]}
        raise AssertionError(f"{route}: {bad.size} of {ops.size} signatures differ from the oracle's; first ops and their classes: {names}")
    cnt = cc.counts(pset, ops)
    print(f"ML-DSA-{pset} {route}: {ops.size} ops;", {f: {c: v for c, v in d.items() if v} for f, d in cnt.items() if any(d.values())})
    return cnt


def sign_all(m, d, **kw):
    n = d["n"]
    sig = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    m.sign_device(d["sks"], d["mb"], d["mo"], d["rn"], sig, n, key_idx=d["kidx_dev"], mode=MODE_PURE, status=st, **kw)
    assert not host(st).any()
    return host(sig)


def sign_ops(m, d, ops, hp=None):
    """one call that signs the ops `ops` of the batch (their own messages, rnd and keys).  With hp: (signatures, the call's stages as the
    library's own profile names them) -- which kernels ran the second half of its rounds is read from there, not inferred"""
    ops = [int(i) for i in ops]
    n = len(ops)
    mb, mo = _cat_with_offsets([d["msgs"][i] for i in ops], m.device)
    idx = torch.as_tensor(ops, device="cuda")
    sig = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    rn, kidx = d["rn"][idx].contiguous(), d["kidx_dev"][idx].contiguous()
    if hp is not None:
        hp.profile_enable(True)
    try:
        m.sign_device(d["sks"], mb, mo, rn, sig, n, key_idx=kidx, mode=MODE_PURE, status=st)
        torch.cuda.synchronize()
        stages = str(hp.profile_report()) if hp is not None else None
    finally:
        if hp is not None:
            hp.profile_enable(False)
    assert not host(st).any()
    return host(sig) if hp is None else (host(sig), stages)


def assert_back_half(stages, fused, what):
    """fused: EVERY round's tests ran in k_sign_back_small (resolve_coop4) -- no k_sign_tail / k_resolve launch in the call; not fused: the
    three batch kernels and no k_sign_back_small"""
    if fused:
        assert "sign_back_small" in stages and "sign_tail" not in stages and "resolve" not in stages, (what, stages[:400])
    else:
        assert "sign_tail" in stages and "resolve" in stages and "sign_back_small" not in stages, (what, stages[:400])


# ------------------------------------------------------------------------------------------------ ML-DSA-44: the large-batch routes
def test_ml_dsa_44_large_batch(hp, sets):
    """mldsa_sign at the full batch: k_sign_tail with speculative rounds through k_resolve (tail_attempt), bound first, exact on demand"""
    assert hp.get_option(_lib.OPT_SIGN_CT0_EXACT) == 0 and hp.get_option(_lib.OPT_SIGN_LANES) == 0
    m = sets[44]
    d = device_batch(m, 44)
    assert cc.unmet(check(44, sign_all(m, d), np.arange(d["n"]), "sign_device")) == []


def test_ml_dsa_44_exact_test_for_every_attempt(hp, sets):
    """MLDSA_OPT_SIGN_CT0_EXACT = 1: c t0 itself for every surviving attempt, the bound's verdict unused"""
    m = sets[44]
    d = device_batch(m, 44)
    hp.set_option(_lib.OPT_SIGN_CT0_EXACT, 1)
    try:
        got = sign_all(m, d)
    finally:
        hp.set_option(_lib.OPT_SIGN_CT0_EXACT, 0)
    assert cc.unmet(check(44, got, np.arange(d["n"]), "sign_device, CT0_EXACT = 1")) == []


def test_ml_dsa_44_two_lanes(hp, sets):
    """MLDSA_OPT_SIGN_LANES = 2: the batch (>= 8 192 ops) as two slices on two streams"""
    m = sets[44]
    d = device_batch(m, 44)
    assert d["n"] >= 8192
    hp.set_option(_lib.OPT_SIGN_LANES, 2)
    try:
        got = sign_all(m, d)
    finally:
        hp.set_option(_lib.OPT_SIGN_LANES, 0)
    assert cc.unmet(check(44, got, np.arange(d["n"]), "sign_device, SIGN_LANES = 2")) == []


def test_ml_dsa_44_cached_a(hp, sets):
    """mldsa_sign_cached_a: A_hat kept with the keys"""
    m = sets[44]
    d = device_batch(m, 44)
    got = sign_all(m, d, a_hat=m.expand_a_for_keys(d["sks"]))
    assert cc.unmet(check(44, got, np.arange(d["n"]), "mldsa_sign_cached_a")) == []


def test_ml_dsa_44_sign_host(hp, sets):
    """mldsa_sign_host: wire keys, messages and rnd in host memory, the batch in the library's own sub-batches"""
    m = sets[44]
    d = device_batch(m, 44)
    rnd = np.frombuffer(b"".join(d["rnd"]), dtype=np.uint8)
    got = m.sign_host(d["sk"], d["msgs"], rnd, key_idx=d["kidx"], mode=MODE_PURE)
    assert cc.unmet(check(44, got, np.arange(d["n"]), "sign_host")) == []


def test_ml_dsa_44_sign_from_mu(hp, sets):
    """mldsa_sign_mu (k_accept of mu/mu.hip) from mu = external_mu(tr, M): the core's signatures and the oracle's"""
    m = sets[44]
    d = device_batch(m, 44)
    n = d["n"]
    sig = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    m.sign_mu_device(d["sks"], d["mus"], d["rn"], sig, n, key_idx=d["kidx_dev"], status=st)
    assert not host(st).any()
    got = host(sig)
    assert cc.unmet(check(44, got, np.arange(n), "sign_mu_device")) == []
    assert np.array_equal(got, sign_all(m, d))


# ------------------------------------------------------------------------------------------------ ML-DSA-44: small calls
def small_calls(d):
    """Every class member of the batch in small calls, padded with neighbours in the batch.  A small call's round runs its tests in
    k_sign_back_small only if the round is PLANNED at <= 2 560 candidate slots (MLDSA_SMALL_BACK_SLOTS_MAX), else on k_sign_tail +
    k_resolve like a large batch; a class is decided in an op's first rounds, so the calls are sized for round 0: alternately
    90 members + 30 neighbours (120 ops x 19 candidates = 2 280 slots) and 48 + 16 (64 ops: the small calls' own speculation rule,
    1 024 slots).  test_ml_dsa_44_small_calls reads from the library's profile that it came out so."""
    cl = cc.classes(44)
    member = np.zeros(d["n"], dtype=bool)
    for c in cc.CLASSES:
        member |= cl[c]
    members = np.flatnonzero(member)
    calls, lo, big = [], 0, True
    while lo < members.size:
        take, size = (90, 120) if big else (48, 64)
        own = members[lo:lo + take]
        ops = [int(i) for i in own]
        have = set(ops)
        for i in own:
            if len(ops) >= size:
                break
            if int(i) + 1 < d["n"] and int(i) + 1 not in have:
                ops.append(int(i) + 1)
                have.add(int(i) + 1)
        calls.append(np.array(sorted(ops)))
        lo, big = lo + take, not big
    return members, calls


@pytest.mark.parametrize("fused", [256, 0])
def test_ml_dsa_44_small_calls(hp, sets, fused):
    """Calls of <= 120 ops holding every class member.  fused = 256 (the default): every round of every call runs its tests in
    k_sign_back_small, i.e. resolve_coop4 decides every class member -- asserted on the profile's stage names; 0: the same calls on
    k_sign_tail + k_resolve at small sizes."""
    m = sets[44]
    d = device_batch(m, 44)
    members, calls = small_calls(d)
    assert all(len(ops) <= 120 for ops in calls) and {len(ops) for ops in calls} >= {120, 64} and set(members) <= set(np.concatenate(calls))
    assert hp.get_option(_lib.OPT_SMALL_FUSED) == 256
    hp.set_option(_lib.OPT_SMALL_FUSED, fused)
    try:
        out = [sign_ops(m, d, ops, hp) for ops in calls]
    finally:
        hp.set_option(_lib.OPT_SMALL_FUSED, 256)
    for j, (_, stages) in enumerate(out):
        assert_back_half(stages, fused, (j, len(calls[j])))
    ops = np.concatenate(calls)
    cnt = check(44, np.concatenate([g for g, _ in out]), ops, f"{len(calls)} small calls of <= 120 ops, SMALL_FUSED = {fused}")
    assert cc.unmet(cnt) == [] and cnt == cc.counts(44)


def test_ml_dsa_44_one_op_calls(hp, sets):
    """the reference's call shape, one op per call (k_sign_back_small every round), for eight class members: two rejected only with
    beta in the bound, two on gamma2 itself, two accepted by c t0 proper, two of those with d alone over gamma2"""
    m = sets[44]
    d = device_batch(m, 44)
    cl = cc.classes(44)
    # (equal_gamma2 ops are reject_decided ops too and accept_needs_beta ops accept_by_exact ops: eight different ops)
    ops = np.concatenate([np.flatnonzero(cl["reject_needs_beta"] & ~cl["equal_gamma2"])[:2], np.flatnonzero(cl["equal_gamma2"])[:2],
                          np.flatnonzero(cl["accept_by_exact"] & ~cl["accept_needs_beta"])[:2], np.flatnonzero(cl["accept_needs_beta"])[:2]])
    assert np.unique(ops).size == 8
    out = [sign_ops(m, d, [i], hp) for i in ops]
    for i, (_, stages) in zip(ops, out):
        assert_back_half(stages, True, int(i))
    cnt = check(44, np.concatenate([g for g, _ in out]), ops, "1-op calls")
    assert all(sum(f[c] for f in cnt.values()) >= 2 for c in ("reject_needs_beta", "equal_gamma2", "accept_by_exact", "accept_needs_beta"))


# ------------------------------------------------------------------------------------------------ ML-DSA-65 / 87: the test compiled out
@pytest.mark.parametrize("pset", [65, 87])
def test_the_test_cannot_fail_for_ml_dsa_65_and_87(hp, sets, pset):
    """The device leaves the t0 test out for gamma2 = (q - 1) / 32 (||c t0||inf <= tau * 2^12 < gamma2); the oracle runs it.  Two rows at the
    largest encodable |t0|, one coherent row and every row coherent: the same signatures on the large route (all 1 600 ops, the honest
    key's 64 included), in a 200-op call fused and not (a small call by its prologue and round fronts; its round 0 is planned at
    200 x 19 = 3 800 candidate slots, over the 2 560 of k_sign_back_small, so k_sign_tail + k_resolve test most of its ops), in the same
    200 ops as calls of 120 and 80 (k_sign_back_small in every round, read from the profile) and from mu."""
    m = sets[pset]
    d = device_batch(m, pset)
    n = d["n"]
    assert d["slices"]["two_rows_extreme"] == (0, 1024)
    check(pset, sign_all(m, d), np.arange(n), "sign_device")
    small = np.concatenate([np.arange(0, 120), np.arange(1024, 1064), np.arange(1280, 1320)])
    assert small.size == 200 and small.max() < n
    try:
        for fused in (256, 0):
            hp.set_option(_lib.OPT_SMALL_FUSED, fused)
            check(pset, sign_ops(m, d, small), small, f"200-op call, SMALL_FUSED = {fused}")
    finally:
        hp.set_option(_lib.OPT_SMALL_FUSED, 256)
    for part in (small[:120], small[120:]):
        got, stages = sign_ops(m, d, part, hp)
        assert_back_half(stages, True, (pset, part.size))
        check(pset, got, part, f"{part.size}-op call, k_sign_back_small in every round")
    sig = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    m.sign_mu_device(d["sks"], d["mus"], d["rn"], sig, n, key_idx=d["kidx_dev"], status=st)
    assert not host(st).any()
    check(pset, host(sig), np.arange(n), "sign_mu_device")


# ------------------------------------------------------------------------------------------------ verify
def test_ml_dsa_44_verdicts_under_the_derived_public_key(hp, sets):
    """The batch's signatures under get_public_key(sk): verify and verify_mu_device give the oracle's verdicts.  t0 does not belong to
    t = A s1 + s2 for the crafted keys, so the hints are wrong and those verdicts are False; the honest family's are True: both occur."""
    m = sets[44]
    d = device_batch(m, 44)
    n = d["n"]
    sigs = cc.traced(44)[0]
    pks = m.get_public_key(d["sks"])
    pk_o = [orc.get_public_key(44, k) for k in cc.oracle_keys(44)]
    want = np.asarray(orc.verify_batch_mt(44, pk_o, d["kidx"], d["msgs"], [s.tobytes() for s in sigs], cc.THREADS, 1, mode=0), dtype=bool)
    lo, hi = d["slices"]["honest"]
    assert want[lo:hi].all() and not want[:lo].all() and want.any() and not want.all()
    d_sig = dev(sigs)
    got = m.verify(pks, d["msgs"], d_sig, key_idx=d["kidx"], mode=MODE_PURE)
    assert np.array_equal(got, want)
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    m.verify_mu_device(pks, d["mus"], d_sig, ok, n, key_idx=d["kidx_dev"])
    assert np.array_equal(host(ok).astype(bool), want)
    print("verdicts: True", int(want.sum()), "False", int((~want).sum()), "True outside the honest family", int(want[:lo].sum()))
