"""tests/arith_cases.py on the CPU: every definitional reference agrees with the oracle's counterpart (which is the reference's own
algorithm: the butterfly network, the multiply-shift Decompose) wherever the reference's contracts let the oracle run, every generated
input lies inside the contract include/mldsa_hip.h states for it, the verify-arith edge cases respect the kernel's own 2^54
precondition, and the growth fixture reproduces.  The oracle does not reduce on load as the kernels do, so inputs beyond its ranges
reach it through partial_reduce32_def -- the same class mod q."""
import ctypes as C

import numpy as np
import pytest

import arith_cases as ac
from arith_cases import EXT, H, LIM, N, Q, SETS
from oracle import oracle as orc


def _canon(a):
    return np.asarray(a, dtype=np.int64) % Q


def _reduced(a):
    return ac.i32(ac.partial_reduce32_def(a))


# ------------------------------------------------------------------------------------------ NTT
def test_ntt_def_is_the_definition():
    """independent of any implementation: NTT^-1 NTT = id, and NTT turns the product in Z_q[X] / (X^256 + 1) into the pointwise one"""
    rng = np.random.default_rng(1)
    w = rng.integers(0, Q, (8, N))
    assert np.array_equal(ac.inv_ntt_def(ac.ntt_def(w)), w) and np.array_equal(ac.ntt_def(ac.inv_ntt_def(w)), w)
    a, b = rng.integers(0, Q, (2, N))
    full = np.zeros(2 * N, dtype=object)
    for i in range(N):
        full[i:i + N] += int(a[i]) * b.astype(object)
    prod = np.array([(full[i] - full[i + N]) % Q for i in range(N)], dtype=np.int64)
    assert np.array_equal(ac.ntt_def(prod), ac.ntt_def(a) * ac.ntt_def(b) % Q)
    # X -> the roots themselves, in the order of Algorithm 41: zeta^(2 brv8(i) + 1)
    x = np.zeros(N, dtype=np.int64)
    x[1] = 1
    assert ac.ntt_def(x).tolist() == [pow(ac.ZETA, 2 * ac.brv8(i) + 1, Q) for i in range(N)]


def test_ntt_defs_match_oracle():
    rng = np.random.default_rng(2)
    cases = dict(ac.ntt_inputs(rng))
    cases["uniform_many"] = rng.integers(0, Q, (2000, N))
    cases["centered"] = rng.integers(-H, H + 1, (500, N))
    cases.update(ac.ntt_edge_inputs())
    for name, w in cases.items():
        w = np.asarray(w, dtype=np.int64)
        assert np.abs(w).max() < LIM, name
        fed = _reduced(w)                       # what k_ntt / k_inv_ntt hand to their transforms
        assert np.array_equal(_canon(fed), _canon(w)), name
        assert np.array_equal(_canon(orc.ntt(fed)), ac.ntt_def(w)), name
        assert np.array_equal(orc.inv_ntt(fed), ac.inv_ntt_def(w)), name


# ------------------------------------------------------------------------------------------ reductions
def test_reduction_defs_match_oracle():
    lib = orc.lib()
    rng = np.random.default_rng(3)
    sweep = ac.reduce_sweep()
    assert 8_400_000 < sweep.size < 8_450_000 and sweep[0] == -EXT and sweep[-1] <= EXT and EXT - sweep[-1] < 509
    vals = np.concatenate([ac.reduce_edge_values(), ac.contract_values(), rng.integers(-EXT, LIM, 4000), sweep[:: 4099]])
    assert np.abs(vals).max() < LIM and vals.size > 10_000
    for fn, ref in ((lib.orc_partial_reduce32, ac.partial_reduce32_def), (lib.orc_full_reduce32, ac.full_reduce32_def),
                    (lib.orc_center_mod, ac.center_mod_def)):
        want = np.array([fn(int(v)) for v in vals], dtype=np.int64)
        assert np.array_equal(ref(vals), want), fn
    p = ac.partial_reduce32_def(sweep)
    assert np.abs(p).max() < Q and np.array_equal(p % Q, sweep % Q)
    c = ac.center_mod_def(sweep)
    assert c.min() == -H and c.max() == H and np.array_equal(c % Q, sweep % Q)
    # the breakpoints are really there: both sides of every rounding step of reduce32 occur among the edge values
    e = ac.reduce_edge_values()
    steps = (e + (1 << 22)) >> 23
    assert steps.min() == -255 and steps.max() == 255 and np.unique(steps).size == 511
    w = rng.integers(-EXT, LIM, (6, 3, N))
    assert ac.infinity_norm_def(w).tolist() == [orc.infinity_norm(ac.i32(x)) for x in w]
    for gen in (ac.norm_position_ops, ac.norm_straddle_ops):
        for ppo in (4, 7):
            w, want = gen(ppo)
            assert np.abs(w).max() < LIM and w.shape[1:] == (ppo, N)
            assert ac.infinity_norm_def(w).tolist() == want.tolist()
            assert [orc.infinity_norm(ac.i32(x)) for x in w[:: 13]] == want[:: 13].tolist()
    w, want = ac.norm_position_ops(4)
    where = np.abs(ac.center_mod_def(w)).reshape(w.shape[0], -1).argmax(axis=1)
    assert where.tolist() == list(range(4 * N)) and np.unique(want).size == want.size   # every position once, every op another maximum


# ------------------------------------------------------------------------------------------ Montgomery-form products
def test_mont_product_defs_match_oracle():
    rng = np.random.default_rng(4)
    x = rng.integers(-67_058_538, 67_058_539, (20, N))       # the reference's to_mont contract (partial_reduce64, helpers.rs:35)
    assert np.array_equal(_canon(orc.to_mont(ac.i32(x))), ac.to_mont_def(x))
    xe = ac.to_mont_inputs(9)
    assert xe.min() == ac.I32_MIN and xe.max() == ac.I32_MAX
    inside = np.where(np.abs(xe) < 67_058_539, xe, 0)
    assert np.array_equal(_canon(orc.to_mont(ac.i32(inside))), ac.to_mont_def(inside))
    assert np.array_equal(ac.to_mont_def(xe) * ac.RINV % Q, xe % Q)
    # pointwise: |c v| < 2^31 q is mont_reduce's own contract (helpers.rs:158-159); the kernel reduces c first, the oracle does not
    c = rng.integers(-9 * Q, 9 * Q, (6, N))
    v = rng.integers(-2 * Q + 1, 2 * Q, (6, 5, N))
    got = np.stack([orc.pointwise_mont(ac.i32(c[i]), ac.i32(v[i])) for i in range(6)])
    assert np.array_equal(_canon(got), ac.pointwise_def(c, v))
    for n_ops in ac.COUNTS:
        c, v = ac.pointwise_inputs(n_ops, 3)
        assert np.abs(c).max() < LIM and v.min() >= ac.I32_MIN and v.max() <= ac.I32_MAX and c.shape == (n_ops, N) and v.shape == (n_ops, 3, N)
        cr = ac.partial_reduce32_def(c)
        assert (np.abs(cr[:, None, :] * v) < (1 << 31) * Q).all()      # mont_mul's precondition holds over the whole of int32
        got = np.stack([orc.pointwise_mont(ac.i32(cr[i]), ac.i32(v[i])) for i in range(n_ops)])
        assert np.array_equal(_canon(got), ac.pointwise_def(c, v))
    c, v = ac.pointwise_inputs(1, 3)
    pairs = {(int(a), int(b)) for p in range(3) for a, b in zip(c[0], v[0, p])}
    assert all((int(a), int(b)) in pairs for a in ac.contract_values() for b in ac.mont_operand_values())
    for pset, (k, l, _, _) in SETS.items():
        a = rng.integers(-(1 << 24) + 1, 1 << 24, (4, k, l, N))
        u = rng.integers(-8 * Q, 8 * Q, (4, l, N))
        got = np.stack([orc.mat_vec_mul(k, l, ac.i32(a[i]), ac.i32(u[i])) for i in range(4)])
        assert np.array_equal(_canon(got), ac.mat_vec_def(a, u)), pset
        for n_ops in ac.COUNTS:
            a, u = ac.mat_vec_inputs(pset, n_ops)
            assert a.shape == (n_ops, k, l, N) and u.shape == (n_ops, l, N) and np.abs(u).max() < LIM
            assert a.min() >= ac.I32_MIN and a.max() <= ac.I32_MAX
            # the kernel's term is mont_mul(a, to_mont(reduce32(u))) with to_mont's output in (-q, q): |a b| < 2^31 q for every int32 a
            assert abs(ac.I32_MIN) * (Q - 1) < (1 << 31) * Q
            # the oracle's to_mont leaves (-2q, 2q) (helpers.rs:42): its a must stay below 2^30, so it sees a mod+- q
            got = np.stack([orc.mat_vec_mul(k, l, ac.i32(ac.center_mod_def(a[i])), _reduced(u[i])) for i in range(n_ops)])
            assert np.array_equal(_canon(got), ac.mat_vec_def(a, u)), pset
        a, u = ac.mat_vec_inputs(pset, 4)
        assert (a[0] == ac.I32_MAX).all() and (a[1] == ac.I32_MIN).all() and (u[0] == EXT).all() and (u[3] == -EXT).all()


# ------------------------------------------------------------------------------------------ verify arithmetic
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verify_arith_def_matches_oracle_and_cases_respect_the_contract(pset):
    k, l, tau, _ = SETS[pset]
    rng = np.random.default_rng(5 + pset)
    n = 6
    a = rng.integers(0, Q, (n, k, l, N))
    z = rng.integers(-(1 << 19) + 1, (1 << 19) + 1, (n, l, N))
    c = np.stack([_canon(ac.challenge(rng, tau)) for _ in range(n)])
    c = np.where(c == Q - 1, -1, c)
    t1 = rng.integers(-2 * Q + 1, 2 * Q, (n, k, N))
    assert np.array_equal(orc.verify_arith(k, l, ac.i32(a), ac.i32(z), ac.i32(c), ac.i32(t1)), ac.verify_arith_def(k, l, a, z, c, t1))
    worst = 0
    cases = ac.verify_arith_cases(pset)
    assert {"a_max_growth_sparse", "a_min_growth_dense", "ext_patterns", "ext_constant", "a_canonical~plus_q", "a_canonical~minus_q"} <= set(cases)
    for name, (a, z, c, t1) in cases.items():
        assert a.shape == (ac.VA_OPS, k, l, N) and z.shape == (ac.VA_OPS, l, N) and c.shape == (ac.VA_OPS, N) and t1.shape == (ac.VA_OPS, k, N)
        assert np.abs(a).max() < ac.A_LIM and max(np.abs(z).max(), np.abs(c).max(), np.abs(t1).max()) < LIM, name
        nz = (c != 0).sum(axis=1)
        assert ((nz == tau) | (nz == N)).all() and np.isin(_canon(c), (0, 1, Q - 1)).all() and ((c % Q != 0) == (c != 0)).all(), name
        if "sparse" in name or "canonical" in name or name == "ext_constant":
            assert (nz == tau).all() and np.abs(c).max() > Q, name
        want = ac.verify_arith_def(k, l, a, z, c, t1)
        # the oracle on the same classes: it reduces nothing on load, so it gets the representatives the kernel makes of them
        # (not `mont_aligned`: the reference sums 32-bit Montgomery products and transforms the sum unreduced, ml_dsa.rs:407-416 --
        # which is exactly what that case is built to break; its definition is the composition of the references checked above)
        if name != "mont_aligned":
            got = orc.verify_arith(k, l, ac.i32(a), _reduced(z), _reduced(c), _reduced(t1))
            assert np.array_equal(got, want), name
        if "~" in name:
            assert np.array_equal(want, ac.verify_arith_def(k, l, *cases[name.split("~")[0]])), name
        # the kernel's precondition (kernels_poly.hip, "rows"): |sum_j a z_hat - c_hat' t1'| < 2^54, in Python ints, with z_hat the
        # lazy representatives of orc.ntt(reduce32(z)), |c_hat'| <= q - 1 (mont_mul's range) and t1' = reduce32(t1)
        z_hat = orc.ntt(_reduced(z)).astype(object)
        s = (a.astype(object) * z_hat[:, None, :, :]).sum(axis=2)
        tot = np.abs(s) + (Q - 1) * np.abs(ac.partial_reduce32_def(t1)).astype(object)
        worst = max(worst, int(tot.max()))
        assert int(tot.max()) < 1 << 54, name
        assert int(np.abs(z_hat).max()) < 9 * Q, name
    print(f"ML-DSA-{pset}: largest |sum| bound over the verify-arith edge cases = {worst} = {worst / 2 ** 54:.4f} * 2^54")
    a, z, _, t1 = cases["a_max_growth_sparse"]
    assert (a == ac.A_LIM - 1).all() and (z == z[:, :1]).all() and (t1[0] == Q - 1).all() and (t1[1] == 2 * Q - 1).all()
    assert (cases["a_min_growth_sparse"][0] == -(ac.A_LIM - 1)).all() and np.abs(cases["ext_patterns"][1]).min() == EXT
    assert (1023 << 13) == Q - 1
    # mont_aligned: the representative model is the oracle's mont_reduce, and L copies of the aligned product overflow an unreduced
    # inverse transform (256 L |m| > 2^31) while the 64-bit sum stays far inside the kernel's bound
    lib = orc.lib()
    p = np.concatenate([rng.integers(-(1 << 31) * Q + 1, (1 << 31) * Q, 3000), [0, 1, -1, Q, -Q, (1 << 32), (1 << 31) * Q - 1, -(1 << 31) * Q + 1]])
    assert ac.mont_repr(p).tolist() == [lib.orc_mont_reduce(int(x)) for x in p] and ac.QINV == 58728449
    a, z, _, _ = cases["mont_aligned"]
    for ax in ac.mont_aligned_a():
        m = int(ac.mont_repr(ax * H))
        assert abs(ax) < ac.A_LIM and abs(m) > 0.49 * Q and 256 * l * abs(m) > 1 << 31 and l * abs(ax) * H < 1 << 50
    assert (orc.ntt(ac.i32(z)) == z[:, :, :1]).all() and set(np.unique(a).tolist()) == set(ac.mont_aligned_a())


# ------------------------------------------------------------------------------------------ rounding
def test_power2round_def_matches_oracle_everywhere():
    r = np.arange(Q, dtype=np.int32)
    w1, w0 = np.zeros_like(r), np.zeros_like(r)
    orc.lib().orc_power2round(r.ctypes.data_as(C.c_void_p), w1.ctypes.data_as(C.c_void_p), w0.ctypes.data_as(C.c_void_p), C.c_size_t(r.size))
    r1, r0 = ac.power2round_def(r)
    assert np.array_equal(r1, w1) and np.array_equal(r0, w0)
    assert r0.min() == -(1 << 12) + 1 and r0.max() == 1 << 12 and r1.max() == 1023


@pytest.mark.parametrize("pset", [44, 65])
def test_rounding_defs_match_oracle(pset):
    lib = orc.lib()
    g2 = SETS[pset][3]
    assert g2 == orc.params(pset).gamma2
    m = (Q - 1) // (2 * g2)
    rng = np.random.default_rng(6 + pset)
    nc = ac.decompose_noncanonical(g2)
    assert np.abs(nc).max() < LIM and nc.max() > EXT - Q and nc.min() < -EXT + Q
    res = nc % Q
    assert set(((res - g2) % (2 * g2)).tolist()) >= {0, 1, 2 * g2 - 1} and {Q - 1, Q - 1 - g2} <= set(res.tolist())
    steps = nc[np.isin((res - g2) % (2 * g2), (0, 1, 2 * g2 - 1))]
    r = np.concatenate([steps, nc[:: 211], nc[-4:], rng.integers(0, Q, 3000), rng.integers(-EXT, LIM, 3000), [0, 1, Q - 1, Q - 2, -1, -Q + 1]])
    a1, a0 = C.c_int32(), C.c_int32()
    want = np.zeros((r.size, 2), dtype=np.int64)
    for i, v in enumerate(r):
        lib.orc_decompose(g2, int(v), C.byref(a1), C.byref(a0))
        want[i] = a1.value, a0.value
    r1, r0 = ac.decompose_def(g2, r)
    assert np.array_equal(r1, want[:, 0]) and np.array_equal(r0, want[:, 1])
    assert np.array_equal(ac.high_bits(g2, r), r1) and np.array_equal(ac.low_bits(g2, r), r0)
    # the whole domain, by the definition's own properties: r = r1 2 gamma2 + r0 mod q, ranges, the wrap
    a1, a0 = (x.astype(np.int64) for x in ac.decompose_all(g2))
    rr = np.arange(Q, dtype=np.int64)
    assert ((a1 * 2 * g2 + a0 - rr) % Q == 0).all() and a1.min() == 0 and a1.max() == m - 1 and a0.min() == -g2 and a0.max() == g2
    assert (a1[Q - g2:] == 0).all() and (a0[Q - g2:] == rr[Q - g2:] - Q).all() and a1[Q - g2 - 1] == m - 1 and a0[Q - g2 - 1] == g2
    # hints: the four z of the GPU sweep on sampled r, against the oracle's scalar functions
    rs = np.concatenate([np.unique(steps % Q), rng.integers(0, Q, 2000), [0, Q - 1]])
    for z in (1, Q - 1, g2, Q - g2):
        want = np.array([lib.orc_make_hint(g2, z, int(v)) for v in rs], dtype=np.int64)
        got = ac.make_hint_def(g2, z, rs)
        assert np.array_equal(got, want) and 0 < got.sum() < got.size
        # FIPS 204 Lemma: UseHint(MakeHint(z, r), r) = HighBits(r + z) for |z| <= gamma2
        assert np.array_equal(ac.use_hint_def(g2, got, rs), ac.high_bits(g2, rs + z))
    for h in (0, 1):
        hv = np.full(rs.size, h)
        assert np.array_equal(ac.use_hint_def(g2, hv, rs), orc.use_hint_vec(g2, hv, ac.i32(rs)))


# ------------------------------------------------------------------------------------------ the growth fixture
def test_growth_fixture_reproduces_and_goes_beyond_the_random_inputs():
    polys, mags = ac.growth_fixture()
    assert polys.shape == (8, N) and np.abs(polys).max() <= H
    got = np.abs(orc.ntt(ac.i32(polys)).astype(np.int64)).max(axis=1)
    assert got.tolist() == mags
    # What the older NTT tests reach.  Their inputs as k_ntt hands them to the transform (reduce32 on load), and unreduced as the oracle
    # takes them wherever they lie inside the transform's own input range |w| < q: that leaves out only `signed_lazy`, whose inputs
    # are themselves up to 9 q, so that |orc.ntt| of them (7.96 q) measures the inputs, not the growth -- no transform on the device
    # ever sees them unreduced.
    inputs = {k: np.asarray(w, dtype=np.int64) for k, w in ac.ntt_inputs(np.random.default_rng(41)).items()}
    grow = lambda w: int(np.abs(orc.ntt(ac.i32(w)).astype(np.int64)).max())  # noqa: E731
    had_reduced = max(grow(ac.partial_reduce32_def(w)) for w in inputs.values())
    had_plain = max(grow(w) for w in inputs.values() if np.abs(w).max() < Q)
    assert [k for k, w in inputs.items() if np.abs(w).max() >= Q] == ["signed_lazy"]
    print(f"growth fixture: {[round(m / Q, 3) for m in mags]} q; the random NTT inputs reach {had_reduced / Q:.3f} q as the device sees them, "
          f"{had_plain / Q:.3f} q unreduced; the header's bound is 9 q")
    assert min(mags) > max(had_reduced, had_plain) and max(mags) < 9 * Q
