"""The arithmetic seams at the edges of their contracts, against the definitional references of tests/arith_cases.py (the NTT as a
Vandermonde matrix, the rounding functions from FIPS 204 Algorithms 35-40 with mod+-) instead of the oracle, which is the same
algorithm as the kernels.  Inputs sit AT what include/mldsa_hip.h allows: the largest magnitudes that survive reduce32 on load, one
input position at a time, the butterfly strides' sign patterns, the searched high-growth polynomials, every residue of [0, q) for the
rounding functions, reduce32's own breakpoints, constant-sign rows at |a| = 2^24 - 1 for the 64-bit row sums.  Counts 1, 3, 4, 5, 9:
a lone wave, a partial block, a full block, a second block (every kernel here runs four waves per block).  test_arith_cases_cpu.py
holds the references against the oracle and the inputs against the contracts."""
import arith_cases as ac
from arith_cases import COUNTS, EXT, H, N, Q, SETS
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


def d32(a):
    return dev(ac.i32(a))


def _mixed_polys():
    """nine polynomials of different edge classes for the count runs"""
    e = ac.ntt_edge_inputs()
    return np.concatenate([e["growth"][:2], e["signs_ext"][[0, 1, 4]], e["signs_H"][[2, 9]], e["unit_H"][[255]], e["signs_q_plus_1"][[3]]])


# ------------------------------------------------------------------------------------------ NTT / inverse NTT
def test_ntt_edges_match_the_definition(hp):
    for name, w in ac.ntt_edge_inputs().items():
        got = host(hp.ntt(d32(w))).astype(np.int64)
        assert np.abs(got).max() < 9 * Q, name                      # the header's representative range
        bad = np.nonzero((got % Q != ac.ntt_def(w)).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8])


def test_inv_ntt_edges_match_the_definition_canonically(hp):
    for name, w in ac.ntt_edge_inputs().items():
        got = host(hp.inv_ntt(d32(w))).astype(np.int64)
        bad = np.nonzero((got != ac.inv_ntt_def(w)).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8])


def test_ntt_counts_and_in_place(hp):
    w = _mixed_polys()
    fwd, inv = ac.ntt_def(w), ac.inv_ntt_def(w)
    for n in COUNTS:
        assert np.array_equal(host(hp.ntt(d32(w[:n]))).astype(np.int64) % Q, fwd[:n]), n
        assert np.array_equal(host(hp.inv_ntt(d32(w[:n]))), inv[:n]), n
        x = d32(w[:n])
        assert hp.ntt(x, out=x) is x
        got = host(x).astype(np.int64)
        assert np.abs(got).max() < 9 * Q and np.array_equal(got % Q, fwd[:n]), n
        x = d32(w[:n])
        hp.inv_ntt(x, out=x)
        assert np.array_equal(host(x), inv[:n]), n
    # how large the growth polynomials come out on the device (only the class mod q and the 9 q are contract: printed, not pinned)
    g, mags = ac.growth_fixture()
    print("device max |ntt| of the growth polynomials, in q:", np.round(np.abs(host(hp.ntt(d32(g))).astype(np.int64)).max(axis=1) / Q, 3).tolist(),
          "-- the fixture's:", np.round(np.array(mags) / Q, 3).tolist())


# ------------------------------------------------------------------------------------------ mldsa_reduce
REDUCE = {"partial": ac.partial_reduce32_def, "full": ac.full_reduce32_def, "center": ac.center_mod_def}


@pytest.mark.parametrize("kind", list(REDUCE))
def test_reduce_breakpoints_and_sweep(hp, kind):
    """bit-exact for partial_reduce32, value-exact for the two whose value is determined: every k q + d and every rounding breakpoint
    k 2^23 - 2^22 + d of reduce32 inside the contract, its ends, and a = -lim + 1 + 509 i over all of it"""
    fn = getattr(hp, {"partial": "partial_reduce32", "full": "full_reduce32", "center": "center_mod"}[kind])
    edges = ac.reduce_edge_values()
    assert np.array_equal(host(fn(dev(ac.as_polys(edges)))).ravel()[:edges.size], REDUCE[kind](edges))
    for n in COUNTS:
        v = ac.as_polys(edges[37:37 + n * N])
        assert np.array_equal(host(fn(dev(v))), REDUCE[kind](v)), n
    sweep = ac.reduce_sweep()
    got = host(fn(dev(ac.as_polys(sweep)))).ravel()[:sweep.size]
    bad = np.nonzero(got != REDUCE[kind](sweep))[0]
    assert bad.size == 0, (kind, sweep[bad[:8]], got[bad[:8]])


# ------------------------------------------------------------------------------------------ mldsa_rounding
@pytest.fixture(scope="module")
def residues():
    """every r in [0, q), the last polynomial padded with zeros: (host int64, device int32)"""
    r = ac.as_polys(np.arange(Q, dtype=np.int64))
    return r.astype(np.int64), dev(r)


def _mismatch(got, want, r):
    bad = np.nonzero(np.asarray(got).ravel() != np.asarray(want).ravel())[0]
    return bad.size, r.ravel()[bad[:8]]


def test_power2round_every_residue(hp, residues):
    from fips204_amd import _lib
    r, r_dev = residues
    r1, r0 = hp.rounding(44, _lib.ROUND_POWER2ROUND, r_dev)
    w1, w0 = ac.power2round_def(r)
    assert _mismatch(host(r1), w1, r)[0] == 0 and _mismatch(host(r0), w0, r)[0] == 0


@pytest.mark.parametrize("pset", [44, 65])
def test_decompose_every_residue(hp, residues, pset):
    from fips204_amd import _lib
    r, r_dev = residues
    g2 = SETS[pset][3]
    a1, a0 = ac.decompose_all(g2)
    w1, w0 = a1[r], a0[r]
    for name, x in (("canonical", r_dev), ("r - q", r_dev - Q)):
        r1, r0 = hp.rounding(pset, _lib.ROUND_DECOMPOSE, x)
        n1, at1 = _mismatch(host(r1), w1, r)
        n0, at0 = _mismatch(host(r0), w0, r)
        assert n1 == 0 and n0 == 0, (name, n1, at1, n0, at0)
        assert torch.equal(hp.rounding(pset, _lib.ROUND_HIGH_BITS, x), r1) and torch.equal(hp.rounding(pset, _lib.ROUND_LOW_BITS, x), r0), name


@pytest.mark.parametrize("pset", [44, 65])
def test_decompose_boundary_residues_at_the_contract_ends(hp, pset):
    from fips204_amd import _lib
    g2 = SETS[pset][3]
    v = ac.decompose_noncanonical(g2)
    a1, a0 = ac.decompose_all(g2)
    x = dev(ac.as_polys(v))
    r1, r0 = (host(t).ravel()[:v.size] for t in hp.rounding(pset, _lib.ROUND_DECOMPOSE, x))
    assert _mismatch(r1, a1[v % Q], v)[0] == 0 and _mismatch(r0, a0[v % Q], v)[0] == 0
    w1, w0 = ac.decompose_def(g2, v[:: 97])           # and the definition itself on the representatives, not through the table
    assert np.array_equal(r1[:: 97], w1) and np.array_equal(r0[:: 97], w0)
    assert np.array_equal(host(hp.rounding(pset, _lib.ROUND_HIGH_BITS, x)).ravel()[:v.size], r1)
    assert np.array_equal(host(hp.rounding(pset, _lib.ROUND_LOW_BITS, x)).ravel()[:v.size], r0)
    for n in COUNTS:
        xs = ac.as_polys(v[11:11 + n * N])
        r1, r0 = hp.rounding(pset, _lib.ROUND_DECOMPOSE, dev(xs))
        assert np.array_equal(host(r1), a1[xs % Q]) and np.array_equal(host(r0), a0[xs % Q]), n


@pytest.mark.parametrize("pset", [44, 65])
def test_use_hint_every_residue(hp, residues, pset):
    from fips204_amd import _lib
    r, r_dev = residues
    g2 = SETS[pset][3]
    a1, a0 = ac.decompose_all(g2)
    dec = (a1[r], a0[r])
    for h in (0, 1):
        got = host(hp.rounding(pset, _lib.ROUND_USE_HINT, torch.full_like(r_dev, h), r_dev))
        n, at = _mismatch(got, ac.use_hint_def(g2, np.full(r.shape, h), r, dec=dec), r)
        assert n == 0, (h, n, at)


@pytest.mark.parametrize("pset", [44, 65])
def test_make_hint_every_residue_and_the_lemma(hp, residues, pset):
    """MakeHint for z = +-1 and +-gamma2 (as 1, q - 1, gamma2, q - gamma2) on every r, and FIPS 204's lemma on the same data, computed
    on the device: UseHint(MakeHint(z, r), r) = HighBits(r + z) for |z| <= gamma2"""
    from fips204_amd import _lib
    r, r_dev = residues
    g2 = SETS[pset][3]
    hb = ac.decompose_all(g2)[0]
    for z in (1, Q - 1, g2, Q - g2):
        z_dev = torch.full_like(r_dev, z)
        h = hp.rounding(pset, _lib.ROUND_MAKE_HINT, z_dev, r_dev)
        want = (hb[r] != hb[(r + z) % Q]).astype(np.int32)       # Algorithm 39 on the table of HighBits
        n, at = _mismatch(host(h), want, r)
        assert n == 0 and 0 < int(want.sum()) < want.size, (z, n, at)
        lhs = hp.rounding(pset, _lib.ROUND_USE_HINT, h, r_dev)
        rhs = hp.rounding(pset, _lib.ROUND_HIGH_BITS, r_dev + z)
        assert torch.equal(lhs, rhs), z
        assert _mismatch(host(rhs), hb[(r + z) % Q], r)[0] == 0, z
    rs = r.ravel()[:: 4001]
    assert np.array_equal(ac.make_hint_def(g2, g2, rs), (hb[rs] != hb[(rs + g2) % Q]).astype(np.int64))


# ------------------------------------------------------------------------------------------ mldsa_infinity_norm
@pytest.mark.parametrize("ppo", [4, 7])
def test_infinity_norm_positions_and_centre(hp, ppo):
    w, want = ac.norm_position_ops(ppo)         # the maximum at each of the 256 positions of each polynomial, one op per position
    got = host(hp.infinity_norm(d32(w), ppo))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    w, want = ac.norm_straddle_ops(ppo)         # (q - 1) / 2, (q + 1) / 2, q - 1, q, -q, -(q - 1) / 2 at the contract's ends; an all-zero op
    assert want[-1] == 0 and H in want.tolist() and 1 in want.tolist()
    assert host(hp.infinity_norm(d32(w), ppo)).tolist() == want.tolist()
    for n in COUNTS:
        assert host(hp.infinity_norm(d32(w[3:3 + n]), ppo)).tolist() == want[3:3 + n].tolist(), n
    assert np.array_equal(ac.infinity_norm_def(w), want)


# ------------------------------------------------------------------------------------------ to_mont, pointwise_mont, mat_vec_mul, add
def test_to_mont_over_the_whole_of_int32(hp):
    for n in COUNTS:
        x = ac.to_mont_inputs(n)
        got = host(hp.to_mont(d32(x))).astype(np.int64)
        assert np.abs(got).max() < Q and np.array_equal(got % Q, ac.to_mont_def(x)), n


def test_pointwise_mont_at_the_operand_extremes(hp):
    for n, ppo in [(n, 3) for n in COUNTS] + [(2, 1), (3, 7)]:
        c, v = ac.pointwise_inputs(n, ppo)
        got = host(hp.pointwise_mont(d32(c), d32(v))).astype(np.int64)
        assert np.abs(got).max() < Q and np.array_equal(got % Q, ac.pointwise_def(c, v)), (n, ppo)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_mat_vec_mul_at_the_operand_extremes(hp, pset):
    l = SETS[pset][1]
    for n in COUNTS:
        a, u = ac.mat_vec_inputs(pset, n)
        got = host(hp.mat_vec_mul(pset, d32(a), d32(u))).astype(np.int64)
        assert np.abs(got).max() < l * Q, n                          # the header's output range
        assert np.array_equal(got % Q, ac.mat_vec_def(a, u)), n
    # constant-sign rows: every one of the L terms is the same product, nothing cancels
    a, u = ac.mat_vec_inputs(pset, 4)
    got = host(hp.mat_vec_mul(pset, d32(a), d32(u))).astype(np.int64)
    for op in range(4):
        assert np.unique(got[op]).size == 1 and got[op, 0, 0] % l == 0 and got[op, 0, 0] != 0, op     # L times one term in (-q, q)


def test_add_vector_ntt_does_not_reduce(hp):
    rng = np.random.default_rng(8)
    a = rng.integers(ac.I32_MIN // 2, ac.I32_MAX // 2, (5, N))
    b = rng.integers(ac.I32_MIN // 2, ac.I32_MAX // 2, (5, N))
    a[0, :4], b[0, :4] = [ac.I32_MAX, ac.I32_MIN, ac.I32_MAX - 7, EXT], [0, 0, 7, -EXT]
    assert np.array_equal(host(hp.add_vector_ntt(d32(a), d32(b))), a + b)


# ------------------------------------------------------------------------------------------ mldsa_verify_arith
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verify_arith_at_the_contract_edges(hp, pset):
    """|a| = 2^24 - 1 in constant-sign rows over the same high-growth z (the 64-bit row sum is L a z_hat, up to a quarter of the 2^54 the
    kernel allows itself), a +- q for canonical a, z and t1 at +-(2^31 - 2^22 - 1), c as +-1 + k q
    with tau or 256 non-zeros, t1 = q - 1 and +-(2 q - 1), every term the same Montgomery product at +-q / 2 (which only a wide row sum
    survives): five ops a case, canonical output equal to the definition"""
    k, l, _, _ = SETS[pset]
    outs = {}
    for name, (a, z, c, t1) in ac.verify_arith_cases(pset).items():
        got = host(hp.verify_arith(pset, d32(a), d32(z), d32(c), d32(t1)))
        assert got.shape == (ac.VA_OPS, k, N) and got.min() >= 0 and got.max() < Q, name
        bad = np.argwhere((got != ac.verify_arith_def(k, l, a, z, c, t1)).any(axis=2))
        assert bad.size == 0, (name, bad[:8])
        outs[name] = got
    for name, got in outs.items():
        if "~" in name:
            assert np.array_equal(got, outs[name.split("~")[0]]), name
    # the counts, on the case with the largest row sums
    a, z, c, t1 = ac.verify_arith_cases(pset)["a_max_growth_sparse"]
    for n in (1, 3, 4):
        assert np.array_equal(host(hp.verify_arith(pset, d32(a[:n]), d32(z[:n]), d32(c[:n]), d32(t1[:n]))), outs["a_max_growth_sparse"][:n]), n
