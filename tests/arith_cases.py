"""Definitional references and contract-edge inputs for the arithmetic seams (mldsa_ntt, mldsa_inv_ntt, mldsa_to_mont, mldsa_reduce,
mldsa_rounding, mldsa_mat_vec_mul, mldsa_pointwise_mont, mldsa_infinity_norm, mldsa_verify_arith).

Not a test file, and no library is loaded here: numpy and Python ints only.  The `*_def` functions restate the operations from their
definitions in FIPS 204 -- the NTT as the evaluation of w at the 256 odd powers of zeta (a Vandermonde matrix), the rounding functions
from Algorithms 35-40 with mod+- -- and not from the kernels or the oracle, whose butterfly network and multiply-shift shortcuts they
are there to check (CPU: test_arith_cases_cpu.py compares them with the oracle, GPU: test_gpu_arith_edges.py compares the kernels with
them).  The generators produce inputs AT the contracts that include/mldsa_hip.h states, where the older tests draw random ones far
inside them."""
import functools
import json
import os

import numpy as np

Q = 8380417
N = 256
ZETA = 1753                  # FIPS 204 section 2.5: a 512th root of unity mod q
D = 13
H = (Q - 1) // 2             # the largest magnitude that survives the kernels' reduce32 on load
LIM = 2 ** 31 - 2 ** 22      # the general contract: any representative with |x| < LIM (helpers.rs:62)
EXT = LIM - 1
A_LIM = 1 << 24              # mldsa_verify_arith: |a_hat| < 2^24
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
RINV = pow(2 ** 32, -1, Q)
QINV = pow(Q, -1, 2 ** 32)   # 58728449
# set -> (K, L, tau, gamma2)
SETS = {44: (4, 4, 39, (Q - 1) // 88), 65: (6, 5, 49, (Q - 1) // 32), 87: (8, 7, 60, (Q - 1) // 32)}
COUNTS = (1, 3, 4, 5, 9)     # a lone wave, a partial block, a full block, a second block (four waves per block)
GROWTH_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_growth_inputs.json")


def _i64(a):
    return np.asarray(a, dtype=np.int64)


# ------------------------------------------------------------------------------------------ NTT (FIPS 204 section 2.5, Algorithms 41 / 42)
def brv8(i):
    return int(format(i, "08b")[::-1], 2)


@functools.lru_cache(maxsize=None)
def _vandermonde():
    """V[i][j] = zeta^((2 brv8(i) + 1) j) mod q, and its inverse with the 1/256 folded in"""
    zpow = np.array([pow(ZETA, e, Q) for e in range(512)], dtype=np.int64)
    odd = np.array([2 * brv8(i) + 1 for i in range(N)], dtype=np.int64)
    e = np.outer(odd, np.arange(N, dtype=np.int64)) % 512
    v = zpow[e]
    vinv = zpow[(512 - e.T) % 512] * pow(N, -1, Q) % Q
    return v, vinv


def ntt_def(w):
    """w_hat[i] = sum_j w[j] zeta^((2 brv8(i) + 1) j) mod q, canonical.  Products < 2^46, 256 of them < 2^54: exact in int64."""
    v, _ = _vandermonde()
    return (_i64(w) % Q) @ v.T % Q


def inv_ntt_def(w_hat):
    _, vinv = _vandermonde()
    return (_i64(w_hat) % Q) @ vinv.T % Q


# ------------------------------------------------------------------------------------------ field helpers
def partial_reduce32_def(a):
    """helpers.rs:61-67, bit-exact: a - ((a + 2^22) >> 23) q"""
    a = _i64(a)
    return a - ((a + (1 << 22)) >> 23) * Q


def full_reduce32_def(a):
    return _i64(a) % Q


def center_mod_def(a):
    """mod+-: the representative in (-q/2, q/2]"""
    t = _i64(a) % Q
    return t - (t > H) * Q


def infinity_norm_def(w):
    """max |w mod+- q| over everything but the leading axis"""
    w = _i64(w)
    return np.abs(center_mod_def(w)).reshape(w.shape[0], -1).max(axis=1)


def mont_repr(p):
    """the representative of p 2^-32 mod q that Montgomery reduction yields (helpers.rs:156-165): (p - t q) / 2^32 with
    t = p q^-1 mod+- 2^32, in (-q, q) for |p| < 2^31 q -- the one place where a representative, not a class, has to be predicted"""
    p = _i64(p)
    t = (p & 0xFFFFFFFF) * QINV & 0xFFFFFFFF
    t -= (t >> 31) << 32
    return (p - t * Q) >> 32


@functools.lru_cache(maxsize=None)
def mont_aligned_a():
    """(A+, A-): the a in [2^24 - 2^17, 2^24) whose Montgomery product with H = (q - 1) / 2 has the largest / smallest representative,
    about +-q / 2.  NTT(H X^0) is H at every index, so a constant row of A+ over z = H X^0 makes all L terms of all 256 coefficients the
    same product: their 64-bit sum L A H is tiny, but L copies of the 32-bit representative reach L q / 2 in every coefficient, and an
    inverse NTT fed with them unreduced leaves int32 (256 L q / 2 > 2^31 for L >= 4)."""
    a = np.arange(A_LIM - (1 << 17), A_LIM, dtype=np.int64)
    m = mont_repr(a * H)
    return int(a[m.argmax()]), int(a[m.argmin()])


def to_mont_def(x):
    return _i64(x) % Q * ((1 << 32) % Q) % Q


def pointwise_def(c_hat, v_hat_mont):
    """c_hat[op] o v[op][p] 2^-32 mod q (the 2^-32 of mont_reduce); c_hat [..., 256], v [..., ppo, 256]"""
    c = _i64(c_hat) % Q
    return c[..., None, :] * (_i64(v_hat_mont) % Q) % Q * RINV % Q


def mat_vec_def(a_hat, u_hat):
    """w_hat[i] = sum_j a_hat[i][j] o u_hat[j] mod q; a_hat [..., K, L, 256], u_hat [..., L, 256]"""
    a, u = _i64(a_hat) % Q, _i64(u_hat) % Q
    return (a * u[..., None, :, :] % Q).sum(axis=-2) % Q


def verify_arith_def(k, l, a_hat, z, c, t1_mont):
    """w' = NTT^-1(A_hat NTT(z) - NTT(c) o t1 2^-32) mod q, canonical; t1 in Montgomery form as in PublicKey"""
    a = _i64(a_hat).reshape(-1, k, l, N)
    n = a.shape[0]
    z_hat = ntt_def(_i64(z).reshape(n, l, N))
    c_hat = ntt_def(_i64(c).reshape(n, N))
    ct1 = pointwise_def(c_hat, _i64(t1_mont).reshape(n, k, N))
    return inv_ntt_def((mat_vec_def(a, z_hat) - ct1) % Q)


# ------------------------------------------------------------------------------------------ rounding (FIPS 204 Algorithms 35-40)
def _mod_pm(x, m):
    """x mod+- m for even m: (-m/2, m/2]"""
    t = _i64(x) % m
    return t - (t > m // 2) * m


def power2round_def(r):
    """Algorithm 35: r = r1 2^d + r0, r0 = r mod+- 2^d"""
    rp = _i64(r) % Q
    r0 = _mod_pm(rp, 1 << D)
    return (rp - r0) >> D, r0


def decompose_def(gamma2, r):
    """Algorithm 36: r = r1 (2 gamma2) + r0 with r0 = r mod+- 2 gamma2, except that r - r0 = q - 1 gives r1 = 0, r0 - 1"""
    rp = _i64(r) % Q
    r0 = _mod_pm(rp, 2 * gamma2)
    wrap = rp - r0 == Q - 1
    r1 = np.where(wrap, 0, (rp - r0) // (2 * gamma2))
    return r1, r0 - wrap


def high_bits(gamma2, r):
    return decompose_def(gamma2, r)[0]


def low_bits(gamma2, r):
    return decompose_def(gamma2, r)[1]


def make_hint_def(gamma2, z, r):
    """Algorithm 39"""
    return (high_bits(gamma2, r) != high_bits(gamma2, _i64(r) + _i64(z))).astype(np.int64)


def use_hint_def(gamma2, h, r, dec=None):
    """Algorithm 40, m = (q - 1) / (2 gamma2); dec = decompose_def(gamma2, r) where the caller has it already"""
    m = (Q - 1) // (2 * gamma2)
    r1, r0 = (_i64(x) for x in dec) if dec is not None else decompose_def(gamma2, r)
    return np.where(_i64(h) == 1, np.where(r0 > 0, (r1 + 1) % m, (r1 - 1) % m), r1)


@functools.lru_cache(maxsize=None)
def decompose_all(gamma2):
    """decompose_def of every r in [0, q), computed once: (r1, r0) as int32"""
    r1, r0 = decompose_def(gamma2, np.arange(Q, dtype=np.int64))
    return r1.astype(np.int32), r0.astype(np.int32)


# ------------------------------------------------------------------------------------------ generators
def as_polys(vals):
    """a flat list of coefficients as int32 [n][256], the last polynomial padded with zeros"""
    v = _i64(vals).ravel()
    assert v.min() >= I32_MIN and v.max() <= I32_MAX
    out = np.zeros(-(-v.size // N) * N, dtype=np.int32)
    out[:v.size] = v
    return out.reshape(-1, N)


def rep_ends(r):
    """r + k q for the smallest and the largest k that keep it inside the general contract: the contract's ends of r's class"""
    r = _i64(r)
    return np.stack([r + (-EXT - r + Q - 1) // Q * Q, r + (EXT - r) // Q * Q])


def sign_patterns():
    """name -> +-1 [256]: all +, all -, and the signs alternating with period 1, 2, ..., 128 = the butterfly strides"""
    j = np.arange(N)
    out = {"plus": np.ones(N, dtype=np.int64), "minus": -np.ones(N, dtype=np.int64)}
    for p in (1, 2, 4, 8, 16, 32, 64, 128):
        out[f"alt{p}"] = 1 - 2 * ((j // p) & 1).astype(np.int64)
    return out


def ntt_inputs(rng):
    """the random classes of test_gpu_poly.py"""
    cases = {
        "uniform": rng.integers(0, Q, (37, 256)),
        "zero": np.zeros((1, 256)),
        "q_minus_1": np.full((1, 256), Q - 1),   # k_ntt / k_inv_ntt reduce32 on load: this is -1 from there on, not a large magnitude
        "eta": rng.integers(-4, 5, (3, 256)),
        "gamma1": rng.integers(-(1 << 19) + 1, (1 << 19) + 1, (5, 256)),
        "gamma1_edges": np.where(rng.integers(0, 2, (2, 256)) == 1, 1 << 19, -(1 << 19) + 1),
        "t0": rng.integers(-(1 << 12) + 1, (1 << 12) + 1, (2, 256)),
        "signed_lazy": rng.integers(-9 * Q, 9 * Q, (4, 256)),
    }
    c = np.zeros((2, 256), dtype=np.int64)
    for r in range(2):
        pos = rng.choice(256, 49, replace=False)
        c[r, pos] = rng.choice([-1, 1], 49)
    cases["challenge"] = c
    return cases


def growth_fixture():
    """tools/search_ntt_growth.py's polynomials: (int64 [8][256] with |w| <= H, the |orc.ntt(w)| maximum each was recorded with)"""
    with open(GROWTH_JSON) as f:
        d = json.load(f)
    return np.array(d["polys"], dtype=np.int64), [int(m) for m in d["max_abs_ntt"]]


def ntt_edge_inputs():
    """name -> int64 [n][256] for mldsa_ntt / mldsa_inv_ntt, every value inside |w| < LIM"""
    eye = np.eye(N, dtype=np.int64)
    pats = np.stack(list(sign_patterns().values()))
    out = {"unit_plus": eye, "unit_minus": -eye, "unit_H": H * eye}
    for name, mag in (("H", H), ("ext", EXT), ("q_minus_1", Q - 1), ("q", Q), ("q_plus_1", Q + 1)):
        out["signs_" + name] = mag * pats
    out["growth"] = growth_fixture()[0]
    return out


def reduce_edge_values():
    """every k q + d and every k 2^23 - 2^22 + d (reduce32's own rounding breakpoints) inside the contract, d in -2 .. 2, and the ends"""
    d = np.arange(-2, 3, dtype=np.int64)
    kq = np.arange(-(LIM // Q) - 1, LIM // Q + 2, dtype=np.int64)[:, None] * Q + d
    kb = np.arange(-257, 258, dtype=np.int64)[:, None] * (1 << 23) - (1 << 22) + d
    v = np.concatenate([kq.ravel(), kb.ravel(), [EXT, -EXT]])
    return v[np.abs(v) < LIM]


def reduce_sweep():
    """a = -LIM + 1 + 509 i over the whole contract: about 8.4 M values"""
    return np.arange(-EXT, LIM, 509, dtype=np.int64)


def decompose_noncanonical(gamma2):
    """representatives at the contract's ends of the residues where Decompose can go wrong: r = gamma2 + {-1, 0, 1} mod 2 gamma2 (r0
    changes sign, r1 steps) and the wrap region q - 1 - gamma2 .. q - 1"""
    m = (Q - 1) // (2 * gamma2)
    steps = (np.arange(m + 1, dtype=np.int64)[:, None] * 2 * gamma2 + gamma2 + np.arange(-1, 2)).ravel()
    r = np.concatenate([steps[(steps >= 0) & (steps < Q)], np.arange(Q - 1 - gamma2, Q, dtype=np.int64)])
    return rep_ends(r).ravel()


def norm_position_ops(ppo):
    """ppo * 256 ops of ppo polynomials: op p * 256 + i has its maximum at coefficient i of polynomial p, a different maximum per op,
    given as a non-canonical representative; everything else stays below 1000 in magnitude.  -> (int64 [n][ppo][256], norms [n])"""
    rng = np.random.default_rng(17 + ppo)
    n = ppo * N
    w = rng.integers(-999, 1000, (n, ppo, N))
    w += rng.integers(-3, 4, w.shape) * Q
    op = np.arange(n)
    want = 1000 + op * 4001 % (H - 1000)
    sign = 1 - 2 * (op & 1)
    w[op, op // N, op % N] = sign * want + (op % 5 - 2) * Q
    return w, want


def norm_straddle_ops(ppo):
    """one op per value: the value alone in an otherwise zero op, then an all-zero op.  Values straddle the centre of mod+-, each at
    both ends of the contract.  -> (int64 [n][ppo][256], norms [n])"""
    vals = rep_ends([H, H + 1, Q - 1, Q, -Q, -H]).ravel()
    w = np.zeros((vals.size + 1, ppo, N), dtype=np.int64)
    i = np.arange(vals.size)
    w[i, (i * 3) % ppo, (i * 37 + 5) % N] = vals
    return w, np.append(np.abs(center_mod_def(vals)), 0)


def mont_operand_values():
    """the ends of what a 32-bit operand of mont_mul may be when the other one lies in (-q, q): the whole of int32"""
    return np.array([I32_MIN, I32_MIN + 1, -EXT, -Q, -H - 1, -H, -1, 0, 1, H, H + 1, Q - 1, Q, Q + 1, A_LIM - 1, EXT, I32_MAX - 1, I32_MAX],
                    dtype=np.int64)


def contract_values():
    """the ends of the general contract |x| < LIM, the centre, and the multiples of q next to them"""
    v = np.array([-EXT, -EXT + 1, -2 * Q + 1, -Q - 1, -Q, -Q + 1, -H - 1, -H, -1, 0, 1, H, H + 1, Q - 1, Q, Q + 1, 2 * Q - 1, EXT - 1, EXT],
                 dtype=np.int64)
    return np.concatenate([v, rep_ends([0, 1, Q - 1, H, H + 1]).ravel()])


def to_mont_inputs(n_polys):
    rng = np.random.default_rng(23)
    vals = np.concatenate([mont_operand_values(), contract_values(), rng.integers(I32_MIN, I32_MAX + 1, n_polys * N)])
    return vals[:n_polys * N].reshape(n_polys, N)


def pointwise_inputs(n_ops, ppo):
    """c_hat [n_ops][256] at the ends of the general contract (the kernel reduces it), v [n_ops][ppo][256] over the whole of int32
    (its range follows from |c v| < 2^31 q with |c| < q); every pair of edge values meets once in op 0, constant-sign ops after it"""
    rng = np.random.default_rng(29)
    cv, vv = contract_values(), mont_operand_values()
    c = rng.integers(-EXT, LIM, (n_ops, N))
    v = rng.integers(I32_MIN, I32_MAX + 1, (n_ops, ppo, N))
    # op 0: c cycles through the contract values in whole runs, polynomial p of v holds one operand value per run and starts where
    # polynomial p - 1 stopped: with ppo >= 3 every pair occurs
    idx = np.arange(N)
    c[0] = cv[idx % cv.size]
    for p in range(ppo):
        v[0, p] = vv[(idx // cv.size + p * (N // cv.size)) % vv.size]
    for op, (sc, sv) in zip(range(1, n_ops), ((1, 1), (1, -1), (-1, 1), (-1, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))):
        c[op] = sc * EXT
        v[op] = I32_MAX if sv > 0 else I32_MIN
    return c, v


def mat_vec_inputs(pset, n_ops):
    """a_hat [n_ops][K][L][256] over the whole of int32 (mont_mul's other operand is to_mont's output in (-q, q)), u_hat [n_ops][L][256]
    at the ends of the general contract.  Ops 0 .. 3 are constant: every one of a row's L terms is the same product, all + or all -;
    the later ops mix the edge values"""
    k, l, _, _ = SETS[pset]
    rng = np.random.default_rng(31 + pset)
    av, uv = mont_operand_values(), contract_values()
    a = av[rng.integers(0, av.size, (n_ops, k, l, N))]
    u = uv[rng.integers(0, uv.size, (n_ops, l, N))]
    for op, (ca, cu) in zip(range(n_ops), ((I32_MAX, EXT), (I32_MIN, EXT), (I32_MAX, -EXT), (I32_MIN, -EXT))):
        a[op], u[op] = ca, cu
    return a, u


def challenge(rng, tau, dense=False):
    """c with exactly tau non-zeros (or all 256), each +-1 + k q at the contract's ends or next to zero"""
    c = np.zeros(N, dtype=np.int64)
    pos = np.arange(N) if dense else rng.choice(N, tau, replace=False)
    s = rng.choice([-1, 1], pos.size)
    ends = rep_ends(s)
    pick = rng.integers(0, 3, pos.size)
    c[pos] = np.where(pick == 0, s, np.where(pick == 1, ends[0], ends[1]))
    return c


VA_OPS = 5


def verify_arith_cases(pset):
    """name -> (a_hat [5][K][L][256], z [5][L][256], c [5][256], t1 [5][K][256]), int64, every value inside mldsa_verify_arith's
    contract: |a| < 2^24, z / c / t1 any representative with |x| < LIM.  A case named `x~y` must give the same w' as case `x`."""
    k, l, tau, _ = SETS[pset]
    rng = np.random.default_rng(300 + pset)
    g, _ = growth_fixture()
    pats = list(sign_patterns().values())
    n = VA_OPS
    zg = np.repeat(g[:n, None, :], l, axis=1)                                   # the same high-growth polynomial in all L rows
    c_sparse = np.stack([challenge(rng, tau) for _ in range(n)])
    c_dense = np.stack([challenge(rng, tau, dense=True) for _ in range(n)])
    t1_edge = np.stack([np.full((k, N), v) for v in (Q - 1, 2 * Q - 1, -(2 * Q - 1), EXT, -EXT)])
    out = {}
    # a at the end of its contract, constant: the row sum is L a z_hat, nothing cancels
    for name, av in (("a_max", A_LIM - 1), ("a_min", -(A_LIM - 1))):
        a = np.full((n, k, l, N), av, dtype=np.int64)
        out[name + "_growth_sparse"] = (a, zg, c_sparse, t1_edge)
        out[name + "_growth_dense"] = (a, -zg, c_dense, t1_edge[::-1].copy())
    # z and t1 at the ends of the general contract under the butterfly strides' sign patterns
    a = np.full((n, k, l, N), A_LIM - 1, dtype=np.int64)
    a[1::2] = -(A_LIM - 1)
    z = np.stack([np.stack([EXT * pats[(op + j) % len(pats)] for j in range(l)]) for op in range(n)])
    t1 = np.stack([np.stack([EXT * pats[(op + 2 * i + 1) % len(pats)] for i in range(k)]) for op in range(n)])
    out["ext_patterns"] = (a, z, c_dense, t1)
    zc = np.stack([np.full((l, N), s * EXT) for s in (1, -1, 1, -1, 1)])
    out["ext_constant"] = (a, zc, c_sparse, np.stack([np.full((k, N), s * EXT) for s in (1, 1, -1, -1, 1)]))
    # every term of every coefficient the same Montgomery product at +-q / 2 (mont_aligned_a): a 64-bit row sum is what keeps this small
    ap, am = mont_aligned_a()
    a = np.stack([np.full((k, l, N), ap if op % 2 == 0 else am) for op in range(n)])
    zu = np.zeros((n, l, N), dtype=np.int64)
    zu[:, :, 0] = H
    zu[3:] *= -1
    out["mont_aligned"] = (a, zu, c_sparse, np.full((n, k, N), Q - 1, dtype=np.int64))
    # canonical a against a + q (still below 2^24) and a - q: the same w'
    a = rng.integers(0, Q, (n, k, l, N))
    z = rng.integers(-EXT, LIM, (n, l, N))
    t1 = np.where(rng.integers(0, 2, (n, k, N)) == 1, Q - 1, rng.integers(-2 * Q + 1, 2 * Q, (n, k, N)))
    out["a_canonical"] = (a, z, c_sparse, t1)
    out["a_canonical~plus_q"] = (a + Q, z, c_sparse, t1)
    out["a_canonical~minus_q"] = (a - Q, z, c_sparse, t1)
    out["a_canonical~mixed_q"] = (a + rng.integers(-1, 2, a.shape) * Q, z, c_sparse, t1)
    return out


def i32(a):
    a = _i64(a)
    assert a.min() >= I32_MIN and a.max() <= I32_MAX
    return np.ascontiguousarray(a, dtype=np.int32)
