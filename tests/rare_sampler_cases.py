"""The rare data-dependent paths of the SHAKE-driven samplers: an independent restatement of RejNTTPoly, RejBoundedPoly,
ExpandA, ExpandS and key generation written from FIPS 204 over hashlib (no oracle, no device), the classifier that recomputes
what tests/golden/rare_sampler_seeds.json.gz claims about each seed, the quotas the fixture must keep, and the subtly wrong
samplers that serve as negative controls.  Pure Python / numpy: test_rare_sampler_seeds_cpu.py checks the fixture, the oracle and
the mutants with it, test_gpu_rare_sampler_paths.py takes its expected values from it.

Every sampler returns (coefficients, info); info says what the sampler consumed.  Candidate / half-byte indices count from the
start of the stream; a SHAKE128 block holds 56 three-byte candidates, a SHAKE256 block 272 half-bytes."""
import gzip
import hashlib
import json
import os

import numpy as np

Q = 8380417
N = 256
D = 13
SETS = {44: dict(k=4, l=4, eta=2), 65: dict(k=6, l=5, eta=4), 87: dict(k=8, l=7, eta=2)}
FIXTURE = "rare_sampler_seeds.json.gz"
A_BLOCK, A_CAND = 168, 56       # SHAKE128 rate, candidates per block
S_BLOCK, S_HALF = 136, 272      # SHAKE256 rate, half-bytes per block


def load_fixture():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", FIXTURE)
    with gzip.open(path, "rb") as f:
        return json.loads(f.read().decode())


# ------------------------------------------------------------------------------ FIPS 204 Algorithms 30, 31, 32, 33, 14, 15
def rej_ntt_poly(seed34, accept=None):
    """Algorithm 30.  accept(z, i): whether the 23-bit candidate z at candidate index i is taken (None: z < q).
    info: bytes, blocks, rejections (indices of the rejected candidates before the 256th acceptance), candidates (consumed)."""
    assert len(seed34) == 34
    accept = accept or (lambda z, i: z < Q)
    n_blocks = 5
    while True:
        s = hashlib.shake_128(bytes(seed34)).digest(n_blocks * A_BLOCK)
        out, rej = [], []
        for i in range(len(s) // 3):
            z = s[3 * i] | (s[3 * i + 1] << 8) | ((s[3 * i + 2] & 0x7F) << 16)
            if accept(z, i):
                out.append(z)
                if len(out) == N:
                    used = 3 * (i + 1)
                    return out, dict(bytes=used, blocks=-(-used // A_BLOCK), rejections=rej, candidates=i + 1)
            else:
                rej.append(i)
        n_blocks += 1


def candidates(seed34, n):
    """the first n 23-bit candidates of a RejNTTPoly stream"""
    s = hashlib.shake_128(bytes(seed34)).digest(3 * n)
    return [s[3 * i] | (s[3 * i + 1] << 8) | ((s[3 * i + 2] & 0x7F) << 16) for i in range(n)]


def coeff_from_half_byte(eta, b):
    """Algorithm 15"""
    if eta == 2 and b < 15:
        return 2 - (b % 5)
    if eta == 4 and b < 9:
        return 4 - b
    return None


def rej_bounded_poly(eta, seed66, max_blocks=None, stop_at=N):
    """Algorithm 31.  info: bytes, blocks, accepted_per_block (over every WHOLE block squeezed: what a block-wise form sees),
    last_half (index of the half-byte that gave coefficient 255).
    max_blocks / stop_at exist for the mutants below: squeeze at most that many blocks and leave the rest 0; keep consuming
    after `N` coefficients until `stop_at` half-bytes were accepted (the extra ones overwrite from coefficient 0 on)."""
    assert len(seed66) == 66
    n_blocks = 2
    while True:
        take = n_blocks if max_blocks is None else min(n_blocks, max_blocks)
        s = hashlib.shake_256(bytes(seed66)).digest(take * S_BLOCK)
        halves = [h for z in s for h in (z & 15, z >> 4)]
        per_block = [sum(coeff_from_half_byte(eta, h) is not None for h in halves[b * S_HALF:(b + 1) * S_HALF]) for b in range(take)]
        out, n_acc = [0] * N, 0
        for i, h in enumerate(halves):
            c = coeff_from_half_byte(eta, h)
            if c is None:
                continue
            out[n_acc % N] = c
            n_acc += 1
            if n_acc == stop_at:
                used = i // 2 + 1
                return out, dict(bytes=used, blocks=-(-used // S_BLOCK), accepted_per_block=per_block[:-(-used // S_BLOCK)], last_half=i)
        if max_blocks is not None and take == max_blocks:
            return out, dict(bytes=take * S_BLOCK, blocks=take, accepted_per_block=per_block, last_half=None)
        n_blocks += 1


def expand_a(pset, rho, sampler=rej_ntt_poly):
    """Algorithm 32: int32 [k, l, 256], infos [k][l]"""
    k, l = SETS[pset]["k"], SETS[pset]["l"]
    a = np.zeros((k, l, N), dtype=np.int32)
    infos = []
    for r in range(k):
        row = []
        for s in range(l):
            c, info = sampler(bytes(rho) + bytes([s, r]))
            a[r, s] = c
            row.append(info)
        infos.append(row)
    return a, infos


def expand_s(pset, rho_prime, sampler=rej_bounded_poly):
    """Algorithm 33: (s1 int32 [l, 256], s2 int32 [k, 256], infos [l + k]); stream r < l is s1[r], stream l + r is s2[r]"""
    k, l, eta = SETS[pset]["k"], SETS[pset]["l"], SETS[pset]["eta"]
    out = np.zeros((l + k, N), dtype=np.int32)
    infos = []
    for r in range(l + k):
        c, info = sampler(eta, bytes(rho_prime) + r.to_bytes(2, "little"))
        out[r] = c
        infos.append(info)
    return out[:l], out[l:], infos


def seed_split(pset, xi):
    """Algorithm 6 line 1: (rho, rho', K) = H(xi || k || l, 128)"""
    h = hashlib.shake_256(bytes(xi) + bytes([SETS[pset]["k"], SETS[pset]["l"]])).digest(128)
    return h[:32], h[32:96], h[96:]


# ------------------------------------------------------------------------------ key generation (Algorithms 6, 16, 17, 22, 24, 35, 41, 42)
def _bitrev8(x):
    return int(f"{x:08b}"[::-1], 2)


ZETAS = [pow(1753, _bitrev8(i), Q) for i in range(256)]


def ntt(w):
    """Algorithm 41 on int64 [..., 256]"""
    w = np.array(w, dtype=np.int64) % Q
    m, length = 0, 128
    while length >= 1:
        for start in range(0, N, 2 * length):
            m += 1
            t = ZETAS[m] * w[..., start + length:start + 2 * length] % Q
            w[..., start + length:start + 2 * length] = (w[..., start:start + length] - t) % Q
            w[..., start:start + length] = (w[..., start:start + length] + t) % Q
        length //= 2
    return w


def inv_ntt(w):
    """Algorithm 42"""
    w = np.array(w, dtype=np.int64) % Q
    m, length = 256, 1
    while length < N:
        for start in range(0, N, 2 * length):
            m -= 1
            lo = w[..., start:start + length].copy()
            hi = w[..., start + length:start + 2 * length].copy()
            w[..., start:start + length] = (lo + hi) % Q
            w[..., start + length:start + 2 * length] = (Q - ZETAS[m]) * (lo - hi) % Q
        length *= 2
    return w * 8347681 % Q


def _pack(vals, bits):
    """little-endian packing of non-negative integers of `bits` bits each (IntegerToBits / BitsToBytes)"""
    v = np.asarray(vals, dtype=np.int64).ravel()
    assert v.min() >= 0 and v.max() < (1 << bits)
    b = ((v[:, None] >> np.arange(bits)) & 1).astype(np.uint8).ravel()
    return np.packbits(b, bitorder="little").tobytes()


def keygen(pset, xi):
    """ML-DSA.KeyGen_internal (Algorithm 6): (pk bytes, sk bytes)"""
    k, l, eta = SETS[pset]["k"], SETS[pset]["l"], SETS[pset]["eta"]
    rho, rho_prime, cap_k = seed_split(pset, xi)
    a_hat, _ = expand_a(pset, rho)
    s1, s2, _ = expand_s(pset, rho_prime)
    s1_hat = ntt(s1)
    t_hat = (a_hat.astype(np.int64) * s1_hat[None, :, :] % Q).sum(axis=1) % Q
    t = (inv_ntt(t_hat) + s2) % Q
    r0 = t % (1 << D)
    r0 = np.where(r0 > (1 << (D - 1)), r0 - (1 << D), r0)     # mod+-: -2^12 < r0 <= 2^12
    t1 = (t - r0) >> D
    pk = rho + b"".join(_pack(t1[i], 10) for i in range(k))
    tr = hashlib.shake_256(pk).digest(64)
    eb = 3 if eta == 2 else 4
    sk = (rho + cap_k + tr + b"".join(_pack(eta - s1[i], eb) for i in range(l)) + b"".join(_pack(eta - s2[i], eb) for i in range(k))
          + b"".join(_pack((1 << (D - 1)) - r0[i], D) for i in range(k)))
    return pk, sk


# ------------------------------------------------------------------------------ classifier: the properties the fixture files seeds under
def es_profile(eta, rho_prime, stream):
    """what RejBoundedPoly(rho' || stream) consumes: accepted half-bytes in block one / in blocks one and two, the half-byte that
    fills the row"""
    _, info = rej_bounded_poly(eta, bytes(rho_prime) + int(stream).to_bytes(2, "little"))
    s = hashlib.shake_256(bytes(rho_prime) + int(stream).to_bytes(2, "little")).digest(2 * S_BLOCK)
    acc = [sum(coeff_from_half_byte(eta, h) is not None for z in s[b * S_BLOCK:(b + 1) * S_BLOCK] for h in (z & 15, z >> 4)) for b in (0, 1)]
    return dict(acc1=acc[0], acc2=acc[0] + acc[1], blocks=info["blocks"], bytes=info["bytes"], last_half=info["last_half"])


ES_PROPS = {
    # eta = 4
    "third_block": lambda p: p["acc2"] < N and p["blocks"] == 3,
    "exact_256_in_two": lambda p: p["acc2"] == N and p["blocks"] == 2,
    # eta = 2
    "b1_256": lambda p: p["acc1"] == N and p["blocks"] == 1,
    "b1_255": lambda p: p["acc1"] == N - 1 and p["blocks"] == 2,
    "b1_last_half": lambda p: p["acc1"] == N and p["last_half"] == S_HALF - 1,
}


def ea_profile(rho, r, s):
    """what RejNTTPoly(rho || s || r) consumes: rejections and the boundary candidates (z in {q - 1, q}) before the 256th acceptance"""
    seed = bytes(rho) + bytes([s, r])
    _, info = rej_ntt_poly(seed)
    z = candidates(seed, info["candidates"])
    info["boundary"] = [(i, "q" if v == Q else "q-1") for i, v in enumerate(z) if v in (Q, Q - 1)]
    return info


def _two_in_group(rej):
    g = [i // 4 for i in rej]
    return len(set(g)) < len(g)


EA_SHAPES = {
    "rej5": lambda p: len(p["rejections"]) >= 5,
    "two_in_group": lambda p: _two_in_group(p["rejections"]),
    "cand55": lambda p: any(i % A_CAND == 55 for i in p["rejections"]),
    "cand27_28": lambda p: any(i % A_CAND in (27, 28) for i in p["rejections"]),
}
EA_CELLS = [(v, pos) for v in ("q", "q-1") for pos in range(4)]


def key_streams(pset, xi):
    """the sampler inputs of a key: (rho, rho')"""
    rho, rho_prime, _ = seed_split(pset, xi)
    return rho, rho_prime


def check_entry(cat, pset, e):
    """assert that fixture entry e of category cat has the property it is filed under"""
    eta = SETS[pset]["eta"]
    if cat == "es3_keys":
        rho_prime = key_streams(pset, bytes.fromhex(e["xi"]))[1]
        assert e["streams"], e
        for st in e["streams"]:
            p = es_profile(eta, rho_prime, st["stream"])
            assert ES_PROPS["third_block"](p) and p["acc2"] == st["acc2"] and p["bytes"] > 2 * S_BLOCK, (e, p)
        every = [i for i in range(SETS[pset]["k"] + SETS[pset]["l"]) if es_profile(eta, rho_prime, i)["blocks"] == 3]
        assert every == [st["stream"] for st in e["streams"]], (e, every)
    elif cat == "es_exact_keys":
        rho_prime = key_streams(pset, bytes.fromhex(e["xi"]))[1]
        assert e["streams"], e
        for st in e["streams"]:
            assert ES_PROPS["exact_256_in_two"](es_profile(eta, rho_prime, st["stream"])), e
    elif cat in ("es3_seam", "es_edge"):
        p = es_profile(eta, bytes.fromhex(e["rho_prime"]), e["stream"])
        assert ES_PROPS[e["prop"]](p), (e, p)
        if "acc2" in e:
            assert p["acc2"] == e["acc2"], (e, p)
    elif cat == "ea_boundary":
        rho = key_streams(pset, bytes.fromhex(e["xi"]))[0]
        assert rho.hex() == e["rho"]
        p = ea_profile(rho, e["r"], e["s"])
        assert (e["cand"], e["value"]) in p["boundary"] and e["cand"] % 4 == e["pos"], (e, p["boundary"])
    elif cat == "ea_shape":
        rho = key_streams(pset, bytes.fromhex(e["xi"]))[0]
        assert rho.hex() == e["rho"]
        p = ea_profile(rho, e["r"], e["s"])
        assert EA_SHAPES[e["prop"]](p) and p["rejections"] == e["rejections"], (e, p)
    else:
        raise KeyError(cat)


def entries(fx):
    """every (category, pset, entry) of the fixture"""
    for e in fx["es3_keys"]:
        yield "es3_keys", 65, e
    for e in fx["es_exact_keys"]:
        yield "es_exact_keys", 65, e
    for e in fx["es3_seam"]:
        yield "es3_seam", 65, e
    for cat in ("es_edge", "ea_boundary", "ea_shape"):
        for pset in sorted(fx[cat]):
            for e in fx[cat][pset]:
                yield cat, int(pset), e


def check_quotas(fx):
    """the minimum content of the fixture: a regenerated file cannot thin out unnoticed"""
    ks = fx["es3_keys"]
    l = SETS[65]["l"]
    assert len(ks) >= 8
    acc2 = [st["acc2"] for e in ks for st in e["streams"]]
    idx = [st["stream"] for e in ks for st in e["streams"]]
    assert any(i < l for i in idx) and any(i >= l for i in idx), "a stream of s1 and a stream of s2"
    assert any(a == 255 for a in acc2) and any(a <= 253 for a in acc2)
    seam = fx["es3_seam"]
    assert sum(e["prop"] == "third_block" for e in seam) >= 8
    assert sum(e["prop"] == "exact_256_in_two" for e in seam) >= 2
    for pset in ("44", "87"):
        for prop in ("b1_256", "b1_255", "b1_last_half"):
            assert sum(e["prop"] == prop for e in fx["es_edge"][pset]) >= 2, (pset, prop)
    for pset in ("44", "65", "87"):
        for v, pos in EA_CELLS:
            xs = {e["xi"] for e in fx["ea_boundary"][pset] if e["value"] == v and e["pos"] == pos}
            assert len(xs) >= 2, (pset, v, pos)
        for prop in EA_SHAPES:
            xs = {e["xi"] for e in fx["ea_shape"][pset] if e["prop"] == prop}
            assert len(xs) >= 2, (pset, prop)


def ea_keys(fx, pset):
    """the distinct keygen seeds of the EA entries of a set, in file order"""
    out = []
    for cat in ("ea_boundary", "ea_shape"):
        for e in fx[cat][str(pset)]:
            if e["xi"] not in out:
                out.append(e["xi"])
    return [bytes.fromhex(x) for x in out]


def es_streams(fx, pset):
    """the distinct (rho', stream) of the ES entries of a set: seam entries, and for ML-DSA-65 the rare streams of the ES3 keys"""
    out = []
    if pset == 65:
        for e in fx["es3_seam"]:
            out.append((bytes.fromhex(e["rho_prime"]), e["stream"]))
        for e in fx["es3_keys"] + fx["es_exact_keys"]:
            rp = key_streams(65, bytes.fromhex(e["xi"]))[1]
            out += [(rp, st["stream"]) for st in e["streams"]]
    else:
        out += [(bytes.fromhex(e["rho_prime"]), e["stream"]) for e in fx["es_edge"][str(pset)]]
    return out


# ------------------------------------------------------------------------------ negative controls: subtly wrong samplers
def ntt_accepts_q(seed34):
    """RejNTTPoly accepting z <= q"""
    return rej_ntt_poly(seed34, lambda z, i: z <= Q)


def ntt_rejects_q_minus_1(seed34):
    """RejNTTPoly rejecting z >= q - 1"""
    return rej_ntt_poly(seed34, lambda z, i: z < Q - 1)


def ntt_wrong_at(pos, kind):
    """RejNTTPoly with the boundary wrong at ONE position of the group of four candidates: kind "q" accepts z = q there,
    kind "q-1" rejects z = q - 1 there -- a wrong carry bit or a constant off by one in one field of the packed comparison"""
    if kind == "q":
        return lambda seed34: rej_ntt_poly(seed34, lambda z, i: z <= Q if i % 4 == pos else z < Q)
    return lambda seed34: rej_ntt_poly(seed34, lambda z, i: z < Q - 1 if i % 4 == pos else z < Q)


def bounded_two_blocks_only(eta, seed66):
    """RejBoundedPoly that stops after two blocks and leaves the rest zero"""
    return rej_bounded_poly(eta, seed66, max_blocks=2)


def bounded_keeps_consuming(eta, seed66):
    """RejBoundedPoly that does not stop at the 256th coefficient: every accepted half-byte of the blocks it squeezed is
    written, the ones past 256 wrapping round to coefficient 0 (a lane that goes on while its wave finishes)"""
    _, info = rej_bounded_poly(eta, seed66)
    s = hashlib.shake_256(bytes(seed66)).digest(info["blocks"] * S_BLOCK)
    total = sum(coeff_from_half_byte(eta, h) is not None for z in s for h in (z & 15, z >> 4))
    return rej_bounded_poly(eta, seed66, stop_at=total)


# ------------------------------------------------------------------------------ the seeds of the GPU sampler tests as they were
def legacy_expand_a_rho():
    """(pset, rho) of test_expand_a and test_expand_a_rejection_paths in test_gpu_samplers.py"""
    out = []
    for pset in (44, 65, 87):
        for n_ops in (1, 3, 70):
            rng = np.random.default_rng(1000 + pset + n_ops)
            out += [(pset, r.tobytes()) for r in rng.integers(0, 256, (n_ops, 32), dtype=np.uint8)]
    rho = np.random.default_rng(77).integers(0, 256, (300, 32), dtype=np.uint8)
    out += [(87, rho[i].tobytes()) for i in range(0, 300, 7)]
    return out


def legacy_expand_s_rho():
    """(pset, rho') of test_expand_s in test_gpu_samplers.py"""
    out = []
    for pset in (44, 65, 87):
        rng = np.random.default_rng(2000 + pset)
        out += [(pset, r.tobytes()) for r in rng.integers(0, 256, (23, 64), dtype=np.uint8)]
    return out
