"""Expected verdicts of the strict private-key import (include/mldsa_keycheck.h), restated from FIPS 204 (August 2024), and the ways a
key is damaged in tests/test_keycheck_cpu.py and tests/test_gpu_keycheck.py.

The restatement is numpy on top of the oracle's expand_a, ntt, mat_vec_mul, inv_ntt and shake: skDecode (Algorithm 25) with the
range check its lines 3 and 6 leave to the importer, t = A s1 + s2 (Algorithm 6, lines 3 and 5), Power2Round (Algorithm 35), pkEncode
(Algorithm 22) and tr = H(pk, 64) (Algorithm 6, line 9).  The oracle's sk_try_from_bytes mirrors the reference, accepts every key and
cannot serve as the expected value."""
import gzip
import json
import os

import numpy as np

from oracle import oracle as orc

Q = 8380417
D = 13
S1_RANGE, S2_RANGE, T0, TR, PK = 1, 2, 4, 8, 16
SHAPE = {44: (4, 4, 2), 65: (6, 5, 4), 87: (8, 7, 2)}  # set -> K, L, eta (FIPS 204 Table 1)
SETS = (44, 65, 87)
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acvp_keyGen.json.gz")
_PSET = {"ML-DSA-44": 44, "ML-DSA-65": 65, "ML-DSA-87": 87}


class Layout:
    """byte offsets of the sections of a wire private key: rho 32 | K 32 | tr 64 | s1 | s2 | t0 (Algorithm 24)"""

    def __init__(self, pset):
        self.pset = pset
        self.k, self.l, self.eta = SHAPE[pset]
        self.b = 3 if self.eta == 2 else 4  # bitlen(2 eta)
        self.s1 = 128
        self.s2 = self.s1 + self.l * 32 * self.b
        self.t0 = self.s2 + self.k * 32 * self.b
        self.sk_len = self.t0 + self.k * 32 * D
        self.pk_len = 32 + self.k * 320


def _fields(buf, bits):
    """the little-endian `bits`-bit fields of a byte string (BytesToBits then BitsToInteger, Algorithms 13 and 11)"""
    b = np.unpackbits(np.frombuffer(bytes(buf), dtype=np.uint8), bitorder="little").reshape(-1, bits).astype(np.int64)
    return b @ (1 << np.arange(bits, dtype=np.int64))


def _pack(values, bits):
    """SimpleBitPack with fields of `bits` bits (Algorithm 16)"""
    v = np.asarray(values, dtype=np.int64).reshape(-1, 1)
    return np.packbits(((v >> np.arange(bits)) & 1).astype(np.uint8).reshape(-1), bitorder="little").tobytes()


_MEMO = {}


def expected_flags(pset, sk, pk=None):
    """the verdict byte of one key pair: the range bits, or -- where there is none -- the consistency bits"""
    sk = bytes(sk)
    pk = None if pk is None else bytes(pk)
    memo = (pset, sk, pk)
    if memo in _MEMO:
        return _MEMO[memo]
    y = Layout(pset)
    assert len(sk) == y.sk_len and (pk is None or len(pk) == y.pk_len)
    rho, tr = sk[:32], sk[64:128]
    v1 = _fields(sk[y.s1:y.s2], y.b).reshape(y.l, 256)
    v2 = _fields(sk[y.s2:y.t0], y.b).reshape(y.k, 256)
    v0 = _fields(sk[y.t0:], D).reshape(y.k, 256)
    rng = (S1_RANGE if (v1 > 2 * y.eta).any() else 0) | (S2_RANGE if (v2 > 2 * y.eta).any() else 0)
    s1, s2 = y.eta - v1, y.eta - v2  # BitUnpack(., eta, eta): eta - field (Algorithm 19)
    a_hat = orc.expand_a(y.k, y.l, rho)
    w = orc.inv_ntt(orc.mat_vec_mul(y.k, y.l, a_hat, orc.ntt(s1.astype(np.int32)))).astype(np.int64)
    t = (w + s2) % Q
    r1 = (t + (1 << (D - 1)) - 1) >> D  # Power2Round: t = r1 2^d + r0 with r0 in (-2^(d-1), 2^(d-1)]
    r0 = t - (r1 << D)
    assert (r0 > -(1 << (D - 1))).all() and (r0 <= 1 << (D - 1)).all() and (r1 >= 0).all() and (r1 < 1 << 10).all()
    pk_prime = rho + _pack(r1, 10)
    cons = T0 if ((1 << (D - 1)) - r0 != v0).any() else 0  # BitPack(t0, 2^(d-1) - 1, 2^(d-1)): field = 2^(d-1) - r0
    cons |= TR if orc.shake(256, pk_prime, 64) != tr else 0
    cons |= PK if pk is not None and pk != pk_prime else 0
    out = rng if rng else cons
    _MEMO[memo] = out
    return out


def acvp_pairs(pset):
    """the (sk, pk) pairs of the ACVP keyGen vectors of a set"""
    with gzip.open(_GOLDEN, "rb") as f:
        groups = json.loads(f.read().decode())["testGroups"]
    return [(bytes.fromhex(t["sk"]), bytes.fromhex(t["pk"])) for g in groups if _PSET[g["parameterSet"]] == pset for t in g["tests"]]


def get_field(sk, y, vec, poly, coef):
    at, bits = (y.s1 if vec == "s1" else y.s2), y.b
    region = int.from_bytes(sk[at + poly * 32 * bits:at + (poly + 1) * 32 * bits], "little")
    return (region >> (bits * coef)) & ((1 << bits) - 1)


def set_field(sk, y, vec, poly, coef, value):
    """a copy of sk with field `coef` of polynomial `poly` of s1 / s2 set to `value`"""
    bits = y.b
    at = (y.s1 if vec == "s1" else y.s2) + poly * 32 * bits
    region = int.from_bytes(sk[at:at + 32 * bits], "little")
    region = (region & ~(((1 << bits) - 1) << (bits * coef))) | (value << (bits * coef))
    return sk[:at] + region.to_bytes(32 * bits, "little") + sk[at + 32 * bits:]


def field_places(y):
    """(vector, polynomial, coefficient): the edges of the s1 and s2 sections, where a slip flags the wrong bit; for 3-bit fields also
    coefficients 2 and 10, whose fields straddle a byte and a dword"""
    places = [("s1", 0, 0), ("s1", y.l - 1, 255), ("s2", 0, 0), ("s2", y.k - 1, 255)]
    if y.b == 3:
        places += [("s1", 1, 2), ("s1", 1, 10), ("s2", 1, 2), ("s2", 1, 10)]
    return places


def flip(buf, at, mask):
    at %= len(buf)
    return buf[:at] + bytes([buf[at] ^ mask]) + buf[at + 1:]


def damage_cases(pset, sk, pk):
    """[(name, sk', pk', stated)]: every damage class of one key pair.  `stated` is what the class gives by construction, without pk
    and with it -- a pair (flags without pk, flags with pk) --, or None where only the restatement can say (class b: a legal value
    in place of another leaves the ranges alone and may or may not move t)."""
    y = Layout(pset)
    out = []
    for vec, poly, coef in field_places(y):
        bit = S1_RANGE if vec == "s1" else S2_RANGE
        for v in (2 * y.eta + 1, (1 << y.b) - 1):  # a: the smallest and the largest illegal field
            out.append((f"a:{vec}[{poly}][{coef}]={v}", set_field(sk, y, vec, poly, coef, v), pk, (bit, bit)))
        for v in (0, 2 * y.eta):                   # b: the legal extremes
            out.append((f"b:{vec}[{poly}][{coef}]={v}", set_field(sk, y, vec, poly, coef, v), pk, None))
    out.append(("c:t0 first byte", flip(sk, y.t0, 0x01), pk, (T0, T0)))
    out.append(("c:t0 last byte", flip(sk, y.sk_len - 1, 0x80), pk, (T0, T0)))
    out.append(("d:tr", flip(sk, 64 + 37, 0x10), pk, (TR, TR)))
    out.append(("e:pk t1", sk, flip(pk, 32 + 5, 0x04), (0, PK)))
    out.append(("e:pk rho", sk, flip(pk, 3, 0x40), (0, PK)))
    out.append(("f:sk rho", flip(sk, 9, 0x02), pk, (T0 | TR, T0 | TR | PK)))
    # g: one coefficient of s1 moved inside [-eta, eta]: field v -> v + 1, or v - 1 at the upper end
    v = get_field(sk, y, "s1", y.l // 2, 77)
    assert v <= 2 * y.eta
    out.append(("g:s1 moved", set_field(sk, y, "s1", y.l // 2, 77, v + 1 if v < 2 * y.eta else v - 1), pk, (T0 | TR, T0 | TR | PK)))
    return out


def mixed_batch(pset, pairs, n, classes="abcdefg", first=0):
    """n key pairs for a device batch: intact keys (the pairs, cyclically) with the cases of the named classes dealt over the odd
    positions, from case `first` on and cyclically, so that every damaged key has intact neighbours.  n = 1: one intact key.
    Returns (sk rows, pk rows, names)."""
    sks, pks, names = [], [], []
    for i in range(n):
        sk, pk = pairs[i % len(pairs)]
        name = "intact"
        if i % 2 == 1:
            cases = [c for c in damage_cases(pset, sk, pk) if c[0][0] in classes]
            name, sk, pk, _ = cases[(first + i // 2) % len(cases)]
        sks.append(sk)
        pks.append(pk)
        names.append(name)
    return sks, pks, names
