#!/usr/bin/env python3
"""Search seeds that drive the SHAKE-driven samplers of ML-DSA through branches random inputs of practical size never reach,
and write them to tests/golden/rare_sampler_seeds.json.gz (read by tests/rare_sampler_cases.py).

hashlib and numpy only: no oracle, no GPU.  Trial seeds come from fixed tags (SHAKE256(tag || i)), the search stops at the
first trial that completes every quota, and the gzip header carries no time stamp, so a rerun reproduces the file byte for byte.

  ES3        eta = 4 (ML-DSA-65): RejBoundedPoly streams that accept fewer than 256 of the 544 half-bytes of two SHAKE256 blocks and
             so squeeze a third one (about 7 in a million), as keygen seeds xi and as rho' directly; streams that accept exactly 256
  ES-edge    eta = 2: streams that accept exactly 256 / 255 half-bytes in block one, or take coefficient 255 from its last half-byte
  EA-boundary  keygen seeds whose rho has a RejNTTPoly candidate equal to q or q - 1 before the 256th acceptance, two seeds for every
             (value, candidate index mod 4)
  EA-shape   streams with >= 5 rejections, two rejections in one group of four candidates, a rejection at candidate 55 of a
             block, a rejection at candidate 27 or 28 of a block

usage: python tools/find_rare_sampler_seeds.py [--out PATH] [--check]     (--check: compare with the file's content instead of writing it)
"""
import argparse
import gzip
import hashlib
import json
import os
import sys
import time

import numpy as np

Q = 8380417
SETS = {44: (4, 4, 2), 65: (6, 5, 4), 87: (8, 7, 2)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rare_sampler_seeds.json.gz")
CHUNK = 4096


def trial(tag, i, n=32):
    return hashlib.shake_256(b"rare-sampler-seeds/" + tag + int(i).to_bytes(8, "little")).digest(n)


def split(pset, xi):
    k, l, _ = SETS[pset]
    h = hashlib.shake_256(xi + bytes([k, l])).digest(96)
    return h[:32], h[32:]


def es_counts(eta, seeds66):
    """per stream: accepted half-bytes in block one, in blocks one and two, whether the last half-byte of block one is accepted"""
    raw = np.frombuffer(b"".join(hashlib.shake_256(s).digest(272) for s in seeds66), dtype=np.uint8).reshape(-1, 272)
    bound = 9 if eta == 4 else 15
    lo, hi = (raw & 15) < bound, (raw >> 4) < bound
    per_byte = lo.astype(np.int32) + hi
    return per_byte[:, :136].sum(axis=1), per_byte.sum(axis=1), hi[:, 135]


def search_es3_keys(stats):
    """ML-DSA-65 xi with a third-block stream: >= 8, a stream of s1 and one of s2, one with 255 and one with <= 253 accepted after
    two blocks; keys with an exactly-256 stream met on the way are kept too (at most two)"""
    k, l, eta = SETS[65]
    keys, exact = [], []
    i = 0
    while True:
        xis = [trial(b"es3-key/65", i + j) for j in range(CHUNK)]
        seeds = [split(65, xi)[1] + r.to_bytes(2, "little") for xi in xis for r in range(k + l)]
        _, acc2, _ = es_counts(eta, seeds)
        acc2 = acc2.reshape(CHUNK, k + l)
        for j in np.nonzero((acc2 <= 256).any(axis=1))[0]:
            third = [dict(stream=int(r), acc2=int(acc2[j, r])) for r in range(k + l) if acc2[j, r] < 256]
            if third:
                keys.append(dict(xi=xis[j].hex(), streams=third))
            elif len(exact) < 2:
                exact.append(dict(xi=xis[j].hex(), streams=[dict(stream=int(r), acc2=256) for r in range(k + l) if acc2[j, r] == 256]))
            a = [st["acc2"] for e in keys for st in e["streams"]]
            s = [st["stream"] for e in keys for st in e["streams"]]
            if len(keys) >= 8 and 255 in a and min(a) <= 253 and min(s) < l <= max(s):
                stats["es3_keys"] = i + int(j) + 1
                return keys, exact
        i += CHUNK
        assert i < 4_000_000, "ES3 key search exceeded its budget"


def search_es_seam(pset, tag, want, stats, name):
    """rho' found directly: trial i is stream i mod (k + l) of rho'_i; want: prop -> count, props over (acc1, acc2, last)"""
    k, l, eta = SETS[pset]
    props = {
        "third_block": lambda a1, a2, last: a2 < 256,
        "exact_256_in_two": lambda a1, a2, last: a2 == 256,
        "b1_256": lambda a1, a2, last: a1 == 256 and not last,
        "b1_255": lambda a1, a2, last: a1 == 255,
        "b1_last_half": lambda a1, a2, last: a1 == 256 and last,
    }
    out, have = [], {p: 0 for p in want}
    i = 0
    while True:
        rps = [trial(tag, i + j, 64) for j in range(CHUNK)]
        seeds = [rp + ((i + j) % (k + l)).to_bytes(2, "little") for j, rp in enumerate(rps)]
        acc1, acc2, last = es_counts(eta, seeds)
        hit = np.zeros(CHUNK, dtype=bool)
        if eta == 4:
            hit |= acc2 <= 256
        else:
            hit |= (acc1 == 255) | (acc1 == 256)
        for j in np.nonzero(hit)[0]:
            for p in want:
                if have[p] < want[p] and props[p](int(acc1[j]), int(acc2[j]), bool(last[j])):
                    have[p] += 1
                    e = dict(rho_prime=rps[j].hex(), stream=(i + int(j)) % (k + l), prop=p)
                    if eta == 4:
                        e["acc2"] = int(acc2[j])
                    out.append(e)
            if have == want:
                stats[name] = i + int(j) + 1
                return out
        i += CHUNK
        assert i < 20_000_000, "ES seam search exceeded its budget"


SHAPES = {
    "rej5": lambda rej: len(rej) >= 5,
    "two_in_group": lambda rej: len({i // 4 for i in rej}) < len(rej),
    "cand55": lambda rej: any(i % 56 == 55 for i in rej),
    "cand27_28": lambda rej: any(i % 56 in (27, 28) for i in rej),
}


def search_ea(pset, stats):
    """xi whose rho has boundary candidates (two xi per (value, index mod 4)) and rejection shapes (two xi per shape)"""
    k, l, _ = SETS[pset]
    cells = {(v, pos): set() for v in ("q", "q-1") for pos in range(4)}
    shapes = {p: set() for p in SHAPES}
    boundary, shape = [], []
    n_xi = max(1, CHUNK // (k * l))
    i = 0
    while True:
        xis = [trial(b"ea/%d" % pset, i + j) for j in range(n_xi)]
        rhos = [split(pset, xi)[0] for xi in xis]
        raw = np.frombuffer(b"".join(hashlib.shake_128(rho + bytes([s, r])).digest(840) for rho in rhos for r in range(k) for s in range(l)),
                            dtype=np.uint8).reshape(-1, 280, 3).astype(np.int32)
        z = raw[:, :, 0] | (raw[:, :, 1] << 8) | ((raw[:, :, 2] & 0x7F) << 16)
        for row in np.nonzero((z >= Q - 1).any(axis=1))[0]:
            zr = z[row]
            ok = zr < Q
            n_cand = int(np.searchsorted(np.cumsum(ok), 256)) + 1       # candidates consumed up to the 256th acceptance
            assert n_cand <= 280
            j, r, s = int(row) // (k * l), int(row) % (k * l) // l, int(row) % l
            rej = [int(c) for c in np.nonzero(~ok[:n_cand])[0]]
            for c in np.nonzero((zr[:n_cand] == Q) | (zr[:n_cand] == Q - 1))[0]:
                cell = ("q" if zr[c] == Q else "q-1", int(c) % 4)
                if len(cells[cell] | {xis[j]}) <= 2:
                    cells[cell].add(xis[j])
                    boundary.append(dict(xi=xis[j].hex(), rho=rhos[j].hex(), r=r, s=s, cand=int(c), value=cell[0], pos=cell[1]))
            for p, f in SHAPES.items():
                if f(rej) and len(shapes[p] | {xis[j]}) <= 2:
                    shapes[p].add(xis[j])
                    shape.append(dict(xi=xis[j].hex(), rho=rhos[j].hex(), r=r, s=s, prop=p, rejections=rej))
            if all(len(v) >= 2 for v in cells.values()) and all(len(v) >= 2 for v in shapes.values()):
                stats["ea_%d" % pset] = i + j + 1
                return boundary, shape
        i += n_xi
        assert i < 3_000_000, "EA search exceeded its budget"


def build():
    stats, wall = {}, {}
    fx = dict(version=1, es_edge={}, ea_boundary={}, ea_shape={})
    t = time.time()
    fx["es3_keys"], fx["es_exact_keys"] = search_es3_keys(stats)
    wall["es3_keys"] = time.time() - t
    t = time.time()
    fx["es3_seam"] = search_es_seam(65, b"es3-seam/65", {"third_block": 8, "exact_256_in_two": 2}, stats, "es3_seam")
    wall["es3_seam"] = time.time() - t
    for pset in (44, 87):
        t = time.time()
        fx["es_edge"][str(pset)] = search_es_seam(pset, b"es-edge/%d" % pset, {"b1_256": 3, "b1_255": 3, "b1_last_half": 3}, stats,
                                                  "es_edge_%d" % pset)
        wall["es_edge_%d" % pset] = time.time() - t
    for pset in (44, 65, 87):
        t = time.time()
        fx["ea_boundary"][str(pset)], fx["ea_shape"][str(pset)] = search_ea(pset, stats)
        wall["ea_%d" % pset] = time.time() - t
    fx["trials"] = stats        # trial seeds each search needed: part of the file, a rerun reproduces them
    return fx, wall


def encode(fx):
    import io
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0, compresslevel=9) as f:
        f.write(json.dumps(fx, sort_keys=True, separators=(",", ":")).encode())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="exit 1 if the search does not reproduce the file")
    a = ap.parse_args()
    fx, wall = build()
    blob = encode(fx)
    for name, n in fx["trials"].items():
        print(f"{name:12s} {n:9d} trial seeds  {wall[name]:6.1f} s", file=sys.stderr)
    if a.check:
        with open(a.out, "rb") as f:
            old = f.read()
        same = json.loads(gzip.decompress(old).decode()) == fx
        print(("identical content, " + ("identical bytes" if old == blob else "another deflate stream")) if same else "DIFFERENT", file=sys.stderr)
        return 0 if same else 1
    with open(a.out, "wb") as f:
        f.write(blob)
    print(f"{a.out}: {len(blob)} bytes", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
