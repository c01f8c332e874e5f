#!/usr/bin/env python3
"""Search polynomials whose forward NTT grows large in the lazy representatives: writes tests/golden/ntt_growth_inputs.json.

ntt_fwd_wave (csrc/ntt_wave.h) and the reference's ntt add and subtract without reducing, level after level; the header promises
|w_hat| < 9 q for inputs below q in magnitude.  Uniform inputs stay near 3.4 q.  This script hill-climbs inputs with coefficients in
[-H, H], H = (q - 1) / 2 -- the largest magnitude that survives the kernels' reduce32 on load -- to maximise max |orc.ntt(w)|: the
oracle is built with -fwrapv and reproduces the reference's representatives exactly.  CPU only, fixed seed and a fixed number of
steps (about a minute), so a rerun writes the same file.  The magnitudes it reaches are recorded beside the polynomials;
tests/test_arith_cases_cpu.py asserts that they reproduce and that each lies beyond what the random NTT inputs of the suite reach."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402

Q, N = orc.Q, 256
H = (Q - 1) // 2
N_POLYS, STEPS, BATCH, SEED = 8, 2600, 384, 20241


def score(w):
    return np.abs(orc.ntt(w.astype(np.int32)).astype(np.int64)).reshape(-1, N).max(axis=1)


def climb(rng):
    w = rng.choice([-H, H], N).astype(np.int64)
    best = int(score(w[None])[0])
    rows = np.arange(BATCH)
    for _ in range(STEPS):
        cand = np.repeat(w[None], BATCH, axis=0)
        for _ in range(3):  # up to three coefficients per candidate: at the ends of the range, or anywhere inside it
            pos = rng.integers(0, N, BATCH)
            val = np.where(rng.integers(0, 2, BATCH) == 1, rng.choice([-H, H], BATCH), rng.integers(-H, H + 1, BATCH))
            keep = rng.integers(0, 3, BATCH) == 0
            cand[rows, pos] = np.where(keep, cand[rows, pos], val)
        s = score(cand)
        i = int(s.argmax())
        if s[i] > best:
            best, w = int(s[i]), cand[i].copy()
    return w, best


def main():
    rng = np.random.default_rng(SEED)
    polys, mags = [], []
    for p in range(N_POLYS):
        w, m = climb(rng)
        assert np.abs(w).max() <= H and int(score(w[None])[0]) == m
        polys.append([int(x) for x in w])
        mags.append(m)
        print(f"poly {p}: max |ntt| = {m} = {m / Q:.3f} q", flush=True)
    out = os.path.join(ROOT, "tests", "golden", "ntt_growth_inputs.json")
    with open(out, "w") as f:
        json.dump({"q": Q, "bound": "|w| <= (q - 1) / 2", "seed": SEED, "max_abs_ntt": mags, "polys": polys}, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: {os.path.getsize(out)} bytes, largest {max(mags) / Q:.3f} q")


if __name__ == "__main__":
    main()
