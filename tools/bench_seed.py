#!/usr/bin/env python3
"""Private keys in seed form on the device (include/mldsa_seed.h): one JSON line per measured point, every call of the layer set
against the route the core alone offers for the same seeds.

Per point, alternating in one process on the same device arrays after warm-up, a hipEvent pair on the calls' stream around every
variant, --steps samples per variant, median and p10-p90:
  expand   expand_pk / expand_nopk   mldsa_seed_expand with and without the wire public key
           keygen_sk_expand          mldsa_keygen + mldsa_sk_expand (wire keys written, read back and expanded)
  check    seed_check                mldsa_seed_check
           keygen_compare            mldsa_keygen + a torch byte compare of the private keys, one verdict per key
  sign     sign_seed                 mldsa_sign_seed: n_ops messages over --keys seeds (MODE_INTERNAL, 64-byte messages)
           keygen_sk_expand_sign     mldsa_keygen + mldsa_sk_expand + mldsa_sign on the same seeds and messages
The results of the two routes are compared.  Scratch and outputs are allocated once per point, outside the timed calls, as a C
caller would.

    python tools/bench_seed.py            # writes profiles/seed_keys_bench.jsonl and prints the lines
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q = 8380417


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expand", default="65:65536,65:1,44:65536,87:65536", help="set:n_keys points of the expansion, comma separated")
    ap.add_argument("--check", default="65:65536", help="set:n_keys points of the consistency check")
    ap.add_argument("--sign", default="65:65536", help="set:n_ops points of signing from seeds")
    ap.add_argument("--keys", type=int, default=1024, help="seeds of a signing point (at most n_ops)")
    ap.add_argument("--steps", type=int, default=20, help="timed samples per variant and point (at least 20)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds per point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_keys_bench.jsonl"))
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20")

    import numpy as np
    import torch

    from fips204_amd.ml_dsa import MODE_INTERNAL, MlDsa

    assert torch.cuda.is_available(), "bench_seed.py measures on the GPU; there is no other path"

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def measure(run):
        times = {v: [] for v in run}
        for r in range(args.warmup + args.steps):
            for v, fn in run.items():  # alternating: every round takes one sample of every variant
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[v].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        return {v: stats(t) for v, t in times.items()}

    def points(spec):
        return [tuple(int(x) for x in p.split(":")) for p in spec.split(",") if p]

    def record(kind, pset, n, st, **extra):
        rec = {"workload": "seed_keys", "kind": kind, "label": args.label, "set": pset, "n": n, "steps": args.steps, "warmup": args.warmup,
               "clock": "hipEvent pair on the stream around each variant", "device": torch.cuda.get_device_name(0)}
        rec.update(extra)
        rec.update(st)
        for v in st:
            rec[v + "_per_s"] = round(n / st[v]["median_ms"] * 1e3, 1)
        return rec

    lines = []
    models = {}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def seeds(pset, n):
        rng = np.random.default_rng(1000 * pset + n % 997)
        return torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()

    for pset, n in points(args.expand):
        m = models.setdefault(pset, MlDsa(pset))
        xi = seeds(pset, n)
        out_pk, out_nopk, out_par = m.empty_private_keys(n), m.empty_private_keys(n), m.empty_private_keys(n)
        pk_w = torch.empty((n, m.PK_LEN), dtype=torch.uint8, device="cuda")
        sk_w = torch.empty((n, m.SK_LEN), dtype=torch.uint8, device="cuda")
        scratch = m.seed_scratch(n)
        got_pk = {}

        def expand_pk():
            got_pk["pk"] = m.expand_seeds_device(xi, out=out_pk, want_pk=True, scratch=scratch)[1]

        def parent():
            m.keygen_from_seed(xi, out=(pk_w, sk_w))
            m.private_keys_from_bytes(sk_w, out=out_par)

        st = measure({"expand_pk": expand_pk, "expand_nopk": lambda: m.expand_seeds_device(xi, out=out_nopk, scratch=scratch),
                      "keygen_sk_expand": parent})
        assert torch.equal(got_pk["pk"], pk_w), "mldsa_seed_expand and mldsa_keygen disagree on pk"
        for f in ("rho", "cap_k", "tr"):
            assert torch.equal(getattr(out_pk, f), getattr(out_par, f)) and torch.equal(getattr(out_nopk, f), getattr(out_par, f)), f
        for f in ("s_1_hat_mont", "s_2_hat_mont", "t_0_hat_mont"):
            assert not bool(((getattr(out_pk, f).long() - getattr(out_par, f).long()) % Q).any()), f
        emit(record("expand", pset, n, st, scratch_bytes=scratch.numel(),
                    expand_pk_over_parent_time=round(st["expand_pk"]["median_ms"] / st["keygen_sk_expand"]["median_ms"], 3),
                    expand_nopk_over_parent_time=round(st["expand_nopk"]["median_ms"] / st["keygen_sk_expand"]["median_ms"], 3)))
        del out_pk, out_nopk, out_par, pk_w, sk_w, scratch, got_pk
        torch.cuda.empty_cache()

    for pset, n in points(args.check):
        m = models.setdefault(pset, MlDsa(pset))
        xi = seeds(pset, n)
        _, sk = m.keygen_from_seed(xi)
        sk[1::2, 77] ^= 1  # every other key damaged
        pk_w = torch.empty((n, m.PK_LEN), dtype=torch.uint8, device="cuda")
        sk_w = torch.empty((n, m.SK_LEN), dtype=torch.uint8, device="cuda")
        scratch = m.seed_scratch(n, "check")
        res = {}

        def seed_check():
            res["a"] = m.check_seeds_device(xi, sk, scratch=scratch)

        def keygen_compare():
            m.keygen_from_seed(xi, out=(pk_w, sk_w))
            res["b"] = (sk_w == sk).all(dim=1)

        st = measure({"seed_check": seed_check, "keygen_compare": keygen_compare})
        assert torch.equal(res["a"], res["b"]) and int(res["a"].sum()) == (n + 1) // 2
        emit(record("check", pset, n, st, scratch_bytes=scratch.numel(),
                    seed_check_over_parent_time=round(st["seed_check"]["median_ms"] / st["keygen_compare"]["median_ms"], 3)))
        del sk, pk_w, sk_w, scratch, res
        torch.cuda.empty_cache()

    for pset, n in points(args.sign):
        m = models.setdefault(pset, MlDsa(pset))
        d = max(1, min(args.keys, n))
        xi = seeds(pset, d)
        rng = np.random.default_rng(7 + pset)
        kidx = torch.from_numpy((np.arange(n) * 2654435761 % d).astype(np.uint32).view(np.int32)).cuda()
        m64 = torch.from_numpy(rng.integers(0, 256, n * 64, dtype=np.uint8)).cuda()
        o64 = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device="cuda")
        rnd = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        sig = {v: torch.zeros((n, m.SIG_LEN), dtype=torch.uint8, device="cuda") for v in ("sign_seed", "keygen_sk_expand_sign")}
        pk_w = torch.empty((d, m.PK_LEN), dtype=torch.uint8, device="cuda")
        sk_w = torch.empty((d, m.SK_LEN), dtype=torch.uint8, device="cuda")
        out_par = m.empty_private_keys(d)
        scratch = m.seed_scratch(d, "sign")

        def parent_sign():
            m.keygen_from_seed(xi, out=(pk_w, sk_w))
            m.private_keys_from_bytes(sk_w, out=out_par)
            m.sign_device(out_par, m64, o64, rnd, sig["keygen_sk_expand_sign"], n, key_idx=kidx, mode=MODE_INTERNAL)

        st = measure({"sign_seed": lambda: m.sign_from_seeds_device(xi, m64, o64, rnd, sig["sign_seed"], n, key_idx=kidx, mode=MODE_INTERNAL,
                                                                   scratch=scratch),
                      "keygen_sk_expand_sign": parent_sign})
        assert torch.equal(sig["sign_seed"], sig["keygen_sk_expand_sign"]), "mldsa_sign_seed and mldsa_sign disagree"
        emit(record("sign", pset, n, st, seeds=d, scratch_bytes=scratch.numel(),
                    sign_seed_over_parent_time=round(st["sign_seed"]["median_ms"] / st["keygen_sk_expand_sign"]["median_ms"], 3)))
        del sig, pk_w, sk_w, out_par, scratch, m64, rnd
        torch.cuda.empty_cache()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for m in models.values():
        m.hp.close()


if __name__ == "__main__":
    main()
