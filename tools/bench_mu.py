#!/usr/bin/env python3
"""External-mu ML-DSA on the device (include/mldsa_mu.h): one JSON line per (parameter set, n_ops) point.

Per point, alternating in one process on the same device arrays after warm-up, a hipEvent pair on the calls' stream around every
call, --steps samples per variant, median and p10-p90:
  mu64, mu1k     mldsa_mu_compute on 64-byte and on 1 KiB messages (MODE_PURE, empty ctx)
  verify_mu      mldsa_verify_mu on mu                against  verify   mldsa_verify(MLDSA_MODE_INTERNAL) on the 64-byte messages
  sign_mu        mldsa_sign_mu on mu and rnd          against  sign     mldsa_sign(MLDSA_MODE_INTERNAL) on the same messages
The core library is the one every other figure of the repository was taken on, so its two calls in the same run are the reference the
layered calls are set against.  Verdicts and signatures of the two routes are compared.  Scratch is allocated once per point,
outside the timed calls, as a C caller would.

    python tools/bench_mu.py            # writes profiles/external_mu_bench.jsonl and prints the lines
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="65:65536,65:1,44:65536,87:65536", help="set:n_ops, comma separated")
    ap.add_argument("--keys", type=int, default=1024, help="distinct keys of a point (at most n_ops)")
    ap.add_argument("--steps", type=int, default=20, help="timed samples per variant and point (at least 20)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds per point")
    ap.add_argument("--only", default="", help="comma separated variants to run (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "external_mu_bench.jsonl"))
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20")

    import numpy as np
    import torch

    from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PURE, MlDsa, _cat_with_offsets

    assert torch.cuda.is_available(), "bench_mu.py measures on the GPU; there is no other path"

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    lines = []
    models = {}
    for point in args.points.split(","):
        pset, n = (int(x) for x in point.split(":"))
        m = models.setdefault(pset, MlDsa(pset))
        d = max(1, min(args.keys, n))
        rng = np.random.default_rng(1000 * pset + n % 997)
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(d)])
        sks, pks = m.private_keys_from_bytes(sk), m.public_keys_from_bytes(pk)
        kidx = torch.from_numpy((np.arange(n) * 2654435761 % d).astype(np.uint32).view(np.int32)).cuda()
        m64 = torch.from_numpy(rng.integers(0, 256, n * 64, dtype=np.uint8)).cuda()
        o64 = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device="cuda")
        m1k = torch.from_numpy(rng.integers(0, 256, n * 1024, dtype=np.uint8)).cuda()
        o1k = torch.arange(0, 1024 * (n + 1), 1024, dtype=torch.int64, device="cuda")
        rnd = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        mu, flag = m.mu_device(sks.tr, m64, o64, n, key_idx=kidx, mode=MODE_INTERNAL)
        sig = {v: torch.zeros((n, m.SIG_LEN), dtype=torch.uint8, device="cuda") for v in ("sign", "sign_mu")}
        ok = {v: torch.zeros(n, dtype=torch.uint8, device="cuda") for v in ("verify", "verify_mu")}
        scr_v, scr_s = m.mu_scratch(n), m.mu_scratch(n, sign=True)
        m.sign_device(sks, m64, o64, rnd, sig["sign"], n, key_idx=kidx, mode=MODE_INTERNAL)
        good = sig["sign"].clone()
        run = {
            "mu64": lambda: m.mu_device(sks.tr, m64, o64, n, key_idx=kidx, mode=MODE_PURE),
            "mu1k": lambda: m.mu_device(sks.tr, m1k, o1k, n, key_idx=kidx, mode=MODE_PURE),
            "verify": lambda: m.verify_device(pks, m64, o64, good, ok["verify"], n, key_idx=kidx, mode=MODE_INTERNAL),
            "verify_mu": lambda: m.verify_mu_device(pks, mu, good, ok["verify_mu"], n, kidx, flag, scr_v),
            "sign": lambda: m.sign_device(sks, m64, o64, rnd, sig["sign"], n, key_idx=kidx, mode=MODE_INTERNAL),
            "sign_mu": lambda: m.sign_mu_device(sks, mu, rnd, sig["sign_mu"], n, kidx, flag, None, scr_s),
        }
        if args.only:
            run = {v: f for v, f in run.items() if v in args.only.split(",")}
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
        if "verify" in run and "verify_mu" in run:
            assert bool(ok["verify"].all()) and torch.equal(ok["verify"], ok["verify_mu"])
        if "sign_mu" in run:
            assert torch.equal(sig["sign_mu"], good), "mldsa_sign_mu and mldsa_sign disagree"
        st = {v: stats(t) for v, t in times.items()}
        rec = {"workload": "external_mu", "label": args.label, "set": pset, "n_ops": n, "distinct_keys": d, "steps": args.steps,
               "warmup": args.warmup, "clock": "hipEvent pair on the stream around each call", "device": torch.cuda.get_device_name(0)}
        rec.update({v: s for v, s in st.items()})
        for v in st:
            rec[v + "_Mops_s"] = round(n / st[v]["median_ms"] / 1e3, 4)
        if "mu64" in st:
            rec["mu64_GBs"] = round(n * 64 / st["mu64"]["median_ms"] / 1e6, 2)
        if "mu1k" in st:
            rec["mu1k_GBs"] = round(n * 1024 / st["mu1k"]["median_ms"] / 1e6, 2)
        if "verify" in st and "verify_mu" in st:
            rec["verify_mu_over_verify_time"] = round(st["verify_mu"]["median_ms"] / st["verify"]["median_ms"], 3)
        if "sign" in st and "sign_mu" in st:
            rec["sign_mu_over_sign_time"] = round(st["sign_mu"]["median_ms"] / st["sign"]["median_ms"], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del run, scr_v, scr_s, sig, ok, good, mu, flag, m64, m1k, sks, pks
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for m in models.values():
        m.hp.close()


if __name__ == "__main__":
    main()
