#!/usr/bin/env python3
"""Wire public keys deduplicated on the device in front of batched verification (include/mldsa_keys.h): one JSON line per
(parameter set, distinct keys D) point, --n operations per call, every op carrying its own wire-format key.

Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds samples, median and
p10-p90:
  a  mldsa_verify_pk, one wire key per op                          the baseline: the entry point a caller has without this library
  b  mldsa_verify_pk_dedup with max_cached_keys = D                the cached route at every D, so that the sweep finds where it stops paying
  b_default  ... with the Python default for max_cached_keys       what a caller gets who says nothing (plain route above the default)
  c  mldsa_verify_cached_a on a pre-built table, key_idx and A_hat the bound: nothing left to find or expand
  d  mldsa_keys_dedup alone                                        GB/s of key bytes (n PK_LEN over its time) against the HBM rate
b / a, b / c, and `b_beats_a`: b's median below a's by more than a's own p10-p90 spread.  Verdicts of a, b and c are compared.

    python tools/bench_keys.py > profiles/keys_dedup_bench.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6290.0  # specification; the rate a float4 copy kernel reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--sets", default="44,65,87")
    ap.add_argument("--distinct", default="1,64,1024,8192,65536")
    ap.add_argument("--rounds", type=int, default=15, help="samples per variant and point")
    ap.add_argument("--inner", type=int, default=4, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd.ml_dsa import MlDsa, _cat_with_offsets

    assert torch.cuda.is_available(), "bench_keys.py measures on the GPU; there is no other path"
    n = args.n

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    for pset in [int(x) for x in args.sets.split(",")]:
        m = MlDsa(pset)
        msgs = [b"%032d" % i for i in range(n)]
        mb, mo = _cat_with_offsets(msgs, m.device)
        rnd = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        for d in [int(x) for x in args.distinct.split(",")]:
            d = min(d, n)
            pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(d)])
            sks, pks = m.private_keys_from_bytes(sk), m.public_keys_from_bytes(pk)
            kidx_host = (np.arange(n) * 2654435761 % d).astype(np.uint32)  # repeats spread over the batch, not in runs
            kidx = torch.from_numpy(kidx_host.view(np.int32)).cuda()
            sigs = torch.empty((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
            m.sign_device(sks, mb, mo, rnd, sigs, n, key_idx=kidx)
            del sks, sk
            pk_ops = pk[kidx.long()].contiguous()  # one wire key per op: what a service holds
            a_hat = m.expand_a_for_keys(pks)
            ok = {v: torch.zeros(n, dtype=torch.uint8, device="cuda") for v in "abBc"}
            info, info_default = {}, {}
            # caller-owned scratch, as in the C API: allocated once per point, outside the timed calls
            scr, scr_default = m.dedup_verify_scratch(n, d), m.dedup_verify_scratch(n)
            run = {
                "a": lambda: m.verify_pk_device(pk_ops, mb, mo, sigs, ok["a"], n),
                "b": lambda: m.verify_pk_dedup_device(pk_ops, mb, mo, sigs, ok["b"], n, max_cached_keys=d, info=info, scratch=scr),
                "b_default": lambda: m.verify_pk_dedup_device(pk_ops, mb, mo, sigs, ok["B"], n, info=info_default, scratch=scr_default),
                "c": lambda: m.verify_device(pks, mb, mo, sigs, ok["c"], n, key_idx=kidx, a_hat=a_hat),
                "d": lambda: m.dedup_public_keys_device(pk_ops, table_rows=d),
            }
            times = {v: [] for v in run}
            for r in range(args.warmup + args.rounds):
                for v, fn in run.items():  # alternating: every round takes one sample of every variant
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.inner):
                        fn()
                    e1.record()
                    e1.synchronize()
                    if r >= args.warmup:
                        times[v].append(e0.elapsed_time(e1) / args.inner)
            torch.cuda.synchronize()
            assert bool(ok["a"].all()) and torch.equal(ok["a"], ok["b"]) and torch.equal(ok["a"], ok["B"]) and torch.equal(ok["a"], ok["c"])
            assert info["n_rows"] == d and info["route"] == "cached", info
            st = {v: stats(t) for v, t in times.items()}
            a, b, c, dd = (st[v]["median_ms"] for v in ("a", "b", "c", "d"))
            key_gb = n * m.PK_LEN / 1e9
            rec = {"workload": "keys_dedup", "label": args.label, "set": pset, "n_ops": n, "distinct_keys": d,
                   "rounds": args.rounds, "calls_per_sample": args.inner, "clock": "hipEvent pair around the calls of a sample",
                   "a_verify_pk": st["a"], "b_verify_pk_dedup": st["b"], "b_default_max_cached": st["b_default"],
                   "default_max_cached_keys": m.DEDUP_MAX_CACHED_KEYS, "b_default_route": info_default["route"],
                   "c_verify_cached_a": st["c"], "d_keys_dedup": st["d"],
                   "a_Mverifies_s": round(n / a / 1e3, 1), "b_Mverifies_s": round(n / b / 1e3, 1),
                   "b_default_Mverifies_s": round(n / st["b_default"]["median_ms"] / 1e3, 1), "c_Mverifies_s": round(n / c / 1e3, 1),
                   "b_over_a_time": round(b / a, 3), "b_over_c_time": round(b / c, 3),
                   "b_default_over_a_time": round(st["b_default"]["median_ms"] / a, 3),
                   "b_beats_a": bool(a - b > st["a"]["p90_ms"] - st["a"]["p10_ms"]),
                   "seam_key_GBs": round(key_gb / (dd * 1e-3), 1), "seam_fraction_of_hbm_peak": round(key_gb / (dd * 1e-3) / HBM_PEAK_GBS, 3),
                   "seam_fraction_of_hbm_copy_rate": round(key_gb / (dd * 1e-3) / HBM_COPY_GBS, 3)}
            print(json.dumps(rec), flush=True)
            del pk_ops, a_hat, pks, sigs, ok, scr, scr_default, run
            torch.cuda.empty_cache()
        m.hp.close()


if __name__ == "__main__":
    main()
