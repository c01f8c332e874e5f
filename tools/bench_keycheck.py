#!/usr/bin/env python3
"""Strict import of wire private keys on the device (include/mldsa_keycheck.h): one JSON line per measured point, every call of the
layer set against what the core alone offers.

Per point, alternating in one process on the same device arrays after warm-up, a hipEvent pair on the calls' stream around every
variant, --steps samples per variant, median and p10-p90:
  range    range_check               mldsa_sk_range_check
           hbm_copy                  a device-to-device copy of 1 GiB: the HBM rate of this run; stream_ms is the time to read the s1 | s2
                                     regions ((L + K) 32 b bytes per key) at that rate
  pair     pair_check / _nopk        mldsa_keypair_check with and without pk
           keygen                    mldsa_keygen at the same n: the same class of work (ExpandA, A s1 + s2, Power2Round, tr)
           parent_route              mldsa_sk_expand + mldsa_get_public_key + mldsa_pk_into_bytes + mldsa_pk_expand + a torch compare of pk
                                     and tr, one verdict per key: the nearest the core offers; it checks tr and pk, neither t0 nor ranges
  import   import_range / _pair      mldsa_sk_import at both levels
           sk_expand                 mldsa_sk_expand
Half of the keys of a pair point carry a flipped t0 bit, so the verdicts are compared too.  Scratch and outputs are allocated once per
point, outside the timed calls, as a C caller would.

    python tools/bench_keycheck.py            # writes profiles/keycheck_bench.jsonl and prints the lines
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
    ap.add_argument("--points", default="65:65536,65:1,44:65536,87:65536", help="set:n_keys points, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed samples per variant and point (at least 20)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds per point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keycheck_bench.jsonl"))
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20")

    import numpy as np
    import torch

    from fips204_amd import _keycheck_lib
    from fips204_amd.hotpath import _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa

    assert torch.cuda.is_available(), "bench_keycheck.py measures on the GPU; there is no other path"

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

    def record(kind, pset, n, st, **extra):
        rec = {"workload": "keycheck", "kind": kind, "label": args.label, "set": pset, "n": n, "steps": args.steps, "warmup": args.warmup,
               "clock": "hipEvent pair on the stream around each variant", "device": torch.cuda.get_device_name(0)}
        rec.update(extra)
        rec.update(st)
        return rec

    lines = []
    models = {}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def ratio(st, a, b):
        return round(st[a]["median_ms"] / st[b]["median_ms"], 3)

    hbm_src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    hbm_dst = torch.empty_like(hbm_src)

    for spec in (p for p in args.points.split(",") if p):
        pset, n = (int(x) for x in spec.split(":"))
        m = models.setdefault(pset, MlDsa(pset))
        p = m.params
        rng = np.random.default_rng(1000 * pset + n % 997)
        xi = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        pk, sk = m.keygen_from_seed(xi)
        sk[1::2, -1] ^= 0x80  # every other key: one bit of its t0 field
        want = torch.zeros(n, dtype=torch.uint8, device="cuda")
        want[1::2] = _keycheck_lib.KEY_T0
        lib, h, null = _keycheck_lib.load(), m.hp._h, None
        stream = _stream(m.device)

        # ---- range
        flag_r = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = measure({"range_check": lambda: _keycheck_lib.check(lib.mldsa_sk_range_check(h, pset, _ptr(sk), _ptr(flag_r), n, stream)),
                      "hbm_copy": lambda: hbm_dst.copy_(hbm_src)})
        assert not bool(flag_r.any())
        gbs = 2 * hbm_src.numel() / st["hbm_copy"]["median_ms"] / 1e6
        region = (p.l + p.k) * 32 * (3 if p.eta == 2 else 4)
        stream_ms = n * region / gbs / 1e6
        emit(record("range", pset, n, st, region_bytes_per_key=region, hbm_gb_per_s=round(gbs, 1), stream_ms=round(stream_ms, 5),
                    range_check_over_stream_time=round(st["range_check"]["median_ms"] / stream_ms, 2)))

        # ---- pair
        scratch = m.keycheck_scratch(n)
        flag_p, flag_n = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        pk_w = torch.empty((n, m.PK_LEN), dtype=torch.uint8, device="cuda")
        sk_w = torch.empty((n, m.SK_LEN), dtype=torch.uint8, device="cuda")
        keys, pks_a = m.empty_private_keys(n), m.empty_public_keys(n)
        res = {}

        def pair(with_pk, flag):
            _keycheck_lib.check(lib.mldsa_keypair_check(h, pset, _ptr(sk), _ptr(pk) if with_pk else null, _ptr(flag), n, _ptr(scratch),
                                                        scratch.numel(), stream))

        def parent_route():
            m.private_keys_from_bytes(sk, out=keys)
            pub = m.get_public_key(keys)
            wire = m.public_keys_into_bytes(pub)
            m.public_keys_from_bytes(wire, out=pks_a)
            res["parent"] = (wire != pk).any(dim=1) | (pks_a.tr != keys.tr).any(dim=1)

        st = measure({"pair_check": lambda: pair(True, flag_p), "pair_check_nopk": lambda: pair(False, flag_n),
                      "keygen": lambda: m.keygen_from_seed(xi, out=(pk_w, sk_w)), "parent_route": parent_route})
        assert torch.equal(flag_p, want) and torch.equal(flag_n, want), "mldsa_keypair_check: wrong verdicts"
        assert not bool(res["parent"].any())  # the parent's route cannot see a t0 fault
        emit(record("pair", pset, n, st, scratch_bytes=scratch.numel(), pair_check_over_keygen_time=ratio(st, "pair_check", "keygen"),
                    pair_check_over_parent_route_time=ratio(st, "pair_check", "parent_route")))

        # ---- import
        out_r, out_p, out_x = m.empty_private_keys(n), m.empty_private_keys(n), m.empty_private_keys(n)

        def imp(level, o, flag, with_scratch):
            _keycheck_lib.check(lib.mldsa_sk_import(
                h, pset, level, _ptr(sk), _ptr(pk) if with_scratch else null, _ptr(o.rho), _ptr(o.cap_k), _ptr(o.tr), _ptr(o.s_1_hat_mont),
                _ptr(o.s_2_hat_mont), _ptr(o.t_0_hat_mont), _ptr(flag), n, _ptr(scratch) if with_scratch else null,
                scratch.numel() if with_scratch else 0, stream))

        st = measure({"import_range": lambda: imp(_keycheck_lib.LEVEL_RANGE, out_r, flag_r, False),
                      "import_pair": lambda: imp(_keycheck_lib.LEVEL_PAIR, out_p, flag_p, True),
                      "sk_expand": lambda: m.private_keys_from_bytes(sk, out=out_x)})
        assert torch.equal(flag_p, want) and not bool(flag_r.any())
        assert torch.equal(out_r.s_1_hat_mont, out_x.s_1_hat_mont) and torch.equal(out_p.t_0_hat_mont[0::2], out_x.t_0_hat_mont[0::2])
        assert not bool(out_p.t_0_hat_mont[1::2].any())
        emit(record("import", pset, n, st, import_range_over_sk_expand_time=ratio(st, "import_range", "sk_expand"),
                    import_pair_over_sk_expand_time=ratio(st, "import_pair", "sk_expand")))
        del scratch, flag_p, flag_n, flag_r, pk_w, sk_w, keys, pks_a, out_r, out_p, out_x, res, pk, sk
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for m in models.values():
        m.hp.close()


if __name__ == "__main__":
    main()
