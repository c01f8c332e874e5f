#!/usr/bin/env python3
"""Verification from wire records on the device (include/mldsa_rec.h): what the layer costs over mldsa_verify_pk on arrays packed
beforehand, what its seam costs against a plain copy of the same bytes, and what the host's repack costs instead.  One JSON line per
point: each parameter set at --n ops, and an even three-way mix of --n ops.

A record is key | signature | 32-byte message back to back; records lie 5 mod 16 bytes apart, so keys, signatures and messages fall on every
byte alignment.  Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds samples,
median and p10-p90:
  a  mldsa_verify_pk per parameter set on dense arrays packed beforehand     the floor: nothing left to sort or realign
  b  mldsa_rec_verify on the blob and its descriptors                         the layer: plan, one wait, pack, a's calls, scatter
  c  mldsa_rec_plan + mldsa_rec_pack alone (totals known to the host)         the seam
  d  a device-to-device copy of the bytes the pack moves                      the HBM rate of the same run
  e  the host route: numpy repack of the blob + upload + a                    host clock, --host-rounds samples; the records of a set
                                                                              are equally long here, so the repack is three strided
                                                                              numpy copies per set: the cheapest form a host has
b / a is the overhead of the layer, c / d the seam against the copy, e / b what the host repack costs.  Verdicts of a, b and e are
compared.  Nothing is gated on the ratios.

    python tools/bench_rec.py > profiles/rec_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="distinct keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-rounds", type=int, default=3, help="samples of the host route")
    ap.add_argument("--inner", type=int, default=2, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _rec_lib
    from fips204_amd.hotpath import HotPath
    from fips204_amd.ml_dsa import MlDsa, MlDsaRecords

    assert torch.cuda.is_available(), "bench_rec.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    recs = MlDsaRecords(hotpath=hp)
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    MSG = 32

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def dense(pset, n):
        """n signed ops of one set on the device: (pk [n, PK_LEN], sigs, msgs [n, 32], msg_off)"""
        m = sets[pset]
        d = min(args.keys, n)
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(d)])
        kidx = torch.from_numpy((np.arange(n) * 2654435761 % d).astype(np.uint32).view(np.int32)).cuda()
        msgs = torch.randint(0, 256, (n, MSG), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(pset))
        mo = torch.arange(0, (n + 1) * MSG, MSG, dtype=torch.int64, device="cuda")
        sigs = torch.empty((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
        m.sign_device(m.private_keys_from_bytes(sk), msgs.view(-1), mo, torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), sigs, n, key_idx=kidx)
        return pk[kidx.long()].contiguous(), sigs, msgs, mo

    for point in args.points.split(","):
        psets = (44, 65, 87) if point == "mix" else (int(point),)
        n = args.n
        counts = [n // len(psets) + (1 if c < n % len(psets) else 0) for c in range(len(psets))]
        arrays, blocks, ops, base = {}, [], np.zeros(n, dtype=_rec_lib.OP_DTYPE), 3
        for c, (pset, n_c) in enumerate(zip(psets, counts)):
            pk, sigs, msgs, mo = arrays[pset] = dense(pset, n_c)
            m = sets[pset]
            rec_len = m.PK_LEN + m.SIG_LEN + MSG
            pad = (5 - rec_len) % 16  # records 5 mod 16 bytes apart: consecutive records fall on all sixteen residues
            rows = torch.cat([pk, sigs, msgs, torch.zeros((n_c, pad), dtype=torch.uint8, device="cuda")], dim=1)
            start = np.uint64(base) + np.arange(n_c, dtype=np.uint64) * np.uint64(rec_len + pad)
            mine = ops[c::len(psets)]
            mine["pk_off"], mine["sig_off"], mine["msg_off"] = start, start + np.uint64(m.PK_LEN), start + np.uint64(m.PK_LEN + m.SIG_LEN)
            mine["ctx_off"], mine["msg_len"], mine["set"] = start, MSG, pset
            blocks.append(rows.view(-1))
            base += n_c * (rec_len + pad)
        blob = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda")] + blocks)
        del blocks
        ops_d = recs.ops_tensor(ops)
        moved = sum(n_c * (sets[p].PK_LEN + sets[p].SIG_LEN + MSG) for p, n_c in zip(psets, counts))
        ok_a = {p: torch.zeros(n_c, dtype=torch.uint8, device="cuda") for p, n_c in zip(psets, counts)}
        ok_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
        scratch = recs.verify_scratch(n, n * MSG, 0)
        tot = _rec_lib.RecTotals()
        for p, n_c in zip(psets, counts):
            tot.n[_rec_lib.CLASS_SETS.index(p)], tot.msg_bytes[_rec_lib.CLASS_SETS.index(p)] = n_c, n_c * MSG
        arena = torch.empty(recs.rec.mldsa_rec_scratch_bytes(tot.n[0], tot.n[1], tot.n[2], n * MSG, 0) + 256, dtype=torch.uint8, device="cuda")
        src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")

        def run_a():
            for p in psets:
                pk, sigs, msgs, mo = arrays[p]
                sets[p].verify_pk_device(pk, msgs.view(-1), mo, sigs, ok_a[p], pk.shape[0])

        def run_c():
            class_slot, totals, plan = recs.plan_device(blob, ops_d, n)
            recs.pack_device(blob, ops_d, class_slot, tot, plan, n, arena=arena)

        run = {"a": run_a, "b": lambda: recs.verify_device(blob, ops_d, ok_b, n, scratch=scratch), "c": run_c, "d": lambda: dst.copy_(src)}
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
        for c, p in enumerate(psets):
            assert bool(ok_a[p].all()) and torch.equal(ok_b[c::len(psets)], ok_a[p]), p

        # the host route: the blob lies in host memory; numpy gathers each set's dense arrays, uploads them, then a
        blob_h, host_ms = blob.cpu().numpy(), []
        for r in range(args.host_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c, p in enumerate(psets):
                m, mine = sets[p], ops[c::len(psets)]
                first, stride = int(mine["pk_off"][0]), int(mine["pk_off"][1] - mine["pk_off"][0]) if len(mine) > 1 else len(blob_h)
                block = blob_h[first:first + len(mine) * stride].reshape(len(mine), -1)  # (equal strides: the repack is three strided copies)
                cut = lambda lo, ln: torch.from_numpy(np.ascontiguousarray(block[:, lo:lo + ln])).cuda()  # noqa: E731
                pk, sigs, msgs = cut(0, m.PK_LEN), cut(m.PK_LEN, m.SIG_LEN), cut(m.PK_LEN + m.SIG_LEN, MSG)
                m.verify_pk_device(pk, msgs.view(-1), arrays[p][3], sigs, ok_a[p], pk.shape[0])
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(bool(ok_a[p].all()) for p in psets)
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, d = (st[v]["median_ms"] for v in "abcd")
        e = float(np.median(host_ms))
        print(json.dumps({
            "workload": "rec_verify", "label": args.label, "point": point, "n_ops": n, "ops_per_set": dict(zip(map(str, psets), counts)),
            "message_bytes": MSG, "bytes_packed": moved, "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host route: host clock around repack + upload + calls + synchronise",
            "a_verify_pk_prepacked": st["a"], "b_rec_verify": st["b"], "c_plan_pack": st["c"], "d_d2d_copy_same_bytes": st["d"],
            "e_host_repack_upload_verify_ms": round(e, 2), "host_rounds": args.host_rounds,
            "a_Mverifies_s": round(n / a / 1e3, 1), "b_Mverifies_s": round(n / b / 1e3, 1),
            "b_over_a_time": round(b / a, 3), "c_over_d_time": round(c_ / d, 2), "c_over_a_time": round(c_ / a, 3), "e_over_b_time": round(e / b, 1),
            "seam_GBs_read_plus_written": round(2 * moved / 1e9 / (c_ * 1e-3), 1), "copy_GBs_read_plus_written": round(2 * moved / 1e9 / (d * 1e-3), 1)}),
            flush=True)
        del arrays, blob, ops_d, scratch, arena, src, dst, ok_a, ok_b, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
