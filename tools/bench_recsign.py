#!/usr/bin/env python3
"""Signing of request records on the device (include/mldsa_recsign.h): what the layer costs over mldsa_sign on arrays packed beforehand,
what its seam costs against a plain copy of the same bytes, and what the host's split and scatter cost instead.  One JSON line per
point: each parameter set at --n ops, and an even three-way mix of --n ops.

A record is 32-byte message | 32 bytes of rnd | signature hole back to back, signed in place (out == blob); records lie 5 mod 16 bytes
apart, so messages, rnd and holes fall on every byte alignment.  Per point, alternating in one process after warm-up, hipEvent times
of --inner calls per sample, --rounds samples, median and p10-p90:
  a  mldsa_sign per parameter set on dense arrays packed beforehand, sigs dense    the floor: nothing left to sort, realign or scatter
  b  mldsa_recsign_sign on the blob and its descriptors                            the layer: plan, one wait, pack, a's calls, scatter,
                                                                                   the clearing of rnd
  c  mldsa_recsign_plan + _pack + _scatter alone (totals known to the host)        the seam
  d  a device-to-device copy of the bytes the seam moves                           the HBM rate of the same run
  e  the host route: numpy split of the blob + upload + a + download + scatter     host clock, --host-rounds samples; the records of a set
                                                                                   are equally long here, so split and scatter are
                                                                                   strided numpy copies: the cheapest form a host has
b / a is the overhead of the layer, c / d the seam against the copy, e / b what the host route costs.  Signatures of a, b and e are
compared.  Nothing is gated on the ratios.

    python tools/bench_recsign.py > profiles/recsign_bench.jsonl
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
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-rounds", type=int, default=3, help="samples of the host route")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _recsign_lib
    from fips204_amd.hotpath import HotPath
    from fips204_amd.ml_dsa import MlDsa, MlDsaRecordSigner

    assert torch.cuda.is_available(), "bench_recsign.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    signer = MlDsaRecordSigner(hotpath=hp)
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    MSG, RND = 32, 32
    tables = {}
    for pset, m in sets.items():
        _, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(args.keys)])
        tables[pset] = m.private_keys_from_bytes(sk)
        signer.set_keys(pset, tables[pset])

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def dense(pset, n):
        """n requests of one set on the device: (msgs [n, 32], msg_off, rnd [n, 32], key_idx, room for sigs and status)"""
        gen = torch.Generator(device="cuda").manual_seed(pset)
        msgs = torch.randint(0, 256, (n, MSG), dtype=torch.uint8, device="cuda", generator=gen)
        rnd = torch.randint(0, 256, (n, RND), dtype=torch.uint8, device="cuda", generator=gen)
        mo = torch.arange(0, (n + 1) * MSG, MSG, dtype=torch.int64, device="cuda")
        kidx_h = (np.arange(n) * 2654435761 % args.keys).astype(np.uint32)
        kidx = torch.from_numpy(kidx_h.view(np.int32)).cuda()
        sigs = torch.zeros((n, sets[pset].SIG_LEN), dtype=torch.uint8, device="cuda")
        return dict(msgs=msgs, mo=mo, rnd=rnd, kidx=kidx, kidx_h=kidx_h, sigs=sigs, status=torch.zeros(n, dtype=torch.int32, device="cuda"))

    for point in args.points.split(","):
        psets = (44, 65, 87) if point == "mix" else (int(point),)
        n = args.n
        counts = [n // len(psets) + (1 if c < n % len(psets) else 0) for c in range(len(psets))]
        arrays, blocks, ops, base, layout = {}, [], np.zeros(n, dtype=_recsign_lib.OP_DTYPE), 3, {}
        for c, (pset, n_c) in enumerate(zip(psets, counts)):
            a = arrays[pset] = dense(pset, n_c)
            sig_len = sets[pset].SIG_LEN
            rec_len = MSG + RND + sig_len
            pad = (5 - rec_len) % 16  # records 5 mod 16 bytes apart: consecutive records fall on all sixteen residues
            rows = torch.cat([a["msgs"], a["rnd"], torch.zeros((n_c, sig_len + pad), dtype=torch.uint8, device="cuda")], dim=1)
            start = np.uint64(base) + np.arange(n_c, dtype=np.uint64) * np.uint64(rec_len + pad)
            mine = ops[c::len(psets)]
            mine["msg_off"], mine["rnd_off"], mine["sig_off"] = start, start + np.uint64(MSG), start + np.uint64(MSG + RND)
            mine["ctx_off"], mine["msg_len"], mine["set"], mine["flags"], mine["key"] = start, MSG, pset, _recsign_lib.FLAG_RND, a["kidx_h"]
            layout[pset] = (base, rec_len + pad)
            blocks.append(rows.view(-1))
            base += n_c * (rec_len + pad)
        blob = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda")] + blocks)
        del blocks
        ops_d = signer.ops_tensor(ops)
        moved = sum(n_c * (MSG + RND + sets[p].SIG_LEN) for p, n_c in zip(psets, counts))
        status_b = torch.zeros(n, dtype=torch.int32, device="cuda")
        scratch = signer.sign_scratch(n, n * MSG, 0)
        tot = _recsign_lib.RecsignTotals()
        for p, n_c in zip(psets, counts):
            tot.n[_recsign_lib.CLASS_SETS.index(p)], tot.msg_bytes[_recsign_lib.CLASS_SETS.index(p)] = n_c, n_c * MSG
        arena = torch.empty(signer.lib.mldsa_recsign_arena_bytes(tot.n[0], tot.n[1], tot.n[2], n * MSG, 0) + 256, dtype=torch.uint8, device="cuda")
        seam_out = torch.empty(blob.numel(), dtype=torch.uint8, device="cuda")
        src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")

        def run_a():
            for p in psets:
                a = arrays[p]
                sets[p].sign_device(tables[p], a["msgs"].view(-1), a["mo"], a["rnd"], a["sigs"], a["sigs"].shape[0], key_idx=a["kidx"],
                                    status=a["status"])

        def run_c():
            class_slot, totals, plan = signer.plan_device(ops_d, blob.numel(), blob.numel(), n)
            packed = signer.pack_device(blob, ops_d, blob.numel(), class_slot, tot, plan, n, arena=arena)
            signer.scatter_device(ops_d, blob.numel(), seam_out, class_slot, packed, status_b, n)

        run = {"a": run_a, "b": lambda: signer.sign_device(blob, ops_d, blob, status_b, n, scratch=scratch), "c": run_c,
               "d": lambda: dst.copy_(src)}
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
        run["b"]()  # (variant c's scatter wrote status_b last)
        torch.cuda.synchronize()
        assert not bool(status_b.any())
        for c, p in enumerate(psets):  # the holes hold a's signatures
            first, stride = layout[p]
            n_c, sig_len = counts[c], sets[p].SIG_LEN
            holes = blob[first:first + n_c * stride].view(n_c, stride)[:, MSG + RND:MSG + RND + sig_len]
            assert not bool(arrays[p]["status"].any()) and torch.equal(holes, arrays[p]["sigs"]), p

        # the host route: the blob lies in host memory; numpy gathers each set's dense arrays, uploads them, a signs, the signatures
        # come back and numpy writes them into their holes
        blob_h, host_ms = blob.cpu().numpy().copy(), []
        want_h = blob_h.copy()
        for r in range(args.host_rounds):
            for p in psets:
                first, stride = layout[p]
                blob_h[first:first + arrays[p]["sigs"].shape[0] * stride].reshape(-1, stride)[:, MSG + RND:MSG + RND + sets[p].SIG_LEN] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c, p in enumerate(psets):
                m, n_c = sets[p], counts[c]
                first, stride = layout[p]
                block = blob_h[first:first + n_c * stride].reshape(n_c, stride)  # (equal strides: split and scatter are strided copies)
                up = lambda lo, ln: torch.from_numpy(np.ascontiguousarray(block[:, lo:lo + ln])).cuda()  # noqa: E731
                msgs, rnd = up(0, MSG), up(MSG, RND)
                kidx = torch.from_numpy(np.ascontiguousarray(ops[c::len(psets)]["key"]).view(np.int32)).cuda()
                sigs = torch.empty((n_c, m.SIG_LEN), dtype=torch.uint8, device="cuda")
                m.sign_device(tables[p], msgs.view(-1), arrays[p]["mo"], rnd, sigs, n_c, key_idx=kidx, status=arrays[p]["status"])
                block[:, MSG + RND:MSG + RND + m.SIG_LEN] = sigs.cpu().numpy()
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(blob_h, want_h)
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, d = (st[v]["median_ms"] for v in "abcd")
        e = float(np.median(host_ms))
        print(json.dumps({
            "workload": "recsign_sign", "label": args.label, "point": point, "n_ops": n, "ops_per_set": dict(zip(map(str, psets), counts)),
            "message_bytes": MSG, "keys_per_set": args.keys, "bytes_moved": moved, "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host route: host clock around split + upload + calls + download + scatter",
            "a_sign_prepacked": st["a"], "b_recsign_sign": st["b"], "c_plan_pack_scatter": st["c"], "d_d2d_copy_same_bytes": st["d"],
            "e_host_split_upload_sign_download_scatter_ms": round(e, 2), "host_rounds": args.host_rounds,
            "a_Msigns_s": round(n / a / 1e3, 2), "b_Msigns_s": round(n / b / 1e3, 2),
            "b_over_a_time": round(b / a, 3), "c_over_d_time": round(c_ / d, 2), "c_over_a_time": round(c_ / a, 3), "e_over_b_time": round(e / b, 2),
            "seam_GBs_read_plus_written": round(2 * moved / 1e9 / (c_ * 1e-3), 1), "copy_GBs_read_plus_written": round(2 * moved / 1e9 / (d * 1e-3), 1)}),
            flush=True)
        del arrays, blob, ops_d, scratch, arena, src, dst, seam_out, status_b, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
