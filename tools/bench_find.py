#!/usr/bin/env python3
"""Path building on the device (include/mldsa_find.h): what finding every certificate's issuer costs next to the calls it stands in
front of, and what the same work costs on the host.  One JSON line per point: each parameter set at --n certificates, and an even
three-way mix.

The batch is that of tools/bench_path.py -- chains of depth 3, a self-signed root, an intermediate, a leaf, validly signed on the
device, 5 mod 16 bytes apart, three extensions in every certificate, a subjectKeyIdentifier among them -- with the certificate ARRAY
shuffled by a seeded permutation and every issuer index withheld.  Per point, alternating in one process after warm-up, hipEvent times
of --inner calls per sample, --rounds samples, median and p10-p90:
  a  mldsa_find_build: k_find_ids, the table, k_find_issuers                          the call
  b  mldsa_x509_ops on the same certificates, with the issuers found                  its comparison point: two Names per certificate
  c  mldsa_rec_verify on the ops of b                                                  the work that follows
  d  mldsa_find_table alone: the clears, k_find_claim, k_find_confirm                 the table build
  e  a device-to-device copy of the bytes d reads                                      its comparison point: the traffic floor
  g  mldsa_find_ids alone;  h  mldsa_find_issuers alone                                the per-kernel split of a
  r  mldsa_x509_parse, mldsa_path_parse, mldsa_find_build, mldsa_x509_link             the whole route to linked ops, as a caller sees it
  f  a plain Python walk of every certificate, a dict keyed by (set, subject Name), the lookups, and the upload of the indices
                                                                                       host clock, on --host-certs of them, scaled to --n
Every issuer found is checked against the permutation, and every status of b is checked to be OK.  Nothing is gated on the ratios.

    python tools/bench_find.py > profiles/find_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_path import template  # noqa: E402
from bench_x509 import host_walk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-certs", type=int, default=1023, help="certificates the host route is timed on (whole chains)")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--seed", type=int, default=204, help="of the permutation")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _find_lib, _path_lib, _x509_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MODE_PURE, MlDsa, MlDsaPathBuilder, MlDsaPathValidator

    assert torch.cuda.is_available(), "bench_find.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    pv = MlDsaPathValidator(hotpath=hp)
    pb = MlDsaPathBuilder(hotpath=hp, seed=bytes(range(16)))
    x5 = pv.certificates
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    keys = {}
    for pset, m in sets.items():
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(args.keys)])
        keys[pset] = (pk, m.private_keys_from_bytes(sk))

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def digits(idx):
        idx = np.asarray(idx, dtype=np.uint64)
        return np.stack([np.frombuffer(b"0123456789abcdef", dtype=np.uint8)[((idx >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)]
                         for d in range(8)], axis=1)

    for point in args.points.split(","):
        psets = (44, 65, 87) if point == "mix" else (int(point),)
        n = args.n // 3 * 3
        order = np.arange(n)
        set_of = (order // 3) % len(psets)
        issuer = np.where(order % 3 == 0, order, order - 1)
        certs = np.zeros(n, dtype=_x509_lib.CERT_DTYPE)
        blocks, base, tbs_bytes, name_len = [], 3, 0, 0
        for c, pset in enumerate(psets):
            m = sets[pset]
            mine = order[set_of == c]
            der, issuer_at, subject_at, key_at, sig_at, tbs_at, tbs_len = template(pset, m.PK_LEN, m.SIG_LEN)
            stride = len(der) + (5 - len(der)) % 16
            rows = torch.from_numpy(np.frombuffer(der + bytes(stride - len(der)), dtype=np.uint8).copy()).cuda().repeat(len(mine), 1)
            rows[:, issuer_at:issuer_at + 8] = torch.from_numpy(digits(issuer[mine])).cuda()
            rows[:, subject_at:subject_at + 8] = torch.from_numpy(digits(mine)).cuda()
            kidx = mine * 2654435761 % args.keys
            rows[:, key_at:key_at + m.PK_LEN] = keys[pset][0][torch.from_numpy(kidx).cuda()]
            msgs = rows[:, tbs_at:tbs_at + tbs_len].contiguous()
            mo = torch.arange(0, (len(mine) + 1) * tbs_len, tbs_len, dtype=torch.int64, device="cuda")
            rnd = torch.zeros((len(mine), 32), dtype=torch.uint8, device="cuda")
            sigs = torch.zeros((len(mine), m.SIG_LEN), dtype=torch.uint8, device="cuda")
            signer = torch.from_numpy((issuer[mine] * 2654435761 % args.keys).astype(np.uint32).view(np.int32)).cuda()
            st = torch.zeros(len(mine), dtype=torch.int32, device="cuda")
            m.sign_device(keys[pset][1], msgs.view(-1), mo, rnd, sigs, len(mine), key_idx=signer, status=st)
            torch.cuda.synchronize()
            assert not bool(st.any())
            rows[:, sig_at:sig_at + m.SIG_LEN] = sigs
            certs["off"][mine] = base + np.arange(len(mine), dtype=np.uint64) * np.uint64(stride)
            certs["len"][mine] = len(der)
            blocks.append(rows.view(-1))
            base += len(mine) * stride
            tbs_bytes += len(mine) * tbs_len
            del rows, msgs, sigs
        blob = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda")] + blocks)
        del blocks
        # the shuffle: position q of the array holds certificate perm[q]; the blob stays as it is, nobody is told an issuer
        perm = np.random.default_rng(args.seed).permutation(n)
        where = np.argsort(perm)
        want = where[issuer[perm]].astype(np.uint32)
        shuffled = certs[perm].copy()
        shuffled["issuer"] = _x509_lib.NO_ISSUER
        certs_d = x5.certs_tensor(shuffled)
        new = lambda size: torch.empty(size, dtype=torch.uint8, device="cuda")  # noqa: E731
        fields, policy, ids, totals, certs_out, results = new(n * 56), new(n * 48), new(n * 24), new(16), new(n * 16), new(n * 12)
        ops, status, ok = new(n * 40), new(n), torch.zeros(n, dtype=torch.uint8, device="cuda")
        scratch = pb.scratch_memory(n)
        rec_scratch = x5.records.verify_scratch(n, tbs_bytes, 0)
        h, s, seed = hp._h, _stream(pv.device), pb.seed
        _x509_lib.check(x5.lib.mldsa_x509_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, _ptr(fields), s))
        _path_lib.check(pv.lib.mldsa_path_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, 0, _ptr(policy), s))
        torch.cuda.synchronize()
        name_len = int(fields.cpu().numpy().view(_x509_lib.FIELDS_DTYPE)[0]["subject_len"])
        table_read = n * (16 + 56 + 24 + 3 * name_len + 20)  # three rows; the subject Name for two hashes and one comparison; the identifier
        copy_src, copy_dst = new(table_read), new(table_read)

        def run_a():
            _find_lib.check(pb.lib.mldsa_find_build(h, _ptr(blob), blob.numel(), _ptr(certs_d), _ptr(fields), _ptr(policy), n, seed, 64, _ptr(ids),
                                                    _ptr(totals), _ptr(certs_out), _ptr(results), _ptr(scratch), scratch.numel(), s))

        def run_b():
            _x509_lib.check(x5.lib.mldsa_x509_ops(h, _ptr(blob), blob.numel(), _ptr(certs_out), n, _x509_lib.CHECK_NAMES, _ptr(fields), _ptr(ops),
                                                  _ptr(status), s))

        def run_c():
            x5.records.verify_device(blob, ops, ok, n, MODE_PURE, scratch=rec_scratch)

        def run_d():
            _find_lib.check(pb.lib.mldsa_find_table(h, _ptr(blob), blob.numel(), _ptr(certs_d), _ptr(fields), _ptr(ids), n, seed, 64, _ptr(totals),
                                                    _ptr(scratch), scratch.numel(), s))

        def run_g():
            _find_lib.check(pb.lib.mldsa_find_ids(h, _ptr(blob), blob.numel(), _ptr(certs_d), _ptr(policy), n, _ptr(ids), s))

        def run_h():
            _find_lib.check(pb.lib.mldsa_find_issuers(h, _ptr(blob), blob.numel(), _ptr(certs_d), _ptr(fields), _ptr(ids), n, seed, 64, _ptr(totals),
                                                      _ptr(scratch), scratch.numel(), _ptr(certs_out), _ptr(results), s))

        def run_r():
            _x509_lib.check(x5.lib.mldsa_x509_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, _ptr(fields), s))
            _path_lib.check(pv.lib.mldsa_path_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, 0, _ptr(policy), s))
            run_a()
            _x509_lib.check(x5.lib.mldsa_x509_link(h, _ptr(blob), blob.numel(), _ptr(certs_out), _ptr(fields), n, _x509_lib.CHECK_NAMES, _ptr(ops),
                                                   _ptr(status), s))

        run = {"a": run_a, "b": run_b, "c": run_c, "d": run_d, "e": lambda: copy_dst.copy_(copy_src), "g": run_g, "h": run_h, "r": run_r}
        run_a()  # (b takes certs_out, c the ops of b, d and h the ids from here on)
        run_b()
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
        res = results.cpu().numpy().view(_find_lib.RESULT_DTYPE)
        tot = totals.cpu().numpy().view(_find_lib.TOTALS_DTYPE)[0]
        assert not res["status"].any() and np.array_equal(res["issuer"], want) and (res["candidates"] == 1).all(), "an issuer was not found"
        assert not status.cpu().numpy().any() and bool(ok.all()), "a certificate does not verify under the issuer found"
        assert int(tot["overflow"]) == 0 and int(tot["candidates"]) == n

        # the host: the blob lies in host memory; Python walks each certificate, enters it into a dict, looks its issuer up, uploads
        blob_h = blob.cpu().numpy().tobytes()
        k = min(args.host_certs, n) // 3 * 3
        first = perm[:k]  # the host sees the same shuffled array; its chains are whole where the first k positions hold them
        t0 = time.perf_counter()
        walked = [host_walk(blob_h, int(shuffled[q]["off"]), int(shuffled[q]["len"])) for q in range(k)]
        table = {}
        for q, w in enumerate(walked):
            table.setdefault(w[5], q)
        found = np.array([table.get(w[4], 0xFFFFFFFF) for w in walked], dtype=np.uint32)
        torch.from_numpy(found.view(np.int32)).cuda()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        inside = np.isin(perm[want[:k]], first)  # the issuer lies among the first k positions
        assert np.array_equal(found[inside], want[:k][inside])
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, d, e, g, hh, rr = (st[v]["median_ms"] for v in "abcdeghr")
        f = host_ms * n / k
        print(json.dumps({
            "workload": "find", "label": args.label, "point": point, "n_certs": n, "chain_depth": 3, "extensions": 3, "shuffled": True,
            "keys_per_set": args.keys, "blob_bytes": int(blob.numel()), "name_bytes": name_len, "table_slots": int(pb.lib.mldsa_find_table_slots(n)),
            "scratch_bytes": int(scratch.numel()), "table_read_bytes": table_read, "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host: host clock around walk, dict, lookups and upload of host_certs certificates, scaled",
            "a_find_build": st["a"], "b_x509_ops": st["b"], "c_rec_verify": st["c"], "d_find_table": st["d"], "e_copy_of_the_bytes_read": st["e"],
            "g_find_ids": st["g"], "h_find_issuers": st["h"], "r_whole_route": st["r"],
            "f_host_ms_scaled": round(f, 1), "host_certs": k, "host_us_per_cert": round(host_ms * 1e3 / k, 2),
            "a_ns_per_cert": round(a * 1e6 / n, 2), "a_over_b_time": round(a / b, 3), "a_over_c_time": round(a / c_, 4),
            "d_over_e_time": round(d / e, 3), "g_d_h_over_a_time": round((g + d + hh) / a, 3), "f_over_r_time": round(f / rr, 1)}), flush=True)
        del blob, certs_d, fields, policy, ids, totals, certs_out, results, ops, status, ok, scratch, rec_scratch, copy_src, copy_dst, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
