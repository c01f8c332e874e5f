#!/usr/bin/env python3
"""Certificates issued from TBSCertificates on the device (include/mldsa_x509sign.h): what the check, the layout and the frame cost
next to the signing they feed, what the frame kernel reaches next to a plain copy, and what framing on the host costs instead.  One JSON
line per point: each parameter set at --n TBSs, and an even three-way mix of --n TBSs.

The batch is the depth-3 shape of tools/bench_x509.py -- a self-signed root, an intermediate, a leaf -- of v3 TBSCertificates with
21-byte Names and no extensions (a chain is of one parameter set; in the mix the chains take the sets in turn), signed deterministically
by the issuer's key out of --keys keys per set.  TBSs lie 5 mod 16 bytes apart, so source and destination fall on every byte alignment.
Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds samples, median and p10-p90:
  a  mldsa_x509sign_issue_ops: check + offsets + apply + frame                       the code this tool is about
  b  mldsa_recsign_sign on the ops a produced                                        the comparison point, in the same run
  c  a then b, as MlDsaCertificateIssuer.issue_device makes them                     what a caller sees
  f  mldsa_x509sign_frame alone on a's rows                                          2 * tbs_bytes + 22 n bytes read + written
  g  a device-to-device copy that moves the same bytes                               tbs_bytes + 11 n bytes copied
  h  the host route: the certificates framed in Python around a hole (host clock, on --host-certs of them, scaled to --n), the
     framed buffer uploaded (host clock), then b
a / b is what the framing adds to the signing, h / c what the host route costs instead.  Every certificate of c is checked to verify
through mldsa_x509_ops + mldsa_rec_verify.  Nothing is gated on the ratios.

    python tools/bench_x509sign.py > profiles/x509sign_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OID = bytes.fromhex("06096086480165030403")


def tlv(tag, body):
    n = len(body)
    return bytes([tag]) + (bytes([n]) if n < 128 else b"\x81" + bytes([n]) if n < 256 else b"\x82" + n.to_bytes(2, "big")) + body


def alg_id(pset):
    return tlv(0x30, OID + bytes([{44: 0x11, 65: 0x12, 87: 0x13}[pset]]))


def template(pset, pk_len):
    """a TBSCertificate of the set with zero key and Name digits: (bytes, positions of issuer digits, subject digits and key)"""
    alg = alg_id(pset)
    name = tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, b"0" * 8))))
    dates = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))
    head = tlv(0xA0, b"\x02\x01\x02") + tlv(0x02, b"\x12\x34") + alg
    tbs = tlv(0x30, head + name + dates + name + tlv(0x30, alg + tlv(0x03, bytes(1 + pk_len))))
    issuer_at = 4 + len(head) + len(name) - 8
    return tbs, issuer_at, issuer_at + len(dates) + len(name), len(tbs) - pk_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-certs", type=int, default=1024, help="certificates the host framing is timed on")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _x509_lib, _x509sign_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa, MlDsaCertificateIssuer, MlDsaCertificates

    assert torch.cuda.is_available(), "bench_x509sign.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    ca = MlDsaCertificateIssuer(hotpath=hp)
    x5 = MlDsaCertificates(hotpath=hp)
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    pks = {}
    for pset, m in sets.items():
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(args.keys)])
        pks[pset] = pk
        ca.set_keys(pset, m.private_keys_from_bytes(sk))

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def digits(idx):
        """[len(idx), 8] uint8: the indices as eight hex digits, a certificate's common name"""
        idx = np.asarray(idx, dtype=np.uint64)
        return np.stack([np.frombuffer(b"0123456789abcdef", dtype=np.uint8)[((idx >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)]
                         for d in range(8)], axis=1)

    for point in args.points.split(","):
        psets = (44, 65, 87) if point == "mix" else (int(point),)
        n = args.n
        order = np.arange(n)
        set_of = (order // 3) % len(psets)                         # a chain is of one set; the chains take the sets in turn
        issuer = np.where(order % 3 == 0, order, order - 1)
        reqs = np.zeros(n, dtype=_x509sign_lib.REQ_DTYPE)
        reqs["issuer"] = issuer
        blocks, base, tbs_bytes, out_len = [], 3, 0, 0
        for c, pset in enumerate(psets):
            m = sets[pset]
            mine = order[set_of == c]
            tbs, issuer_at, subject_at, key_at = template(pset, m.PK_LEN)
            stride = len(tbs) + (5 - len(tbs)) % 16               # TBSs 5 mod 16 bytes apart: they fall on all sixteen residues
            rows = torch.from_numpy(np.frombuffer(tbs + bytes(stride - len(tbs)), dtype=np.uint8).copy()).cuda().repeat(len(mine), 1)
            rows[:, issuer_at:issuer_at + 8] = torch.from_numpy(digits(issuer[mine])).cuda()
            rows[:, subject_at:subject_at + 8] = torch.from_numpy(digits(mine)).cuda()
            kidx = mine * 2654435761 % args.keys                  # the subject key of every certificate, and through it its issuer's
            rows[:, key_at:key_at + m.PK_LEN] = pks[pset][torch.from_numpy(kidx).cuda()]
            reqs["off"][mine] = base + np.arange(len(mine), dtype=np.uint64) * np.uint64(stride)
            reqs["len"][mine], reqs["set"][mine] = len(tbs), pset
            reqs["key"][mine] = issuer[mine] * 2654435761 % args.keys
            blocks.append(rows.view(-1))
            base += len(mine) * stride
            tbs_bytes += len(mine) * len(tbs)
            out_len += len(mine) * (len(tbs) + 22 + m.SIG_LEN)
            del rows
        blob = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda")] + blocks)
        del blocks
        reqs_d = ca.requests_tensor(reqs)
        out = torch.zeros(out_len, dtype=torch.uint8, device="cuda")
        out_certs = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        ops = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(3, dtype=torch.int64, device="cuda")
        sig_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan = ca.plan_memory(n)
        scratch = ca.signer.sign_scratch(n, tbs_bytes, 0)
        moved = 2 * tbs_bytes + 22 * n
        src = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        lib, nk = ca.lib, ca.signer._n_keys()

        def run_a():
            _x509sign_lib.check(lib.mldsa_x509sign_issue_ops(hp._h, _ptr(blob), blob.numel(), _ptr(reqs_d), n, nk, _ptr(out), out_len, _ptr(out_certs),
                                                             _ptr(ops), _ptr(status), _ptr(totals), _ptr(plan), plan.numel(), _stream(ca.device)))

        def run_b():
            ca.signer.sign_device(blob, ops, out, sig_status, n, 0, scratch=scratch)

        def run_f():
            _x509sign_lib.check(lib.mldsa_x509sign_frame(hp._h, _ptr(blob), blob.numel(), _ptr(reqs_d), n, _ptr(out), out_len, _ptr(out_certs),
                                                         _ptr(status), _stream(ca.device)))

        run = {"a": run_a, "b": run_b, "c": lambda: (run_a(), run_b()), "f": run_f, "g": lambda: dst.copy_(src)}
        run_a()  # (b and f take a's rows from their first sample on)
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
        assert not bool(status.any()) and not bool(sig_status.any()) and totals.tolist() == [n, 0, out_len], "a TBS of the batch was not issued"
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st_v = x5.verify_device(out, out_certs, ok)
        torch.cuda.synchronize()
        assert not bool(st_v.any()) and bool(ok.all()), "an issued certificate did not verify"

        # the host route: Python frames each certificate around a hole of zeros, the framed buffer is uploaded, the device signs
        blob_h = blob.cpu().numpy().tobytes()
        k = min(args.host_certs, n)
        sig_len = {p: sets[p].SIG_LEN for p in psets}
        t0 = time.perf_counter()
        framed = [tlv(0x30, blob_h[int(r["off"]):int(r["off"]) + int(r["len"])] + alg_id(int(r["set"])) + tlv(0x03, bytes(1 + sig_len[int(r["set"])])))
                  for r in reqs[:k]]
        host_ms = (time.perf_counter() - t0) * 1e3
        out_h = out.cpu().numpy()
        at = 0
        for i, der in enumerate(framed):  # what the device framed, the signature aside
            hole = at + int(reqs[i]["len"]) + 22
            assert out_h[at:hole].tobytes() == der[:hole - at] and len(der) == hole - at + sig_len[int(reqs[i]["set"])], i
            at += len(der)
        t0 = time.perf_counter()
        up = torch.from_numpy(out_h).cuda()
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        del up
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, f, g = (st[v]["median_ms"] for v in "abcfg")
        h = host_ms * n / k + upload_ms + b
        print(json.dumps({
            "workload": "x509sign_issue", "label": args.label, "point": point, "n_certs": n, "chain_depth": 3, "keys_per_set": args.keys,
            "blob_bytes": int(blob.numel()), "tbs_bytes": int(tbs_bytes), "out_bytes": int(out_len), "frame_bytes_moved": int(moved),
            "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host route: host clock around the framing of host_certs certificates, scaled, "
                     "and around the upload of the framed buffer, plus b",
            "a_issue_ops": st["a"], "b_recsign_sign_on_the_ops": st["b"], "c_issue_device": st["c"], "f_frame": st["f"], "g_copy": st["g"],
            "host_certs": k, "host_frame_us_per_cert": round(host_ms * 1e3 / k, 2), "host_upload_ms": round(upload_ms, 2),
            "h_host_route_ms": round(h, 1), "a_ns_per_cert": round(a * 1e6 / n, 2), "b_Msigns_s": round(n / b / 1e3, 2),
            "f_TB_s": round(moved / f / 1e9, 3), "g_TB_s": round(moved / g / 1e9, 3), "f_over_g_time": round(f / g, 2),
            "a_over_b_time": round(a / b, 4), "c_over_b_time": round(c_ / b, 3), "h_over_c_time": round(h / c_, 2)}), flush=True)
        del blob, reqs_d, out, out_certs, ops, status, sig_status, plan, scratch, src, dst, run, ok
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
