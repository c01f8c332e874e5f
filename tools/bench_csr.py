#!/usr/bin/env python3
"""Certification requests on the device (include/mldsa_csr.h): what the walk and the TBSCertificate assembly cost next to the two crypto
calls they feed, what the write kernel reaches next to a plain copy, and what walking and assembling on the host costs instead.  One
JSON line per point: each parameter set at --n requests, and an even three-way mix of --n requests.

The batch: PKCS#10 requests with a 21-byte subject Name, the key of one of --keys keys per set and empty attributes, each signed on the
device by its own key (mldsa_recsign_sign writes the signature into the request's BIT STRING); the CA key is of the request's set, the
template one issuer Name and one Validity shared by all entries, an 8-byte serial per entry, no extensions, deterministic signing.
Requests lie 5 mod 16 bytes apart, so the copied pieces fall on every byte alignment.
Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds samples, median and p10-p90:
  a  mldsa_csr_parse                                                                  the walk
  b  mldsa_rec_verify on the ops a produced                                           its comparison point, in the same run
  c  mldsa_csr_tbs: check + offsets + apply + write                                   the assembly
  d  mldsa_x509sign_issue_ops + mldsa_recsign_sign on what c produced                 its comparison point, in the same run
  e  the five calls, as MlDsaCertificateRequests.issue_device makes them              what a caller sees
  w  mldsa_csr_tbs_write alone on c's rows                                            2 * tbs_bytes read + written
  g  a device-to-device copy that moves the same bytes                                tbs_bytes copied
  h  the host route: a Python DER walk and TBSCertificate assembly (host clock, on --host-reqs requests, scaled to --n), the assembled
     buffer uploaded (host clock), then b and d
a / b and c / d are what the two stages add to the crypto calls behind them, h / e what the host route costs instead.  Every request is
checked to be possessed, every certificate to be signed and to parse through mldsa_x509_ops, and the TBSCertificates of the host route to
be the device's bytes.  Nothing is gated on the ratios.

    python tools/bench_csr.py > profiles/csr_bench.jsonl
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


def name(cn):
    return tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, cn))))


DATES = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))


def template(pset, pk_len, sig_len):
    """a request of the set with zero key, signature and Name digits: (bytes, positions of the CertificationRequestInfo and its length,
    the subject digits, the key and the signature)"""
    alg = alg_id(pset)
    cri = tlv(0x30, tlv(0x02, b"\x00") + name(b"0" * 8) + tlv(0x30, alg + tlv(0x03, bytes(1 + pk_len))) + tlv(0xA0, b""))
    der = tlv(0x30, cri + alg + tlv(0x03, bytes(1 + sig_len)))
    return der, 4, len(cri), 4 + 4 + 3 + len(name(b"0" * 8)) - 8, 4 + len(cri) - 2 - pk_len, len(der) - sig_len


def host_walk(der):
    """a plain Python walk of one request: (subject TLV, SPKI TLV), after the checks of the device walk's path"""
    def take(pos):
        tag, first = der[pos], der[pos + 1]
        if first < 0x80:
            return tag, pos + 2, pos + 2 + first
        k = first & 0x7F
        return tag, pos + 2 + k, pos + 2 + k + int.from_bytes(der[pos + 2:pos + 2 + k], "big")
    _, at, end = take(0)
    _, cri_at, cri_end = take(at)
    _, alg_at, alg_end = take(cri_end)
    _, sig_at, sig_end = take(alg_end)
    _, ver_at, ver_end = take(cri_at)
    _, _, sub_end = take(ver_end)
    _, spki_at, spki_end = take(sub_end)
    _, kalg_at, kalg_end = take(spki_at)
    tag, _, attrs_end = take(spki_end)
    assert end == len(der) == sig_end and der[ver_at:ver_end] == b"\x00" and der[kalg_at:kalg_end] == der[alg_at:alg_end] and tag == 0xA0 and \
        attrs_end == cri_end
    return der[ver_end:sub_end], der[sub_end:spki_end]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-reqs", type=int, default=1024, help="requests the host walk and assembly are timed on")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _csr_lib, _recsign_lib, _x509_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa, MlDsaCertificateRequests, MlDsaCertificates

    assert torch.cuda.is_available(), "bench_csr.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    ca = MlDsaCertificateRequests(hotpath=hp)
    x5 = MlDsaCertificates(hotpath=hp)
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    pks = {}
    for pset, m in sets.items():
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(args.keys)])
        pks[pset] = pk
        ca.set_keys(pset, m.private_keys_from_bytes(sk))  # requesters and CAs draw from one table per set

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def digits(idx):
        """[len(idx), 8] uint8: the indices as eight hex digits, a request's common name"""
        idx = np.asarray(idx, dtype=np.uint64)
        return np.stack([np.frombuffer(b"0123456789abcdef", dtype=np.uint8)[((idx >> np.uint64(4 * (7 - d))) & np.uint64(15)).astype(np.int64)]
                         for d in range(8)], axis=1)

    issuer_name = name(b"bench CA")
    for point in args.points.split(","):
        psets = (44, 65, 87) if point == "mix" else (int(point),)
        n = args.n
        order = np.arange(n)
        set_of = order % len(psets)
        items = np.zeros(n, dtype=_csr_lib.ITEM_DTYPE)
        entries = np.zeros(n, dtype=_csr_lib.ISSUE_DTYPE)
        sign_ops = np.zeros(n, dtype=_recsign_lib.OP_DTYPE)
        blocks, base = [], 3
        for c, pset in enumerate(psets):
            m = sets[pset]
            mine = order[set_of == c]
            der, cri_at, cri_len, cn_at, key_at, sig_at = template(pset, m.PK_LEN, m.SIG_LEN)
            stride = len(der) + (5 - len(der)) % 16               # requests 5 mod 16 bytes apart: they fall on all sixteen residues
            rows = torch.from_numpy(np.frombuffer(der + bytes(stride - len(der)), dtype=np.uint8).copy()).cuda().repeat(len(mine), 1)
            rows[:, cn_at:cn_at + 8] = torch.from_numpy(digits(mine)).cuda()
            kidx = mine * 2654435761 % args.keys                  # the requester's key
            rows[:, key_at:key_at + m.PK_LEN] = pks[pset][torch.from_numpy(kidx).cuda()]
            off = base + np.arange(len(mine), dtype=np.uint64) * np.uint64(stride)
            items["off"][mine], items["len"][mine] = off, len(der)
            sign_ops["msg_off"][mine], sign_ops["msg_len"][mine] = off + np.uint64(cri_at), cri_len
            sign_ops["sig_off"][mine], sign_ops["key"][mine], sign_ops["set"][mine] = off + np.uint64(sig_at), kidx, pset
            entries["set"][mine], entries["key"][mine] = pset, (mine + 1) * 2654435761 % args.keys
            blocks.append(rows.view(-1))
            base += len(mine) * stride
            del rows
        # the template pieces behind the requests: one issuer Name, one Validity, eight serial bytes per entry
        serials = np.zeros((n, 8), dtype=np.uint8)
        serials[:, 0] = 0x01
        serials[:, 1:] = digits(order)[:, 1:]
        tail = issuer_name + DATES
        blob = torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda")] + blocks +
                         [torch.from_numpy(np.frombuffer(tail, dtype=np.uint8).copy()).cuda(), torch.from_numpy(serials.reshape(-1)).cuda()])
        del blocks
        entries["issuer_off"], entries["issuer_len"] = base, len(issuer_name)
        entries["validity_off"], entries["validity_len"] = base + len(issuer_name), len(DATES)
        entries["serial_off"], entries["serial_len"] = base + len(tail) + 8 * order.astype(np.uint64), 8
        # every request signed by its own key, in place
        sst = torch.zeros(n, dtype=torch.int32, device="cuda")
        ca.issuer.signer.sign_device(blob, ca.issuer.signer.ops_tensor(sign_ops), blob, sst, n, 0,
                                     scratch=ca.issuer.signer.sign_scratch(n, int(sign_ops["msg_len"].sum()), 0))
        torch.cuda.synchronize()
        assert not bool(sst.any()), "a request of the batch was not signed"

        items_d, entries_d = ca.items_tensor(items), ca.issue_tensor(entries)
        fields = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
        ops = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
        st1 = torch.empty(n, dtype=torch.uint8, device="cuda")
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        vscratch = ca.records.verify_scratch(n, int(blob.numel()), 0)
        plan = ca.plan_memory(n)
        lib, s = ca.lib, _stream(ca.device)

        def run_a():
            _csr_lib.check(lib.mldsa_csr_parse(hp._h, _ptr(blob), blob.numel(), _ptr(items_d), n, _ptr(fields), _ptr(ops), _ptr(st1), s))

        def run_b():
            ca.records.verify_device(blob, ops, ok, n, 0, scratch=vscratch)

        run_a()
        run_b()
        torch.cuda.synchronize()
        assert not bool(st1.any()) and bool(ok.all()), "a request of the batch was refused"
        rows_1 = fields.cpu().numpy().view(_csr_lib.FIELDS_DTYPE)
        tbs_bytes = (24 + 8 + len(tail)) * n + int(rows_1["subject_len"].astype(np.int64).sum() + rows_1["spki_len"].astype(np.int64).sum())
        out_len = tbs_bytes + sum(int((set_of == c).sum()) * (22 + sets[p].SIG_LEN) for c, p in enumerate(psets))
        tbs = torch.zeros(tbs_bytes, dtype=torch.uint8, device="cuda")
        out = torch.zeros(out_len, dtype=torch.uint8, device="cuda")
        reqs = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        st2 = torch.empty(n, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(3, dtype=torch.int64, device="cuda")
        sig_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        iplan = ca.issuer.plan_memory(n)
        sscratch = ca.issuer.signer.sign_scratch(n, tbs_bytes, 0)
        src = torch.zeros(tbs_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        issued = {}

        def run_c():
            _csr_lib.check(lib.mldsa_csr_tbs(hp._h, _ptr(blob), blob.numel(), _ptr(fields), _ptr(entries_d), _ptr(ok), n, _ptr(tbs), tbs_bytes,
                                             _ptr(reqs), _ptr(st2), _ptr(totals), _ptr(plan), plan.numel(), s))

        def run_d():
            issued["rows"], issued["status"], _ = ca.issuer.issue_device(tbs, reqs, out, sig_status, n, plan=iplan, scratch=sscratch)

        def run_w():
            _csr_lib.check(lib.mldsa_csr_tbs_write(hp._h, _ptr(blob), blob.numel(), _ptr(fields), _ptr(entries_d), n, _ptr(tbs), tbs_bytes, _ptr(reqs),
                                                   _ptr(st2), s))

        run = {"a": run_a, "b": run_b, "c": run_c, "d": run_d, "e": lambda: (run_a(), run_b(), run_c(), run_d()), "w": run_w,
               "g": lambda: dst.copy_(src)}
        run_c()  # (d and w take c's rows from their first sample on)
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
        assert not bool(st2.any()) and not bool(issued["status"].any()) and not bool(sig_status.any()) and totals.tolist() == [n, 0, tbs_bytes], \
            "a request of the batch was not issued"
        # every certificate parses on the verifying side (the CA keys differ per entry, so no chain is linked here)
        rows_h = issued["rows"].cpu().numpy().view(_x509_lib.CERT_DTYPE).copy()
        rows_h["issuer"] = _x509_lib.NO_ISSUER
        _, st_v, _ = x5.ops_device(out, x5.certs_tensor(rows_h), n)
        torch.cuda.synchronize()
        assert bool((st_v == _x509_lib.PARSE_ONLY).all()), "an issued certificate does not parse"

        # the host route: Python walks each request and assembles its TBSCertificate, the buffer is uploaded, the device verifies and signs
        blob_h = blob.cpu().numpy().tobytes()
        k = min(args.host_reqs, n)
        t0 = time.perf_counter()
        built = []
        for it, e in zip(items[:k], entries[:k]):
            der = blob_h[int(it["off"]):int(it["off"]) + int(it["len"])]
            subject, spki = host_walk(der)
            serial = blob_h[int(e["serial_off"]):int(e["serial_off"]) + 8]
            built.append(tlv(0x30, tlv(0xA0, b"\x02\x01\x02") + tlv(0x02, serial) + alg_id(int(e["set"])) + issuer_name + DATES + subject + spki))
        host_ms = (time.perf_counter() - t0) * 1e3
        tbs_h = tbs.cpu().numpy()
        at = 0
        for i, t in enumerate(built):  # what the device assembled
            assert tbs_h[at:at + len(t)].tobytes() == t, i
            at += len(t)
        t0 = time.perf_counter()
        up = torch.from_numpy(tbs_h).cuda()
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        del up
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, d, e_, w, g = (st[v]["median_ms"] for v in "abcdewg")
        h = host_ms * n / k + upload_ms + b + d
        print(json.dumps({
            "workload": "csr_issue", "label": args.label, "point": point, "n_requests": n, "keys_per_set": args.keys,
            "blob_bytes": int(blob.numel()), "tbs_bytes": int(tbs_bytes), "out_bytes": int(out_len), "write_bytes_moved": int(2 * tbs_bytes),
            "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host route: host clock around the walk and assembly of host_reqs requests, "
                     "scaled, and around the upload of the assembled buffer, plus b and d",
            "a_parse": st["a"], "b_rec_verify_on_the_ops": st["b"], "c_tbs": st["c"], "d_issue_ops_and_recsign_sign": st["d"], "e_five_calls": st["e"],
            "w_tbs_write": st["w"], "g_copy": st["g"], "host_reqs": k, "host_walk_and_assembly_us_per_request": round(host_ms * 1e3 / k, 2),
            "host_upload_ms": round(upload_ms, 2), "h_host_route_ms": round(h, 1), "a_ns_per_request": round(a * 1e6 / n, 2),
            "c_ns_per_request": round(c_ * 1e6 / n, 2), "w_TB_s": round(2 * tbs_bytes / w / 1e9, 3), "g_TB_s": round(2 * tbs_bytes / g / 1e9, 3),
            "w_over_g_time": round(w / g, 2), "a_over_b_time": round(a / b, 4), "c_over_d_time": round(c_ / d, 4),
            "e_over_b_plus_d_time": round(e_ / (b + d), 3), "h_over_e_time": round(h / e_, 2)}), flush=True)
        del blob, items_d, entries_d, fields, ops, st1, ok, vscratch, plan, tbs, out, reqs, st2, sig_status, iplan, sscratch, src, dst, run, issued
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
