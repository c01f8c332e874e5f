#!/usr/bin/env python3
"""Certificate signatures from DER on the device (include/mldsa_x509.h): what the DER walk and the link cost next to the verification
they feed, and what the same walk costs on the host.  One JSON line per point: each parameter set at --n certificates, and an even
three-way mix of --n certificates.

The batch is chains of depth 3 -- a self-signed root, an intermediate, a leaf -- of v3 certificates with 21-byte Names and no
extensions, validly signed on the device (a chain is of one parameter set; in the mix the chains take the sets in turn).  Certificates
lie 5 mod 16 bytes apart, so keys, signatures and TBS fall on every byte alignment.  Per point, alternating in one process after
warm-up, hipEvent times of --inner calls per sample, --rounds samples, median and p10-p90:
  a  mldsa_x509_ops on the blob: parse + link with MLDSA_X509_CHECK_NAMES          the code this tool is about
  b  mldsa_rec_verify on the ops a produced                                        the comparison point, in the same run
  c  a then b, as MlDsaCertificates.verify_device makes them                       what a caller sees
  d  a plain Python walk of the same certificates on the host                      host clock, on --host-certs of them, scaled to --n
a / b is what the walk adds to the verification, d / a what the host walk costs instead.  Every verdict of c is checked to be 1.
Nothing is gated on the ratios.

    python tools/bench_x509.py > profiles/x509_bench.jsonl
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


def template(pset, pk_len, sig_len):
    """a certificate of the set with zero key, signature and Name digits: (bytes, positions of issuer digits, subject digits, key,
    signature, TBS and its length)"""
    alg = tlv(0x30, OID + bytes([{44: 0x11, 65: 0x12, 87: 0x13}[pset]]))
    name = tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, b"0" * 8))))
    dates = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))
    head = tlv(0xA0, b"\x02\x01\x02") + tlv(0x02, b"\x12\x34") + alg
    tbs = tlv(0x30, head + name + dates + name + tlv(0x30, alg + tlv(0x03, bytes(1 + pk_len))))
    der = tlv(0x30, tbs + alg + tlv(0x03, bytes(1 + sig_len)))
    issuer_at = 8 + len(head) + len(name) - 8
    subject_at = issuer_at + len(dates) + len(name)
    return der, issuer_at, subject_at, len(tbs) + 4 - pk_len, len(der) - sig_len, 4, len(tbs)


def host_walk(buf, off, length):
    """the walk of include/mldsa_x509.h in plain Python: (tbs_off, tbs_len, key_off, sig_off, issuer Name, subject Name) or None"""
    def item(pos, end):
        if pos + 2 > end or buf[pos] & 0x1F == 0x1F:
            raise ValueError
        first, header, n = buf[pos + 1], 2, buf[pos + 1]
        if first >= 0x80:
            k = first & 0x7F
            if k == 0 or k > 4 or pos + 2 + k > end or buf[pos + 2] == 0:
                raise ValueError
            n, header = int.from_bytes(buf[pos + 2:pos + 2 + k], "big"), 2 + k
            if n < 128:
                raise ValueError
        if pos + header + n > end:
            raise ValueError
        return buf[pos], pos + header, pos + header + n

    def want(pos, end, tag):
        got, at, behind = item(pos, end)
        if got != tag:
            raise ValueError
        return at, behind
    try:
        end = off + length
        at, behind = want(off, end, 0x30)
        tbs_at, tbs_end = want(at, end, 0x30)
        alg_at, alg_end = want(tbs_end, end, 0x30)
        sig_at, sig_end = want(alg_end, end, 0x03)
        pos = tbs_at
        if item(pos, tbs_end)[0] == 0xA0:
            pos = item(pos, tbs_end)[2]
        inner = want(pos, tbs_end, 0x02)[1]          # where the inner algorithm begins, behind the serial number
        issuer = want(inner, tbs_end, 0x30)[1]       # ... the issuer Name
        validity = want(issuer, tbs_end, 0x30)[1]
        subject = want(validity, tbs_end, 0x30)[1]
        spki = want(subject, tbs_end, 0x30)[1]
        spki_at, spki_end = want(spki, tbs_end, 0x30)
        kalg_end = want(spki_at, spki_end, 0x30)[1]
        key_at, key_end = want(kalg_end, spki_end, 0x03)
        if behind != end or sig_end != end or key_end != spki_end or buf[inner:issuer] != buf[tbs_end:alg_end] or buf[alg_at:alg_at + 10] != OID:
            return None
        return at, tbs_end - at, key_at + 1, sig_at + 1, buf[issuer:validity], buf[subject:spki]
    except ValueError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-certs", type=int, default=1024, help="certificates the host walk is timed on")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _x509_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa, MlDsaCertificates

    assert torch.cuda.is_available(), "bench_x509.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    x5 = MlDsaCertificates(hotpath=hp)
    sets = {s: MlDsa(s, hotpath=hp) for s in (44, 65, 87)}
    keys = {}
    for pset, m in sets.items():
        pk, sk = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(args.keys)])
        keys[pset] = (pk, m.private_keys_from_bytes(sk))

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
        certs = np.zeros(n, dtype=_x509_lib.CERT_DTYPE)
        certs["issuer"] = issuer
        blocks, base, tbs_bytes = [], 3, 0
        for c, pset in enumerate(psets):
            m = sets[pset]
            mine = order[set_of == c]
            der, issuer_at, subject_at, key_at, sig_at, tbs_at, tbs_len = template(pset, m.PK_LEN, m.SIG_LEN)
            stride = len(der) + (5 - len(der)) % 16            # certificates 5 mod 16 bytes apart: they fall on all sixteen residues
            rows = torch.from_numpy(np.frombuffer(der + bytes(stride - len(der)), dtype=np.uint8).copy()).cuda().repeat(len(mine), 1)
            rows[:, issuer_at:issuer_at + 8] = torch.from_numpy(digits(issuer[mine])).cuda()
            rows[:, subject_at:subject_at + 8] = torch.from_numpy(digits(mine)).cuda()
            kidx = mine * 2654435761 % args.keys               # the subject key of every certificate, and through it its issuer's
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
        certs_d = x5.certs_tensor(certs)
        fields = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
        ops = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        scratch = x5.records.verify_scratch(n, tbs_bytes, 0)

        def run_a():
            _x509_lib.check(x5.lib.mldsa_x509_ops(hp._h, _ptr(blob), blob.numel(), _ptr(certs_d), n, _x509_lib.CHECK_NAMES, _ptr(fields), _ptr(ops),
                                                  _ptr(status), _stream(x5.device)))

        run = {"a": run_a, "b": lambda: x5.records.verify_device(blob, ops, ok, n, scratch=scratch),
               "c": lambda: x5.verify_device(blob, certs_d, ok, status=status, scratch=scratch)}
        run_a()  # (b takes a's ops from its first sample on)
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
        assert not bool(status.any()) and bool(ok.all()), "a certificate of the batch did not verify"

        # the host walk: the blob lies in host memory, Python reads each certificate's structure and compares the Names
        blob_h = blob.cpu().numpy().tobytes()
        fields_h = fields.cpu().numpy().view(_x509_lib.FIELDS_DTYPE)
        k = min(args.host_certs, n)
        t0 = time.perf_counter()
        walked = [host_walk(blob_h, int(certs[i]["off"]), int(certs[i]["len"])) for i in range(k)]
        linked = [walked[i] is not None and walked[int(issuer[i])] is not None and walked[i][4] == walked[int(issuer[i])][5] for i in range(k)]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(linked)
        for i in range(k):
            assert walked[i][:4] == tuple(int(fields_h[i][f]) for f in ("tbs_off", "tbs_len", "key_off", "sig_off")), i
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_ = (st[v]["median_ms"] for v in "abc")
        d = host_ms * n / k
        print(json.dumps({
            "workload": "x509_ops", "label": args.label, "point": point, "n_certs": n, "chain_depth": 3, "keys_per_set": args.keys,
            "blob_bytes": int(blob.numel()), "tbs_bytes": int(tbs_bytes), "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host walk: host clock around the walk of host_certs certificates, scaled",
            "a_x509_ops": st["a"], "b_rec_verify_on_the_ops": st["b"], "c_verify_device": st["c"],
            "d_host_walk_ms_scaled": round(d, 1), "host_certs": k, "host_walk_us_per_cert": round(host_ms * 1e3 / k, 2),
            "a_ns_per_cert": round(a * 1e6 / n, 2), "b_Mverifies_s": round(n / b / 1e3, 2),
            "a_over_b_time": round(a / b, 4), "c_over_b_time": round(c_ / b, 3), "d_over_a_time": round(d / a, 1)}), flush=True)
        del blob, certs_d, fields, ops, status, ok, scratch, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
