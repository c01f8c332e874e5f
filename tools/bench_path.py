#!/usr/bin/env python3
"""Path validation on the device (include/mldsa_path.h): what the policy walk and the climb cost next to the calls they stand beside,
and what the same work costs on the host.  One JSON line per point: each parameter set at --n certificates, and an even three-way mix.

The batch is that of tools/bench_x509.py -- chains of depth 3, a self-signed root (the trust anchor), an intermediate, a leaf, validly
signed on the device, 5 mod 16 bytes apart -- with three extensions in every certificate: basicConstraints (cA), keyUsage and one
this library does not read.  Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds
samples, median and p10-p90:
  a  mldsa_path_parse                                                              the policy walk
  b  mldsa_x509_parse on the same certificates                                     its comparison point: the walk it extends
  c  mldsa_path_chain: k_path_node + k_path_climb                                  the climb
  d  a device-to-device copy of the node array (8 bytes per certificate)           its comparison point: the traffic floor
  e  mldsa_x509_ops, mldsa_rec_verify, mldsa_path_parse, mldsa_path_chain          the whole route without CRLs, as a caller sees it
  f  a plain Python walk, policy walk and climb of the same certificates           host clock, on --host-certs of them, scaled to --n
Every verdict of e is checked to be TRUSTED.  Nothing is gated on the ratios.

    python tools/bench_path.py > profiles/path_bench.jsonl
"""
import argparse
import calendar
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_x509 import OID, host_walk, tlv  # noqa: E402

TAIL = tlv(0xA3, tlv(0x30, tlv(0x30, bytes.fromhex("0603551d13") + b"\x01\x01\xff" + tlv(0x04, tlv(0x30, b"\x01\x01\xff"))) +
                     tlv(0x30, bytes.fromhex("0603551d0f") + b"\x01\x01\xff" + tlv(0x04, bytes.fromhex("03020106"))) +
                     tlv(0x30, bytes.fromhex("0603551d0e") + tlv(0x04, tlv(0x04, bytes(range(20)))))))
NOW = calendar.timegm((2030, 1, 1, 0, 0, 0))


def template(pset, pk_len, sig_len):
    """bench_x509's certificate with TAIL behind the key: (bytes, positions of issuer digits, subject digits, key, signature, TBS, its length)"""
    alg = tlv(0x30, OID + bytes([{44: 0x11, 65: 0x12, 87: 0x13}[pset]]))
    name = tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, b"0" * 8))))
    dates = tlv(0x30, tlv(0x17, b"250101000000Z") + tlv(0x17, b"350101000000Z"))
    head = tlv(0xA0, b"\x02\x01\x02") + tlv(0x02, b"\x12\x34") + alg
    tbs = tlv(0x30, head + name + dates + name + tlv(0x30, alg + tlv(0x03, bytes(1 + pk_len))) + TAIL)
    der = tlv(0x30, tbs + alg + tlv(0x03, bytes(1 + sig_len)))
    issuer_at = 8 + len(head) + len(name) - 8
    subject_at = issuer_at + len(dates) + len(name)
    return der, issuer_at, subject_at, len(tbs) + 4 - pk_len - len(TAIL), len(der) - sig_len, 4, len(tbs)


def host_time(text):
    """seconds of a UTCTime's 13 content bytes"""
    yy = int(text[0:2])
    return calendar.timegm((2000 + yy if yy < 50 else 1900 + yy, int(text[2:4]), int(text[4:6]), int(text[6:8]), int(text[8:10]), int(text[10:12])))


def host_policy(buf, walked):
    """the policy walk in plain Python behind host_walk's: (not_before, not_after, is_ca, key_cert_sign) of a v3 certificate"""
    tbs_off, tbs_len, key_off = walked[0], walked[1], walked[2]
    tbs_end = tbs_off + tbs_len
    at = buf.index(b"\x30\x1e\x17\x0d", tbs_off, key_off)  # the validity of two UTCTimes
    not_before, not_after = host_time(buf[at + 4:at + 17]), host_time(buf[at + 19:at + 32])
    pos = tbs_end - len(TAIL) + 2  # behind the [3] header: the Extensions SEQUENCE
    end = pos + 2 + buf[pos + 1]
    pos += 2
    is_ca = sign = False
    while pos < end:
        ext_end = pos + 2 + buf[pos + 1]
        oid = buf[pos + 4:pos + 4 + buf[pos + 3]]
        value = buf[ext_end - (3 if oid == b"\x55\x1d\x13" else 2):ext_end]
        if oid == b"\x55\x1d\x13":
            is_ca = value == b"\x01\x01\xff"
        elif oid == b"\x55\x1d\x0f":
            sign = bool(value[1] & 0x04)
        pos = ext_end
    return not_before, not_after, is_ca, sign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,mix")
    ap.add_argument("--keys", type=int, default=1024, help="keys per parameter set")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-certs", type=int, default=1023, help="certificates the host walk is timed on (whole chains)")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _path_lib, _x509_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa, MlDsaPathValidator

    assert torch.cuda.is_available(), "bench_path.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    pv = MlDsaPathValidator(hotpath=hp)
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
        n = args.n
        order = np.arange(n)
        set_of = (order // 3) % len(psets)
        issuer = np.where(order % 3 == 0, order, order - 1)
        certs = np.zeros(n, dtype=_x509_lib.CERT_DTYPE)
        certs["issuer"] = issuer
        blocks, base, tbs_bytes = [], 3, 0
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
        certs_d = x5.certs_tensor(certs)
        anchor = torch.from_numpy((order % 3 == 0).astype(np.uint8)).cuda()
        fields = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
        policy = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        ops = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        results = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
        nodes = torch.empty(max(pv.lib.mldsa_path_scratch_bytes(n), 256), dtype=torch.uint8, device="cuda")
        nodes_copy = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
        scratch = x5.records.verify_scratch(n, tbs_bytes, 0)
        h, s = hp._h, _stream(pv.device)

        def run_a():
            _path_lib.check(pv.lib.mldsa_path_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, 0, _ptr(policy), s))

        def run_b():
            _x509_lib.check(x5.lib.mldsa_x509_parse(h, _ptr(blob), blob.numel(), _ptr(certs_d), n, _ptr(fields), s))

        def run_c():
            _path_lib.check(pv.lib.mldsa_path_chain(h, _ptr(certs_d), _ptr(policy), _ptr(status), _ptr(ok), None, _ptr(anchor), n, NOW, 0, _ptr(results),
                                                    _ptr(nodes), nodes.numel(), s))

        def run_e():
            x5.verify_device(blob, certs_d, ok, status=status, scratch=scratch)
            run_a()
            run_c()

        run = {"a": run_a, "b": run_b, "c": run_c, "d": lambda: nodes_copy.copy_(nodes[:n * 8]), "e": run_e}
        run_e()  # (c takes status, ok and policy from here on)
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
        res = results.cpu().numpy().view(_path_lib.RESULT_DTYPE)
        assert not res["verdict"].any() and np.array_equal(res["depth"], order % 3), "a certificate of the batch is not trusted"

        # the host: the blob lies in host memory, Python walks each certificate, reads its policy and climbs its chain
        blob_h = blob.cpu().numpy().tobytes()
        policy_h = policy.cpu().numpy().view(_path_lib.FIELDS_DTYPE)
        k = min(args.host_certs, n) // 3 * 3
        t0 = time.perf_counter()
        walked = [host_walk(blob_h, int(certs[i]["off"]), int(certs[i]["len"])) for i in range(k)]
        rules = [host_policy(blob_h, w) for w in walked]
        verdicts = []
        for i in range(k):
            a, trusted = i, True
            for depth in range(17):
                if a % 3 == 0:  # the anchor
                    break
                nb, na, is_ca, sign = rules[a]
                trusted = trusted and nb <= NOW <= na and (depth == 0 or (is_ca and sign)) and walked[a][4] == walked[int(issuer[a])][5]
                a = int(issuer[a])
            verdicts.append(trusted)
        host_ms = (time.perf_counter() - t0) * 1e3
        assert all(verdicts)
        for i in range(k):
            assert rules[i][:2] == (int(policy_h[i]["not_before"]), int(policy_h[i]["not_after"])) and policy_h[i]["flags"] == 15, i
        st = {v: stats(t) for v, t in times.items()}
        a, b, c_, d, e = (st[v]["median_ms"] for v in "abcde")
        f = host_ms * n / k
        print(json.dumps({
            "workload": "path", "label": args.label, "point": point, "n_certs": n, "chain_depth": 3, "extensions": 3, "keys_per_set": args.keys,
            "blob_bytes": int(blob.numel()), "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host: host clock around walk, policy and climb of host_certs certificates, scaled",
            "a_path_parse": st["a"], "b_x509_parse": st["b"], "c_path_chain": st["c"], "d_copy_of_the_nodes": st["d"], "e_whole_route": st["e"],
            "f_host_ms_scaled": round(f, 1), "host_certs": k, "host_us_per_cert": round(host_ms * 1e3 / k, 2),
            "a_ns_per_cert": round(a * 1e6 / n, 2), "c_ns_per_cert": round(c_ * 1e6 / n, 2),
            "a_over_b_time": round(a / b, 3), "c_over_d_time": round(c_ / d, 3), "a_plus_c_over_e_time": round((a + c_) / e, 4),
            "f_over_e_time": round(f / e, 1)}), flush=True)
        del blob, certs_d, fields, policy, ops, status, ok, results, nodes, nodes_copy, scratch, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
