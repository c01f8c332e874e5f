#!/usr/bin/env python3
"""Certificate revocation lists on the device (include/mldsa_crl.h): what the walk of the CRLs and of their entries costs next to the
signature check it feeds, what building the lookup table costs next to a plain copy of the entry rows, what the lookup costs next to the
certificates' own walk, and what walking and looking up on the host costs instead.  One JSON line per point: --crls CRLs of --entries
entries for each parameter set, and one CRL of --big entries (ML-DSA-44).

The batch: one self-signed CA certificate around a real key, CRLs under its Name (v2, thisUpdate and nextUpdate, entries of 27 bytes: an
8-byte serial and a UTCTime, no extensions), each signed on the device by the CA's key (mldsa_recsign_sign writes the signature into the
CRL's BIT STRING), and --certs leaf certificates under the same Name whose 8-byte serials are 0, 1, 2, ...: the CRLs list the even
numbers, so every second certificate is revoked as long as the lists reach that far.  CRLs and certificates lie 5 mod 16 bytes apart.
Per point, alternating in one process after warm-up, hipEvent times of --inner calls per sample, --rounds samples, median and p10-p90:
  p  mldsa_crl_parse                                                                  the header walk alone
  a  mldsa_crl_ops: clear + parse + place + entries + link                            the walk
  b  mldsa_rec_verify on the ops a produced                                           its comparison point, in the same run
  t  mldsa_crl_table: clear + insert                                                  the table
  g  a device-to-device copy of the entry rows                                        its comparison point, in the same run
  k  mldsa_crl_check on the certificates                                              the lookup
  x  mldsa_x509_ops on the same certificates                                          its comparison point, in the same run
  h  the host route: a Python walk of the CRLs' entries into a set of serials (host clock, on --host-entries entries, scaled) and the
     lookup of the certificates' serials in it (host clock, on --host-certs certificates, scaled)
(a - p) over the entries is the hop's share of the walk: place, entries and link, of which the entry kernel is all but a few
microseconds.  Every CRL is checked to be accepted and to verify, the totals to count every entry, the table not to overflow and the
answers to be the expected pattern.  Nothing is gated on the ratios.

    python tools/bench_crl.py > profiles/crl_bench.jsonl
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
ENTRY_LEN = 27


def tlv(tag, body):
    n = len(body)
    if n < 128:
        return bytes([tag, n]) + body
    digits = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag, 0x80 | len(digits)]) + digits + body


def alg_id(pset):
    return tlv(0x30, OID + bytes([{44: 0x11, 65: 0x12, 87: 0x13}[pset]]))


def name(cn):
    return tlv(0x30, tlv(0x31, tlv(0x30, bytes.fromhex("0603550403") + tlv(0x0C, cn))))


WHEN = tlv(0x17, b"250101000000Z")
DATES = tlv(0x30, WHEN + tlv(0x17, b"350101000000Z"))
CA_NAME = name(b"bench CA")


def crl_template(pset, n_entries, sig_len):
    """a CRL with zero serials and signature: (bytes, position and length of the tbsCertList, of the first serial, of the signature)"""
    alg = alg_id(pset)
    revoked = tlv(0x30, tlv(0x30, tlv(0x02, bytes(8)) + WHEN) * n_entries)
    tbs = tlv(0x30, tlv(0x02, b"\x01") + alg + CA_NAME + WHEN + WHEN + revoked)
    der = tlv(0x30, tbs + alg + tlv(0x03, bytes(1 + sig_len)))
    tbs_at = der.index(tbs)
    first_serial = tbs_at + len(tbs) - ENTRY_LEN * n_entries + 4
    assert der[first_serial - 4:first_serial] == b"\x30\x19\x02\x08"
    return der, tbs_at, len(tbs), first_serial, len(der) - sig_len


def cert_template(pset, pk, sig_len, subject):
    """a certificate under the CA's Name with a zero 8-byte serial and signature: (bytes, position of the serial)"""
    alg = alg_id(pset)
    tbs = tlv(0x30, tlv(0xA0, b"\x02\x01\x02") + tlv(0x02, bytes(8)) + alg + CA_NAME + DATES + subject + tlv(0x30, alg + tlv(0x03, b"\x00" + pk)))
    der = tlv(0x30, tbs + alg + tlv(0x03, bytes(1 + sig_len)))
    at = der.index(b"\x02\x08" + bytes(8)) + 2
    return der, at


def host_take(der, pos):
    tag, first = der[pos], der[pos + 1]
    if first < 0x80:
        return tag, pos + 2, pos + 2 + first
    k = first & 0x7F
    return tag, pos + 2 + k, pos + 2 + k + int.from_bytes(der[pos + 2:pos + 2 + k], "big")


def host_list(der):
    """(position of the first entry, end of the list) of one CRL, by a plain Python walk of its header"""
    _, at, _ = host_take(der, 0)
    _, pos, _ = host_take(der, at)
    for _ in range(5):  # version, algorithm, issuer, thisUpdate, nextUpdate
        _, _, pos = host_take(der, pos)
    _, at, end = host_take(der, pos)
    return at, end


def host_entries(der, pos, end, limit, crl, into):
    """walks up to `limit` entries into the set: the entry's header, the serial's, the date's"""
    done = 0
    while pos < end and done < limit:
        _, at, behind = host_take(der, pos)
        _, s_at, s_end = host_take(der, at)
        _, _, d_end = host_take(der, s_end)
        assert d_end == behind
        into.add((crl, der[s_at:s_end]))
        pos = behind
        done += 1
    return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crls", type=int, default=4096)
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--big", type=int, default=262144, help="entries of the one CRL of the last point")
    ap.add_argument("--certs", type=int, default=65536)
    ap.add_argument("--points", default="44,65,87,one")
    ap.add_argument("--rounds", type=int, default=12, help="samples per device variant and point")
    ap.add_argument("--host-entries", type=int, default=32768, help="entries the host walk is timed on")
    ap.add_argument("--host-certs", type=int, default=2048, help="certificates the host lookup is timed on")
    ap.add_argument("--inner", type=int, default=1, help="calls per sample")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per point")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fips204_amd import _crl_lib, _recsign_lib, _x509_lib
    from fips204_amd.hotpath import HotPath, _ptr, _stream
    from fips204_amd.ml_dsa import MlDsa, MlDsaRecordSigner, MlDsaRevocationLists

    assert torch.cuda.is_available(), "bench_crl.py measures on the GPU; there is no other path"
    hp = HotPath(0)
    rl = MlDsaRevocationLists(hotpath=hp)
    x5 = rl.certificates
    signer = MlDsaRecordSigner(hotpath=hp)
    lib, s = rl.lib, _stream(rl.device)

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def rows_of(der, n):
        """[n, stride] uint8: n copies of der, 5 mod 16 bytes apart"""
        stride = len(der) + (5 - len(der)) % 16
        return np.tile(np.frombuffer(der + bytes(stride - len(der)), dtype=np.uint8), (n, 1)), stride

    def put_numbers(rows, cols, values):
        """the 7 low bytes of values [n, len(cols)] big-endian at rows[:, cols + 1 ... cols + 7]; the byte at cols is 0x01"""
        rows[:, cols] = 0x01
        for b in range(7):
            rows[:, cols + 1 + b] = ((values >> np.uint64(8 * (6 - b))) & np.uint64(0xFF)).astype(np.uint8)

    for point in args.points.split(","):
        pset = 44 if point == "one" else int(point)
        n, per = (1, args.big) if point == "one" else (args.crls, args.entries)
        m = MlDsa(pset, hotpath=hp)
        pk, sk = m.keygen_from_seed([bytes([pset]) * 32])
        signer.set_keys(pset, m.private_keys_from_bytes(sk))
        ca, _ = cert_template(pset, pk[0].cpu().numpy().tobytes(), m.SIG_LEN, CA_NAME)
        ca = ca.replace(b"\x02\x08" + bytes(8), b"\x02\x08\x7f" + bytes(7), 1)
        # the CRLs: entry j of CRL i lists the serial 2 (i * per + j)
        der, tbs_at, tbs_len, first_serial, sig_at = crl_template(pset, per, m.SIG_LEN)
        crl_rows, crl_stride = rows_of(der, n)
        listed = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(per) + np.arange(per, dtype=np.uint64)[None, :]) * np.uint64(2)
        put_numbers(crl_rows, first_serial + ENTRY_LEN * np.arange(per), listed)
        # the certificates: serial k, covered by the CRL that would list it
        leaf, serial_at = cert_template(pset, bytes(m.PK_LEN), m.SIG_LEN, name(b"bench leaf"))
        leaf_rows, leaf_stride = rows_of(leaf, args.certs)
        numbers = np.arange(args.certs, dtype=np.uint64)
        put_numbers(leaf_rows, np.array([serial_at]), numbers[:, None])
        crl_base = 3 + len(ca) + (5 - (3 + len(ca))) % 16
        leaf_base = crl_base + n * crl_stride
        blob_h = np.concatenate([np.zeros(3, np.uint8), np.frombuffer(ca, dtype=np.uint8), np.zeros(crl_base - 3 - len(ca), np.uint8),
                                 crl_rows.reshape(-1), leaf_rows.reshape(-1)])
        del crl_rows, leaf_rows
        blob = torch.from_numpy(blob_h).cuda()
        items = np.zeros(n, dtype=_crl_lib.ITEM_DTYPE)
        items["off"], items["len"] = crl_base + np.arange(n, dtype=np.uint64) * np.uint64(crl_stride), len(der)
        certs = np.zeros(1 + args.certs, dtype=_x509_lib.CERT_DTYPE)
        certs["off"][0], certs["len"][0] = 3, len(ca)
        certs["off"][1:], certs["len"][1:] = leaf_base + numbers * np.uint64(leaf_stride), len(leaf)
        cover = np.zeros(1 + args.certs, dtype=np.uint32)
        cover[0] = _crl_lib.NONE
        cover[1:] = np.minimum(numbers // np.uint64(2 * per), np.uint64(n - 1)).astype(np.uint32)
        want = np.where((numbers % np.uint64(2) == 0) & (numbers // np.uint64(2) < np.uint64(n * per)), _crl_lib.REVOKED, _crl_lib.GOOD).astype(np.uint8)
        # every CRL signed by the CA's key, in place
        sign_ops = np.zeros(n, dtype=_recsign_lib.OP_DTYPE)
        sign_ops["msg_off"], sign_ops["msg_len"], sign_ops["sig_off"], sign_ops["set"] = items["off"] + np.uint64(tbs_at), tbs_len, items["off"] + np.uint64(sig_at), pset
        sst = torch.zeros(n, dtype=torch.int32, device="cuda")
        signer.sign_device(blob, signer.ops_tensor(sign_ops), blob, sst, n, 0, scratch=signer.sign_scratch(n, n * tbs_len, 0))
        torch.cuda.synchronize()
        assert not bool(sst.any()), "a CRL of the batch was not signed"

        n_certs = 1 + args.certs
        certs_d, items_d = x5.certs_tensor(certs), rl.items_tensor(items)[:n * 16]
        cover_d = torch.from_numpy(cover.view(np.int32).copy()).cuda()
        cert_fields = torch.empty(n_certs * 56, dtype=torch.uint8, device="cuda")
        cert_ops = torch.empty(n_certs * 40, dtype=torch.uint8, device="cuda")
        cert_status = torch.empty(n_certs, dtype=torch.uint8, device="cuda")
        max_entries = n * int(lib.mldsa_crl_entries_bound(ENTRY_LEN * per))
        slots = int(lib.mldsa_crl_table_slots(max_entries))
        fields = torch.empty(n * 88, dtype=torch.uint8, device="cuda")
        entries = torch.empty(max_entries * 32, dtype=torch.uint8, device="cuda")
        ops = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.uint8, device="cuda")
        totals = torch.zeros(5, dtype=torch.int64, device="cuda")
        scratch = torch.empty(max(int(lib.mldsa_crl_scratch_bytes(n)), 256), dtype=torch.uint8, device="cuda")
        table = torch.empty(slots, dtype=torch.int32, device="cuda")
        copy_to = torch.empty_like(entries)
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rev = torch.empty(n_certs, dtype=torch.uint8, device="cuda")
        vscratch = rl.records.verify_scratch(n, n * tbs_len, 0)

        def run_x():
            _x509_lib.check(x5.lib.mldsa_x509_ops(hp._h, _ptr(blob), blob.numel(), _ptr(certs_d), n_certs, 1, _ptr(cert_fields), _ptr(cert_ops),
                                                  _ptr(cert_status), s))

        def run_p():
            _crl_lib.check(lib.mldsa_crl_parse(hp._h, _ptr(blob), blob.numel(), _ptr(items_d), n, _ptr(fields), s))

        def run_a():
            _crl_lib.check(lib.mldsa_crl_ops(hp._h, _ptr(blob), blob.numel(), _ptr(items_d), n, _ptr(cert_fields), n_certs, 1, _ptr(fields),
                                             _ptr(entries), max_entries, _ptr(ops), _ptr(status), _ptr(totals), _ptr(scratch), scratch.numel(), s))

        def run_b():
            rl.records.verify_device(blob, ops, ok, n, 0, scratch=vscratch)

        def run_t():
            _crl_lib.check(lib.mldsa_crl_table(hp._h, _ptr(entries), max_entries, _ptr(table), slots, _ptr(totals), s))

        def run_k():
            _crl_lib.check(lib.mldsa_crl_check(hp._h, _ptr(blob), blob.numel(), _ptr(certs_d), _ptr(cert_fields), _ptr(cover_d), n_certs, _ptr(items_d),
                                               _ptr(fields), _ptr(status), _ptr(ok), n, _ptr(entries), max_entries, _ptr(table), slots, _ptr(rev), s))

        run = {"x": run_x, "p": run_p, "a": run_a, "b": run_b, "t": run_t, "g": lambda: copy_to.copy_(entries), "k": run_k}
        times = {v: [] for v in run}
        for r in range(args.warmup + args.rounds):
            for v, fn in run.items():  # alternating: every round takes one sample of every variant, each on what the ones before left
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    fn()
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[v].append(e0.elapsed_time(e1) / args.inner)
        torch.cuda.synchronize()
        tot = totals.cpu().numpy().view(_crl_lib.TOTALS_DTYPE)[0]
        assert not bool(status.any()) and bool(ok.all()) and not bool(cert_status.any()), "a CRL or a certificate of the batch was refused"
        assert (int(tot["accepted"]), int(tot["entries"]), int(tot["slots"]), int(tot["overflow"])) == (n, n * per, max_entries, 0), tot
        got = rev.cpu().numpy()
        assert got[0] == _crl_lib.NO_CRL and np.array_equal(got[1:], want), "the lookup's answers are not the expected pattern"

        # the host route: Python walks the entries into a set and looks the certificates' serials up
        raw = blob_h.tobytes()
        seen, walked, left = set(), 0, min(args.host_entries, n * per)
        t0 = time.perf_counter()
        for i in range(n):
            if left == 0:
                break
            one = raw[int(items[i]["off"]):int(items[i]["off"]) + int(items[i]["len"])]
            at, end = host_list(one)
            done = host_entries(one, at, end, left, i, seen)
            walked += done
            left -= done
        walk_ms = (time.perf_counter() - t0) * 1e3
        kc = min(args.host_certs, args.certs)
        t0 = time.perf_counter()
        hits = 0
        for j in range(1, 1 + kc):
            one = raw[int(certs[j]["off"]):int(certs[j]["off"]) + int(certs[j]["len"])]
            _, at, _ = host_take(one, 0)
            _, at, _ = host_take(one, at)
            _, _, pos = host_take(one, at)
            _, s_at, s_end = host_take(one, pos)
            hits += (int(cover[j]), one[s_at:s_end]) in seen
        look_ms = (time.perf_counter() - t0) * 1e3
        assert walked > 0 and hits > 0
        st = {v: stats(t) for v, t in times.items()}
        x, p, a, b, t, g, k = (st[v]["median_ms"] for v in "xpabtgk")
        h = walk_ms * n * per / walked + look_ms * args.certs / kc
        print(json.dumps({
            "workload": "crl_check", "label": args.label, "point": point, "set": pset, "n_crls": n, "entries_per_crl": per, "n_certs": n_certs,
            "blob_bytes": int(blob.numel()), "crl_bytes": len(der), "revoked_bytes": ENTRY_LEN * per * n, "max_entries": max_entries,
            "table_slots": slots, "rounds": args.rounds, "calls_per_sample": args.inner,
            "clock": "hipEvent pair around the calls of a sample; host route: host clock around the walk of host_entries entries and the lookup "
                     "of host_certs certificates, each scaled",
            "p_parse": st["p"], "a_crl_ops": st["a"], "b_rec_verify_on_the_ops": st["b"], "t_table": st["t"], "g_copy_of_the_entry_rows": st["g"],
            "k_check": st["k"], "x_x509_ops_on_the_certificates": st["x"], "host_entries": walked, "host_certs": kc,
            "host_walk_us_per_entry": round(walk_ms * 1e3 / walked, 3), "host_lookup_us_per_cert": round(look_ms * 1e3 / kc, 3),
            "h_host_route_ms": round(h, 1), "entries_per_s_of_crl_ops": round(n * per / a * 1e3), "entries_per_s_of_the_hop": round(n * per / max(a - p, 1e-6) * 1e3),
            "a_over_b_time": round(a / b, 4), "t_over_g_time": round(t / g, 2), "k_over_x_time": round(k / x, 3), "k_ns_per_cert": round(k * 1e6 / n_certs, 2),
            "h_over_a_t_k_time": round(h / (a + t + k), 1)}), flush=True)
        del blob, blob_h, raw, certs_d, items_d, cover_d, cert_fields, cert_ops, cert_status, fields, entries, ops, status, table, copy_to, ok, rev, vscratch, run
        torch.cuda.empty_cache()
    hp.close()


if __name__ == "__main__":
    main()
