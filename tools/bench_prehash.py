#!/usr/bin/env python3
"""HashML-DSA with the pre-hash on the device (include/mldsa_ph.h) against the host pre-hash, ML-DSA-65: one JSON line per
(message length, PH) point.

Per point: mldsa_prehash alone (us, GB/s of message, fraction of the derived issue ceiling), hash_verify_device and
hash_sign_device (ms), the same calls with the host pre-hash (hashlib loop included), and pure-mode verify_device /
sign_device on the same raw messages (one lane-per-message pass over the bytes in k_mu).  Device times are hipEvent times
after warm-up; host-path times are wall clock around the whole list-level call.

The ceiling: cycles per block per wave = sum over the kernel's instruction classes of count x issue cost.  The counts are
those of k_prehash<PH>'s compression loop in its disassembly (llvm-objdump -d --mcpu=gfx950 of the device object of
fips204_amd/ph/prehash.hip); the issue costs are the column cyc/instr@clk of tools/ubench_valu.hip's output (--ubench FILE).
Ceiling GB/s = SIMDs x clock x 64 lanes x block bytes / cycles per block, for one message per lane and full issue.

    python tools/bench_prehash.py --ubench profiles/prehash_ubench_valu.txt > profiles/prehash_bench.jsonl

--stream runs the legs of the incremental pre-hash and of the host-memory calls instead, one JSON line each:
  prehash_stream   mldsa_ph_init + updates + final (1 piece, 4 equal pieces; hipEvent time) against mldsa_prehash of the same run
  hash_host        mldsa_hash_verify_host / _sign_host on page-locked buffers (wall clock) against (i) the hashlib loop +
                   verify_host / sign_host in MLDSA_MODE_PREHASH and (ii) those calls on precomputed rows + message bytes / the
                   measured page-locked H2D rate
  staging_sweep    mldsa_hash_verify_host at --sweep-len bytes per message for staging chunks of --sweep-mib MiB

    python tools/bench_prehash.py --stream >> profiles/prehash_stream_bench.jsonl

--phs takes any of the twelve Ph names of fips204_amd.ml_dsa.  --lib PATH measures another build of libmldsa_ph.so (the parent
commit's, or one compiled with -DMLDSA_PH_COOP_MAX_OPS=0) through the same Python, and --label TEXT tags every line with it.
--small measures the small-call latency instead: mldsa_prehash and hash_verify_device for --ns operations, the host clock around
a call that ends in a synchronise, --calls calls after warm-up, median and percentiles (one JSON line per PH, length and n).

    python tools/bench_prehash.py --small --phs SHAKE256,SHA3_512 --lens 1024,16384 --label wave >> profiles/prehash_fips_list_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIMDS, CLOCK_GHZ = 256 * 4, 2.4
BLOCK_BYTES = {"SHA256": 64, "SHA224": 64, "SHA512": 128, "SHA384": 128, "SHA512_224": 128, "SHA512_256": 128,
               "SHAKE128": 168, "SHA3_224": 144, "SHA3_256": 136, "SHAKE256": 136, "SHA3_384": 104, "SHA3_512": 72}
# instruction classes of one block of one wave, from the disassembly of k_prehash<PH> (counts of the compression / permutation loop)
MIX = {
    "SHA256": {"v_alignbit_b32": 576, "v_bitop3_b32": 352, "v_add3_u32": 241, "v_add_u32": 119, "v_lshrrev_b32": 96, "v_perm_b32": 16},
    "SHA512": {"v_alignbit_b32": 1570, "v_bitop3_b32": 896, "v_lshl_add_u64": 768, "v_add3_u32": 448, "v_mov_b32": 992,
               "v_add_u32": 247, "v_lshrrev_b32": 128, "v_perm_b32": 32},
}
# the functions of a family run the same compression loop: only initial value and digest length differ
MIX.update({"SHA224": MIX["SHA256"], "SHA384": MIX["SHA512"], "SHA512_224": MIX["SHA512"], "SHA512_256": MIX["SHA512"]})
# Keccak family: 24 rounds of csrc/keccak.h (70 bitop3 + 58 alignbit + 62 xor per round) + one absorbing XOR per dword of the rate
MIX.update({ph: {"v_bitop3_b32": 24 * 70, "v_alignbit_b32": 24 * 58, "v_xor_b32": 24 * 62 + BLOCK_BYTES[ph] // 4}
            for ph in ("SHAKE128", "SHA3_224", "SHA3_256", "SHAKE256", "SHA3_384", "SHA3_512")})


def issue_costs(path):
    """instruction -> cycles per wave64 instruction (cyc/instr@clk) from a ubench_valu output file"""
    costs = {}
    for ln in open(path):
        parts = ln.split()
        if len(parts) == 6 and parts[0].startswith("v_"):
            try:
                costs[parts[0]] = float(parts[5])
            except ValueError:
                pass
    return costs


def ceiling(ph, costs):
    mix = MIX[ph]
    missing = sorted(k for k in mix if k not in costs)
    if missing:
        return None, {"missing_issue_costs": missing}
    cyc = sum(n * costs[k] for k, n in mix.items())
    gbs = SIMDS * CLOCK_GHZ * 64 * BLOCK_BYTES[ph] / cyc
    return gbs, {"mix_per_block_per_wave": mix, "cycles_per_block_per_wave": round(cyc, 1), "ceiling_GBs": round(gbs, 1),
                 "formula": "simds * clock_GHz * 64 lanes * block_bytes / cycles_per_block"}


def stream_legs(args):
    import ctypes as C

    import numpy as np
    import torch

    from benchlib.hostfed import measure_h2d_GBs
    from fips204_amd import _ph_lib
    from fips204_amd.ml_dsa import MODE_PREHASH, MlDsa, hash_message

    m = MlDsa(65)
    lib = _ph_lib.load()
    n, nk = args.n, 64
    phs = args.phs.split(",")
    legs = args.legs.split(",")
    xi = np.frombuffer(b"".join(bytes([i]) * 32 for i in range(nk)), dtype=np.uint8)
    pk, sk = m.keygen_host(xi)
    kidx = (np.arange(n) % nk).astype(np.uint32)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps  # ms

    def wall(fn, steps):
        fn()
        best = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            best.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(best))

    def pinned(nbytes):
        p = C.c_void_p()
        assert m.lib.mldsa_host_alloc(C.byref(p), max(nbytes, 1)) == 0
        return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]

    if "prehash_stream" in legs:
        for L in [int(x) for x in args.lens.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(L)
            buf = torch.randint(0, 256, (n * L + 16,), dtype=torch.uint8, device="cuda", generator=g)
            off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
            q = L // 4
            # 4 equal pieces: piece u of every op packed back to back, as a caller who receives the batch in four parts holds it
            view = buf[:n * L].view(n, L)
            parts = [view[:, u * q:(u + 1) * q].contiguous().view(-1) for u in range(4)]
            parts = [torch.cat([x, torch.zeros(16, dtype=torch.uint8, device="cuda")]) for x in parts]
            off4 = torch.arange(n + 1, dtype=torch.int64, device="cuda") * q
            for ph in phs:
                one_ms = timed(lambda: m.prehash_device(buf, off, n, ph), args.steps, args.warmup)

                def run(pieces):
                    st = m.prehash_stream(n, ph)
                    for b_, o_ in pieces:
                        st.update(b_, o_)
                    return st.final()
                s1_ms = timed(lambda: run([(buf, off)]), args.steps, args.warmup)
                s4_ms = timed(lambda: run([(x, off4) for x in parts]), args.steps, args.warmup)
                assert torch.equal(run([(buf, off)])[0], m.prehash_device(buf, off, n, ph)[0])
                assert torch.equal(run([(x, off4) for x in parts])[0], m.prehash_device(buf, off, n, ph)[0])
                sb = lib.mldsa_ph_state_bytes(m._ph_arg(ph), n)
                print(json.dumps({"workload": "prehash_stream", "ph": ph, "n_ops": n, "msg_len": L, "state_bytes": sb,
                                  "one_shot_us": round(one_ms * 1e3, 1), "stream_1_piece_us": round(s1_ms * 1e3, 1),
                                  "stream_4_pieces_us": round(s4_ms * 1e3, 1), "ratio_1_piece": round(s1_ms / one_ms, 3),
                                  "ratio_4_pieces": round(s4_ms / one_ms, 3),
                                  "extra_1_piece_us": round((s1_ms - one_ms) * 1e3, 1)}), flush=True)
            del buf, parts, view
            torch.cuda.empty_cache()

    def host_batch(L):
        """n messages of L bytes in page-locked memory (handle to free, bytes) and their offsets"""
        hm, msgs = pinned(n * L)
        msgs[:] = np.random.default_rng(L).integers(0, 256, n * L, dtype=np.uint8)
        moff = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        return hm, msgs, moff

    if "hash_host" in legs:
        L = 1024
        hm, msgs, moff = host_batch(L)
        hs, sig_buf = pinned(n * m.SIG_LEN)
        ho, ok_buf = pinned(n)
        hst, st_raw = pinned(4 * n)
        st_buf = st_raw.view(np.int32)
        sig2d = sig_buf.reshape(n, m.SIG_LEN)
        rnd = np.zeros(n * 32, dtype=np.uint8)
        h2d = measure_h2d_GBs()
        raw = msgs.tobytes()
        mlist = [raw[i * L:(i + 1) * L] for i in range(n)]
        for ph in phs:
            sign_ms = wall(lambda: m.hash_sign_host(sk, (msgs, moff), rnd, ph=ph, key_idx=kidx, out=(sig2d, st_buf)), 3)
            ver_ms = wall(lambda: m.hash_verify_host(pk, (msgs, moff), sig2d, ph=ph, key_idx=kidx, out=ok_buf), 5)
            assert ok_buf.all()
            t0 = time.perf_counter()
            rows = [hash_message(x, ph) for x in mlist]
            loop_ms = (time.perf_counter() - t0) * 1e3
            rl = len(rows[0])
            hr, rflat = pinned(n * rl)
            rflat[:] = np.frombuffer(b"".join(rows), dtype=np.uint8)
            roff = np.arange(n + 1, dtype=np.uint64) * np.uint64(rl)
            vfloor_ms = wall(lambda: m.verify_host(pk, (rflat, roff), sig2d, key_idx=kidx, mode=MODE_PREHASH, out=ok_buf), 5)
            assert ok_buf.all()
            sfloor_ms = wall(lambda: m.sign_host(sk, (rflat, roff), rnd, key_idx=kidx, mode=MODE_PREHASH, out=(sig2d, st_buf)), 3)
            m.lib.mldsa_host_free(hr)
            up_ms = n * L / (h2d * 1e9) * 1e3
            print(json.dumps({"workload": "hash_host", "set": 65, "ph": ph, "n_ops": n, "msg_len": L, "memory": "page-locked",
                              "hash_verify_host_ms": round(ver_ms, 3), "hash_sign_host_ms": round(sign_ms, 3),
                              "host_prehash_loop_ms": round(loop_ms, 1),
                              "parent_route_verify_ms": round(loop_ms + vfloor_ms, 1), "parent_route_sign_ms": round(loop_ms + sfloor_ms, 1),
                              "verify_host_on_rows_ms": round(vfloor_ms, 3), "sign_host_on_rows_ms": round(sfloor_ms, 3),
                              "h2d_GBs_measured": round(h2d, 2), "message_upload_ms": round(up_ms, 3),
                              "verify_over_floor": round(ver_ms / (vfloor_ms + up_ms), 3),
                              "sign_over_floor": round(sign_ms / (sfloor_ms + up_ms), 3),
                              "verify_speedup_vs_parent_route": round((loop_ms + vfloor_ms) / ver_ms, 1),
                              "sign_speedup_vs_parent_route": round((loop_ms + sfloor_ms) / sign_ms, 1)}), flush=True)
        for h_ in (hm, hs, ho, hst):
            m.lib.mldsa_host_free(h_)

    if "staging_sweep" in legs:
        L = args.sweep_len
        hm, msgs, moff = host_batch(L)
        hs, sig_buf = pinned(n * m.SIG_LEN)
        sig2d = sig_buf.reshape(n, m.SIG_LEN)
        st_buf = np.zeros(n, dtype=np.int32)
        rnd = np.zeros(n * 32, dtype=np.uint8)
        h2d = measure_h2d_GBs()
        for ph in phs:
            m.hash_sign_host(sk, (msgs, moff), rnd, ph=ph, key_idx=kidx, out=(sig2d, st_buf))
            for mib in [int(x) for x in args.sweep_mib.split(",")]:
                ok = np.zeros(n, dtype=np.uint8)
                ms = wall(lambda: m.hash_verify_host(pk, (msgs, moff), sig2d, ph=ph, key_idx=kidx, out=ok, staging_bytes=mib << 20), 3)
                assert ok.all()
                print(json.dumps({"workload": "staging_sweep", "set": 65, "ph": ph, "n_ops": n, "msg_len": L, "memory": "page-locked",
                                  "staging_MiB": mib, "hash_verify_host_ms": round(ms, 2), "message_GBs": round(n * L / ms / 1e6, 2),
                                  "h2d_GBs_measured": round(h2d, 2)}), flush=True)
        m.lib.mldsa_host_free(hm)
        m.lib.mldsa_host_free(hs)


def small_legs(args):
    """small-call latency: the host clock around one call that ends in a synchronise"""
    import numpy as np
    import torch

    from fips204_amd.ml_dsa import MlDsa

    m = MlDsa(65)
    nk = 16
    pk, sk = m.keygen_from_seed([bytes([i]) * 32 for i in range(nk)])
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)

    def latency(fn):
        for _ in range(args.warmup_calls):
            fn()
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        q = np.percentile(t, [50, 10, 25, 75, 90])
        return {"median_us": round(float(q[0]), 1), "p10_us": round(float(q[1]), 1), "p25_us": round(float(q[2]), 1),
                "p75_us": round(float(q[3]), 1), "p90_us": round(float(q[4]), 1), "min_us": round(float(min(t)), 1),
                "max_us": round(float(max(t)), 1)}

    for ph in args.phs.split(","):
        for L in [int(x) for x in args.lens.split(",")]:
            for n in [int(x) for x in args.ns.split(",")]:
                g = torch.Generator(device="cuda").manual_seed(L)
                buf = torch.randint(0, 256, (n * L + 16,), dtype=torch.uint8, device="cuda", generator=g)
                off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
                kidx = torch.from_numpy((np.arange(n) % nk).astype(np.int32)).cuda()
                rnd = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
                sigs = torch.empty((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
                ok = torch.empty(n, dtype=torch.uint8, device="cuda")
                m.hash_sign_device(sks, buf, off, rnd, sigs, n, ph, key_idx=kidx)

                def call_prehash():
                    m.prehash_device(buf, off, n, ph)
                    torch.cuda.synchronize()

                def call_verify():
                    m.hash_verify_device(pks, buf, off, sigs, ok, n, ph, key_idx=kidx)
                    torch.cuda.synchronize()

                rec = {"workload": "prehash_small_call", "label": args.label, "set": 65, "ph": ph, "n_ops": n, "msg_len": L,
                       "calls": args.calls, "clock": "host perf_counter around call + synchronise",
                       "prehash": latency(call_prehash), "hash_verify_device": latency(call_verify)}
                assert bool(ok.all())
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--lens", default="64,1024,16384")
    ap.add_argument("--phs", default="SHA256,SHA512,SHAKE128")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big", type=int, default=262144, help="also the 1 KiB point at this many ops (0: skip)")
    ap.add_argument("--ubench", default=os.path.join(ROOT, "profiles", "prehash_ubench_valu.txt"))
    ap.add_argument("--no-host", action="store_true", help="skip the host pre-hash calls")
    ap.add_argument("--stream", action="store_true", help="the legs of the incremental pre-hash and the host-memory calls instead")
    ap.add_argument("--legs", default="prehash_stream,hash_host,staging_sweep")
    ap.add_argument("--sweep-len", type=int, default=16384)
    ap.add_argument("--sweep-mib", default="1,4,16,64")
    ap.add_argument("--lib", default="", help="measure this build of libmldsa_ph.so instead of the tree's")
    ap.add_argument("--label", default="", help="copied into every JSON line")
    ap.add_argument("--ops-lens", default="", help="message lengths at which the op-level and pure-mode calls are measured too (default: all)")
    ap.add_argument("--small", action="store_true", help="small-call latency of mldsa_prehash and hash_verify_device instead")
    ap.add_argument("--ns", default="1,8,64,256,1024,4096", help="--small: operations per call")
    ap.add_argument("--calls", type=int, default=200, help="--small: timed calls per point")
    ap.add_argument("--warmup-calls", type=int, default=20)
    args = ap.parse_args()
    if args.lib:
        from fips204_amd import _ph_lib
        _ph_lib.LIB_PATH = os.path.abspath(args.lib)
    if args.stream:
        return stream_legs(args)
    if args.small:
        return small_legs(args)

    import numpy as np
    import torch

    from fips204_amd.ml_dsa import MODE_PREHASH, MlDsa, hash_message

    costs = issue_costs(args.ubench) if os.path.exists(args.ubench) else {}
    m = MlDsa(65)
    nk = 64
    pk, sk = m.keygen_from_seed([bytes([i]) * 32 for i in range(nk)])
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps  # ms

    ops_lens = [int(x) for x in args.ops_lens.split(",")] if args.ops_lens else None
    points = [(n_, L, ph) for L in [int(x) for x in args.lens.split(",")] for ph in args.phs.split(",") for n_ in [args.n]]
    if args.big:
        points += [(args.big, 1024, ph) for ph in args.phs.split(",")]
    for n, L, ph in points:
        g = torch.Generator(device="cuda").manual_seed(L)
        buf = torch.randint(0, 256, (n * L + 16,), dtype=torch.uint8, device="cuda", generator=g)
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * L
        kidx = torch.from_numpy((np.arange(n) % nk).astype(np.int32)).cuda()
        rnd = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        sigs = torch.empty((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
        ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        ph_ms = timed(lambda: m.prehash_device(buf, off, n, ph), args.steps, args.warmup)
        gbs = n * L / (ph_ms * 1e-3) / 1e9
        ceil_gbs, ceil = ceiling(ph, costs) if costs else (None, {"missing_issue_costs": "no ubench file"})
        if ops_lens is not None and L not in ops_lens:
            print(json.dumps({"workload": "prehash", "label": args.label, "set": 65, "ph": ph, "n_ops": n, "msg_len": L,
                              "prehash_us": round(ph_ms * 1e3, 1), "prehash_GBs": round(gbs, 1),
                              "prehash_fraction_of_ceiling": round(gbs / ceil_gbs, 3) if ceil_gbs else None, "ceiling": ceil}), flush=True)
            del buf, sigs
            torch.cuda.empty_cache()
            continue
        hs_ms = timed(lambda: m.hash_sign_device(sks, buf, off, rnd, sigs, n, ph, key_idx=kidx, status=st), max(2, args.steps // 3), 1)
        assert int(st.min()) == 0
        hv_ms = timed(lambda: m.hash_verify_device(pks, buf, off, sigs, ok, n, ph, key_idx=kidx), args.steps, args.warmup)
        assert bool(ok.all())
        pv_ms = timed(lambda: m.verify_device(pks, buf, off, sigs, ok, n, key_idx=kidx), args.steps, args.warmup)
        ps_ms = timed(lambda: m.sign_device(sks, buf, off, rnd, sigs, n, key_idx=kidx, status=st), max(2, args.steps // 3), 1)
        rec = {"workload": "prehash", "label": args.label, "set": 65, "ph": ph, "n_ops": n, "msg_len": L,
               "prehash_us": round(ph_ms * 1e3, 1), "prehash_GBs": round(gbs, 1),
               "prehash_fraction_of_ceiling": round(gbs / ceil_gbs, 3) if ceil_gbs else None,
               "hash_verify_device_ms": round(hv_ms, 3), "hash_sign_device_ms": round(hs_ms, 3),
               "pure_verify_device_ms": round(pv_ms, 3), "pure_sign_device_ms": round(ps_ms, 3), "ceiling": ceil}
        if not args.no_host and n == args.n:
            raw = buf[:n * L].cpu().numpy().tobytes()
            msgs = [raw[i * L:(i + 1) * L] for i in range(n)]
            kh = np.arange(n, dtype=np.uint32) % nk
            sig_t = sigs.clone()
            t0 = time.perf_counter()
            m.verify(pks, [hash_message(x, ph) for x in msgs], sig_t, key_idx=kh, mode=MODE_PREHASH)
            rec["hash_verify_host_prehash_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            m.try_sign_with_seed(sks, [hash_message(x, ph) for x in msgs], rnd, key_idx=kh, mode=MODE_PREHASH)
            rec["hash_sign_host_prehash_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            [hash_message(x, ph) for x in msgs]
            rec["host_prehash_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            del msgs, raw
        print(json.dumps(rec), flush=True)
        del buf, sigs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
