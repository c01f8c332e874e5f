#!/usr/bin/env python3
"""Incremental mu on the device and mu from host memory (include/mldsa_mus.h): one JSON line per case.

Every case alternates its variants in one process on the same device arrays after warm-up, --steps samples per variant, median and
p10 / p90.  Device calls are timed by a hipEvent pair on the calls' stream, the blocking host-memory calls by a host clock around the
call (they return when mu is complete).  The results of the variants of a case are compared before its line is written.

  stream      mldsa_mus_init + K x mldsa_mus_update + mldsa_mus_final (K = 1 and 8 pieces per message)  against  mldsa_mu_compute on
              the whole messages (the reference route: it needs every message whole in device memory)
  host        mldsa_mus_host_compute on messages in pageable host memory                                against  upload of the whole batch
              + mldsa_mu_compute
  forms       (--forms-dir DIR) the two kernel forms against each other, to place MLDSA_MUS_WAVE_MAX_OPS: the layer is built twice in a
              shadow of the tree under DIR, with -DMLDSA_MUS_WAVE_MAX_OPS=0 (one op per lane always) and =1000000 (one op per wave
              always, at these sizes), and init + update + final is timed at n in 1, 64, 1024, 4096, 16384 for 1 KiB and 16 KiB
              messages.  The macro is the largest measured n at which the wave form's median is below the lane form's by more than the
              lane form's p10 to p90 spread at both message sizes; the last line of the run says which n that is.

    python tools/bench_mus.py                       # writes profiles/mu_stream_bench.jsonl and prints the lines
    python tools/bench_mus.py --forms-dir /tmp/f    # appends the forms lines as well
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FORMS = {"lane": 0, "wave": 1000000}
FORM_NS = (1, 64, 1024, 4096, 16384)
FORM_SIZES = (1024, 16384)


def build_form(forms_dir, name, value):
    """libmldsa_mus.so with MLDSA_MUS_WAVE_MAX_OPS = value, built in a shadow of the tree (sources copied, the core's directory, layer/
    and include/ linked) unless it is there already; the links are made again where a copy of the shadow came without them"""
    from fips204_amd import build
    pkg = os.path.join(forms_dir, name, "fips204_amd")
    shadow = os.path.join(pkg, "mus")
    os.makedirs(shadow, exist_ok=True)
    for link, target in ((os.path.join(pkg, "csrc"), build.CSRC), (os.path.join(pkg, "layer"), os.path.join(build._HERE, "layer")),
                         (os.path.join(forms_dir, name, "include"), os.path.join(ROOT, "include"))):
        if not os.path.exists(link):
            if os.path.islink(link):
                os.unlink(link)
            os.symlink(target, link)
    so = os.path.join(shadow, "libmldsa_mus.so")
    if not os.path.exists(so):
        for f in ("Makefile", "mus.hip"):
            shutil.copy(os.path.join(build.MUS_DIR, f), os.path.join(shadow, f))
        flags = f"-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DMLDSA_MUS_WAVE_MAX_OPS={value}"
        subprocess.run(["make", "-C", shadow, f"CXXFLAGS={flags}"], check=True, capture_output=True)
    return so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed samples per variant and case (at least 20)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds per case")
    ap.add_argument("--forms-dir", default="", help="build and measure the two kernel forms in a shadow of the tree under this directory")
    ap.add_argument("--build-forms-only", action="store_true", help="with --forms-dir: build the two forms and stop (needs no GPU)")
    ap.add_argument("--only", default="", help="comma separated workloads to run: stream, host, forms (default: all that apply)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mu_stream_bench.jsonl"))
    ap.add_argument("--label", default="", help="copied into every JSON line")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20")
    form_libs = {name: build_form(args.forms_dir, name, v) for name, v in FORMS.items()} if args.forms_dir else {}
    if args.build_forms_only:
        print(json.dumps(form_libs))
        return

    import numpy as np
    import torch

    from fips204_amd import _mus_lib
    from fips204_amd.hotpath import _ptr, _stream
    from fips204_amd.ml_dsa import MODE_PURE, MlDsa

    assert torch.cuda.is_available(), "bench_mus.py measures on the GPU; there is no other path"
    want = set(args.only.split(",")) if args.only else {"stream", "host", "forms"}
    m = MlDsa(44)
    dev_name = torch.cuda.get_device_name(0)
    n_keys = 64
    pk, _ = m.keygen_from_seed([i.to_bytes(4, "little") * 8 for i in range(n_keys)])
    tr = m.public_keys_from_bytes(pk).tr.clone()

    def stats(ms):
        q = np.percentile(ms, [50, 10, 90])
        return {"median_ms": round(float(q[0]), 4), "p10_ms": round(float(q[1]), 4), "p90_ms": round(float(q[2]), 4)}

    def timed(run, on_host=()):
        times = {v: [] for v in run}
        for r in range(args.warmup + args.steps):
            for v, fn in run.items():  # alternating: every round takes one sample of every variant
                if v in on_host:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1)
                if r >= args.warmup:
                    times[v].append(ms)
        torch.cuda.synchronize()
        return {v: stats(t) for v, t in times.items()}

    def batch(n, size, seed):
        rng = np.random.default_rng(seed)
        buf = torch.from_numpy(rng.integers(0, 256, n * size, dtype=np.uint8)).cuda()
        off = torch.arange(0, size * (n + 1), size, dtype=torch.int64, device="cuda")
        kidx = torch.from_numpy((np.arange(n) * 2654435761 % n_keys).astype(np.uint32).view(np.int32)).cuda()
        return buf, off, kidx

    def streamer(lib, n, buf, offs, kidx):
        """init + one update per offset table + final through `lib`, into buffers allocated once: (call, mu, flag)"""
        sb = lib.mldsa_mus_state_bytes(n)
        state = torch.empty(sb, dtype=torch.uint8, device="cuda")
        mu = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        flag = torch.zeros(n, dtype=torch.int32, device="cuda")

        def call():
            s = _stream(m.device)
            rc = lib.mldsa_mus_init(m.hp._h, MODE_PURE, _ptr(tr), n_keys, _ptr(kidx), None, None, _ptr(state), sb, n, s)
            for o in offs:
                rc = rc or lib.mldsa_mus_update(m.hp._h, _ptr(state), sb, _ptr(buf), _ptr(o), n, s)
            rc = rc or lib.mldsa_mus_final(m.hp._h, _ptr(state), sb, _ptr(mu), _ptr(flag), n, s)
            assert rc == 0, lib.mldsa_mus_last_error()
        return call, mu, flag

    lines = []

    def emit(rec, st):
        rec.update({"label": args.label, "steps": args.steps, "warmup": args.warmup, "device": dev_name})
        rec.update(st)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    lib = _mus_lib.load()
    if "stream" in want:
        for n, size in ((1, 1024), (1, 1 << 20), (64, 16384), (4096, 1024), (65536, 1024), (16384, 16384)):
            buf, off, kidx = batch(n, size, 7 * n + size)
            one, mu1, fl1 = streamer(lib, n, buf, [off], kidx)
            run = {"stream_1_piece": one, "mu_compute": lambda: m.mu_device(tr, buf, off, n, key_idx=kidx)}
            if n == 1:  # the one message in eight updates, where it lies: update p names the p-th eighth of the buffer
                tabs = [torch.tensor([p * (size // 8), (p + 1) * (size // 8)], dtype=torch.int64, device="cuda") for p in range(8)]
                eight, mu8, fl8 = streamer(lib, n, buf, tabs, kidx)
                run["stream_8_pieces"] = eight
            st = timed(run)
            ref, _ = m.mu_device(tr, buf, off, n, key_idx=kidx)
            assert torch.equal(mu1, ref) and not bool(fl1.any()), "streamed mu and mldsa_mu_compute disagree"
            if n == 1:
                assert torch.equal(mu8, ref)
            rec = {"workload": "mu_stream", "n_ops": n, "msg_bytes": size, "wave_max_ops": _mus_lib.wave_max_ops(),
                   "clock": "hipEvent pair on the stream around init + update(s) + final / around mldsa_mu_compute",
                   "stream_over_compute_time": round(st["stream_1_piece"]["median_ms"] / st["mu_compute"]["median_ms"], 3),
                   "stream_GBs": round(n * size / st["stream_1_piece"]["median_ms"] / 1e6, 2)}
            emit(rec, st)
            del buf, off, kidx, one, run
            torch.cuda.empty_cache()
    if "host" in want:
        for n, size, staging in ((4096, 16384, 0), (4096, 16384, 1 << 20), (1, 8 << 20, 0), (1, 8 << 20, 1 << 20)):
            rng = np.random.default_rng(n + size)
            flat = rng.integers(0, 256, n * size, dtype=np.uint8)
            hoff = np.arange(0, size * (n + 1), size, dtype=np.uint64)
            kidx_h = (np.arange(n) * 2654435761 % n_keys).astype(np.uint32)
            kidx = torch.from_numpy(kidx_h.view(np.int32)).cuda()
            doff = torch.from_numpy(hoff.view(np.int64)).cuda()
            out = {}

            def hosted():
                out["host"] = m.mu_host(tr, (flat, hoff), None, kidx, MODE_PURE, staging)[0]

            def uploaded():
                out["upload"] = m.mu_device(tr, torch.from_numpy(flat).cuda(), doff, n, key_idx=kidx)[0]

            st = timed({"mu_host": hosted, "upload_mu_compute": uploaded}, on_host=("mu_host", "upload_mu_compute"))
            assert torch.equal(out["host"], out["upload"]), "mu_host and mldsa_mu_compute disagree"
            emit({"workload": "mu_host", "n_ops": n, "msg_bytes": size, "staging_bytes": staging or "default", "memory": "pageable",
                  "clock": "host clock around the blocking call, device synchronised before and after",
                  "device_bytes_for_messages": 2 * (staging or 64 << 20), "device_bytes_for_messages_upload_route": n * size,
                  "host_over_upload_time": round(st["mu_host"]["median_ms"] / st["upload_mu_compute"]["median_ms"], 3),
                  "mu_host_GBs": round(n * size / st["mu_host"]["median_ms"] / 1e6, 2)}, st)
    if "forms" in want and form_libs:
        libs = {}
        for name, path in form_libs.items():
            libs[name] = C.CDLL(path)
            for fn, argtypes in _mus_lib._SIGNATURES.items():
                getattr(libs[name], fn).argtypes = argtypes
                getattr(libs[name], fn).restype = _mus_lib._RESTYPES.get(fn, C.c_int)
        wins = {}
        for size in FORM_SIZES:
            for n in FORM_NS:
                buf, off, kidx = batch(n, size, 13 * n + size)
                calls = {name: streamer(libs[name], n, buf, [off], kidx) for name in libs}
                st = timed({name: c[0] for name, c in calls.items()})
                assert torch.equal(calls["lane"][1], calls["wave"][1]), "the two kernel forms disagree"
                spread = st["lane"]["p90_ms"] - st["lane"]["p10_ms"]
                win = st["wave"]["median_ms"] < st["lane"]["median_ms"] - spread
                wins.setdefault(n, []).append(win)
                emit({"workload": "mu_stream_forms", "n_ops": n, "msg_bytes": size, "clock": "hipEvent pair on the stream around init + update + final",
                      "lane_p10_p90_spread_ms": round(spread, 4), "wave_wins_by_more_than_the_spread": bool(win)}, st)
                del buf, off, kidx, calls
                torch.cuda.empty_cache()
        both = [n for n in FORM_NS if all(wins[n])]
        emit({"workload": "mu_stream_forms_verdict", "rule": "largest measured n at which the wave form's median is below the lane form's by more "
              "than the lane form's p10-p90 spread, at 1 KiB and at 16 KiB", "wave_wins_at": both, "MLDSA_MUS_WAVE_MAX_OPS": max(both) if both else 0,
              "header_has": _mus_lib.wave_max_ops()}, {})
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    m.hp.close()


if __name__ == "__main__":
    main()
