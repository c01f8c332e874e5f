"""Signing ops whose rejection loop (FIPS 204 Algorithm 7, ml_dsa.rs:212-330) runs LONGER than the rounds a call plans, and the
oracle's word on them.  Shared by test_long_tail_cases_cpu.py (the inputs do what they claim, on the oracle alone) and
test_gpu_sign_long_tail.py (every entry point handles the op the plan leaves over, byte for byte).  No GPU import; everything is
derived from the seeds below, tests/golden/long_tail_ops.json only spares the GPU tests the 16 384-op trace
(`python tests/long_tail_cases.py` writes it again, ~15 s on 16 threads).

The signer plans its rounds a priori (plan_sign_compute, csrc/pipeline.hip) and stops where the EXPECTED number of unfinished ops
falls under a threshold; the attempt count of an op is a deterministic function of (key, message, ctx, rnd), and the oracle
reports it.  So "left over by the plan" is arithmetic: with MLDSA_OPT_SPEC_MAX = 1 every round tests ONE candidate per op, and with
MLDSA_OPT_SIGN_ROUNDS = r the plan has (at most) r rounds -- an op is left over exactly when its iteration count exceeds r.  At
default options a call of one op gets at most MLDSA_OPT_SPEC_MAX = 32 candidates in its first round, so the ops of the batch with
more than 32 iterations are the ones a one-op call cannot finish in it.

Batch (per parameter set): N_BATCH ops under one honest key, pure mode, empty ctx

    xi        = SHAKE256(b"tail-key-<set>" || le64(0))[:32]
    message i = SHAKE256(b"tail-<set>-msg" || le64(i))[:32]
    rnd i     = SHAKE256(b"tail-<set>-rnd" || le64(i))[:32]

Forced cases (variant()): the first n ops' messages and rnd under other keys / ctxs / with empty messages; their iteration counts
change with the inputs and are taken from the oracle for exactly those inputs.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # (run as a script: `python tests/long_tail_cases.py`)
    sys.path.insert(0, _ROOT)
from oracle import oracle as orc  # noqa: E402

SETS = (44, 65, 87)
N_BATCH = 16384
THREADS = min(16, os.cpu_count() or 1)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_tail_ops.json")
SPEC_MAX_DEFAULT = 32   # MLDSA_OPT_SPEC_MAX as a context starts: the most candidates an op gets in one round
LONG = 25               # the fixture lists the ops above this many iterations
# What the inputs must give for the tests to mean anything (requirements on the inputs, not measurements): per set, at least this
# many ops with more than `threshold` iterations.
CONDITIONS = {SPEC_MAX_DEFAULT: 1, LONG: 8}
N_FORCED, NK_FORCED = 261, 6   # the forced host cases: 261 ops cut 197 + 64 on a 64-op sub-batch context, key_idx over 6 keys


def shake(tag, i, n=32):
    return hashlib.shake_256(tag + int(i).to_bytes(8, "little")).digest(n)


def xi(pset):
    return shake(b"tail-key-%d" % pset, 0)


def message(pset, i):
    return shake(b"tail-%d-msg" % pset, i)


def rnd(pset, i):
    return shake(b"tail-%d-rnd" % pset, i)


@functools.lru_cache(maxsize=None)
def key(pset):
    """the batch's key: (oracle PubKey, oracle PrivKey, wire pk bytes, wire sk bytes)"""
    pk, sk = orc.keygen_from_seed(pset, xi(pset))
    return pk, sk, orc.pk_into_bytes(pset, pk), orc.sk_into_bytes(pset, sk)


@functools.lru_cache(maxsize=None)
def traced(pset, n=N_BATCH, cap=1):
    """the oracle over the first n ops of the batch: (sigs uint8 [n, SIG_LEN], iterations int32 [n], trace [n, cap]); read-only"""
    out = orc.sign_trace_batch_mt(pset, [key(pset)[1]], np.zeros(n, dtype=np.uint32), [message(pset, i) for i in range(n)],
                                  [rnd(pset, i) for i in range(n)], THREADS, mode=0, cap=cap)
    for a in out:
        a.setflags(write=False)
    return out


def summary(iters):
    """what the fixture records of a set's iteration counts"""
    iters = np.asarray(iters)
    ops = np.nonzero(iters > LONG)[0]
    return {"n_ops": int(iters.size), "over_14": int((iters > 14).sum()), "max": int(iters.max()), "ops": [int(i) for i in ops],
            "iterations": [int(iters[i]) for i in ops]}


def compute_fixture():
    return {str(s): summary(traced(s)[1]) for s in SETS}


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def long_ops(pset, over=LONG):
    """(op indices, iteration counts) of the batch's ops with more than `over` >= LONG iterations, from the fixture"""
    assert over >= LONG
    fx = fixture()[str(pset)]
    ops, it = np.array(fx["ops"], dtype=np.int64), np.array(fx["iterations"], dtype=np.int32)
    return ops[it > over], it[it > over]


def unmet(iters):
    """the CONDITIONS a set's iteration counts miss: list of (threshold, got, need)"""
    iters = np.asarray(iters)
    return [(t, int((iters > t).sum()), need) for t, need in CONDITIONS.items() if int((iters > t).sum()) < need]


def unfinished_after(iters, rounds, per_round=1):
    """bool per op: still unsigned after `rounds` rounds of `per_round` candidates each -- the loop takes the FIRST accepted
    candidate (ml_dsa.rs:212-330), so an op is done as soon as its accepted attempt, number `iterations`, has been tested"""
    return np.asarray(iters) > rounds * per_round


@functools.lru_cache(maxsize=None)
def oracle_sig(pset, i):
    """the oracle's signature of op i of the batch and its iteration count"""
    return orc.sign_internal(pset, key(pset)[1], message(pset, i), rnd(pset, i), ctx=b"", mode=0, want_iters=True)


def padded(pset, n=64, over=LONG):
    """n distinct ops of the batch, ascending: the ops above `over` (those with the most iterations if there are more than n),
    padded with the ops that follow each of them"""
    ops, it = long_ops(pset, over)
    ops = [int(i) for i in ops[np.argsort(-it, kind="stable")[:n]]]
    chosen, step = set(ops), 1
    while len(chosen) < n:
        for i in ops:
            if len(chosen) < n:
                chosen.add((i + step) % N_BATCH)
        step += 1
    return np.array(sorted(chosen), dtype=np.int64)


# ------------------------------------------------------------------------------ the forced cases' inputs
def op_key_seed(pset, i):
    return shake(b"tail-%d-opkey" % pset, i)


@functools.lru_cache(maxsize=None)
def op_keys(pset, n):
    """n further honest keys (one per op of a call without key_idx; the first NK_FORCED serve the key_idx cases):
    (wire pk [n, PK_LEN], wire sk [n, SK_LEN])"""
    pk, sk = orc.keygen_batch_mt(pset, [op_key_seed(pset, i) for i in range(n)], THREADS)
    for a in (pk, sk):
        a.setflags(write=False)
    return pk, sk


@functools.lru_cache(maxsize=None)
def variant(pset, n, with_kidx, with_ctx, empty_msgs, mode=0, ph=None):
    """Inputs of a forced host call and the oracle on them: dict(sk [n_keys, SK_LEN], kidx uint32 [n] or None, msgs, ctxs (list or
    None), rnd, sig uint8 [n, SIG_LEN], iters int32 [n]).  ph: the HashML-DSA signature (pre-hash `ph`) of the same inputs."""
    nk = NK_FORCED if with_kidx else n
    sk = op_keys(pset, n)[1][:nk]
    kidx = np.array([shake(b"tail-%d-kidx" % pset, i, 1)[0] % nk for i in range(n)], dtype=np.uint32) if with_kidx else None
    msgs = [b"" if empty_msgs else message(pset, i) for i in range(n)]
    ctxs = [shake(b"tail-%d-ctx" % pset, i, i % 9) for i in range(n)] if with_ctx else None
    rn = [rnd(pset, i) for i in range(n)]
    sk_o = [orc.sk_try_from_bytes(pset, sk[j].tobytes()) for j in range(nk)]
    sig, iters = np.zeros((n, orc.params(pset).sig_len), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    for i in range(n):
        k, c = sk_o[int(kidx[i]) if with_kidx else i], ctxs[i] if with_ctx else b""
        if ph is not None:
            oid, phm = orc.hash_message(msgs[i], ph)
            s, it = orc.sign_internal(pset, k, oid + phm, rn[i], ctx=c, mode=orc.MODE_PREHASH, want_iters=True)
        else:
            s, it = orc.sign_internal(pset, k, msgs[i], rn[i], ctx=c, mode=mode, want_iters=True)
        sig[i], iters[i] = np.frombuffer(s, dtype=np.uint8), it
    for a in (sig, iters):
        a.setflags(write=False)
    return dict(sk=sk, kidx=kidx, msgs=msgs, ctxs=ctxs, rnd=rn, sig=sig, iters=iters)


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(compute_fixture(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(FIXTURE, {s: (len(v["ops"]), v["max"]) for s, v in fixture().items()})
