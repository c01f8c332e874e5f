"""Inputs of the incremental-mu tests (mldsa_mus_init / _update / _final): operations (ctx, message), the ways the messages are cut into
pieces, and the conditions those inputs must meet.  Pure numpy / hashlib: test_mu_stream_cpu.py checks the generator here,
test_gpu_mu_stream.py feeds the same schedules to the device.

R = 136 is SHAKE256's rate; the sponge has absorbed P bytes before the message: P = 64 (tr; MODE_INTERNAL) or 66 + len(ctx)
(tr | domain | len(ctx) | ctx; MODE_PURE, MODE_PREHASH).  A schedule is (ops, cuts) as in ph_stream_cases: `ops` the indices of the
operations that take part, `cuts[j]` the cut positions of message ops[j], 0 = c_0 <= c_1 <= ... <= c_U = len -- update u absorbs
msg[c_u : c_{u + 1}]; every op of a schedule has U pieces."""
import hashlib

import numpy as np

import piece_schedules
from piece_schedules import gather_pieces, random_cuts  # noqa: F401

MODE_PURE, MODE_INTERNAL, MODE_PREHASH = 0, 1, 2
MODES = (MODE_PURE, MODE_INTERNAL, MODE_PREHASH)
R = 136
# 69: P = 135 (one byte short of a block); 70: P = one block exactly; 71: P = R + 1; 206: P = two blocks
CTX_LENS = (0, 1, 5, 69, 70, 71, 205, 206, 255)
BIG = 300 << 10
# HOST_LENS of test_gpu_prehash_stream.py / test_gpu_prehash_fips_list.py
HOST_LENS = (0, 1, 63, 64, 65, 167, 168, 4095, 4096, 4097, 5000, 12289, 200 << 10, 3, 9000, 128, 100, 2, 70000, 31, 8192, 777, 1, 0)


def prefix_len(mode, ctx):
    return 64 if mode == MODE_INTERNAL else 66 + len(ctx)


def m_prime_prefix(mode, ctx):
    return b"" if mode == MODE_INTERNAL else bytes([1 if mode == MODE_PREHASH else 0, len(ctx)]) + ctx


def _at(P, k, d):
    """the smallest x >= k R with P + x = d (mod R)"""
    return (d - P) % R + k * R


def cases(mode):
    """[(ctx, msg)]: for each ctx length the nine message lengths with P + len = k R + d (mod R, k in 0..2, d in -1, 0, 1) and the empty
    message; 60 seeded lengths below 1000; two messages of 300 KiB among short ones.  MODE_INTERNAL has no ctx: ctx length 0 only."""
    rng = np.random.default_rng(204 + mode)
    ctx_lens = (0,) if mode == MODE_INTERNAL else CTX_LENS
    shape = []
    for cl in ctx_lens:
        P = 64 if mode == MODE_INTERNAL else 66 + cl
        shape += [(cl, _at(P, k, d)) for k in (0, 1, 2) for d in (-1, 0, 1)] + [(cl, 0)]
    shape += [(int(ctx_lens[int(rng.integers(0, len(ctx_lens)))]), int(n)) for n in rng.integers(0, 1000, 60)]
    shape += [(0, BIG), (ctx_lens[-1], 5), (ctx_lens[1 % len(ctx_lens)], BIG), (0, 0)]
    return [(rng.integers(0, 256, cl, dtype=np.uint8).tobytes(), rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for cl, n in shape]


def schedules(ops_, mode):
    """name -> (ops, cuts): (a) one piece, (b) a cut where P + cut = k R + d, k in 0..3, d in -1, 0, 1 (at the message's end if it is
    shorter), (c) 1-byte pieces for the messages of <= 300 bytes, (d) three seeded 9-update schedules with two empty pieces each and an
    empty last update on every third op"""
    n = len(ops_)
    every = list(range(n))
    P = [prefix_len(mode, c) for c, _ in ops_]
    L = [len(m) for _, m in ops_]
    out = {"one_piece": (every, [[0, L[i]] for i in every])}
    for k in (0, 1, 2, 3):
        for d in (-1, 0, 1):
            out[f"cut_{k}R{d:+d}"] = (every, [[0, min(_at(P[i], k, d), L[i]), L[i]] for i in every])
    small = [i for i in every if L[i] <= 300]
    out["bytes"] = (small, [list(range(L[i] + 1)) + [L[i]] * (300 - L[i]) for i in small])
    for seed in (1, 2, 3):
        rng = np.random.default_rng(2000 + 10 * mode + seed)
        U = 9
        cuts = []
        for j in every:
            inner = sorted(int(x) for x in rng.integers(0, L[j] + 1, U - 1))
            for u in rng.choice(U - 1, 2, replace=False):  # two empty pieces somewhere in the middle
                inner[u] = inner[u - 1] if u else 0
            inner.sort()
            if j % 3 == 0:
                inner[-1] = L[j]                            # the last update is empty
            cuts.append([0] + inner + [L[j]])
        out[f"random_{seed}"] = (every, cuts)
    return out


def coverage(ops_, sched, mode):
    """what the operations and schedules exercise: the conditions the tests assert before anything runs"""
    c = dict(fill_135_nonempty=0, completes_exactly=0, completes_then_2_blocks=0, empty_piece=0, one_byte=0, final_update_empty=0,
             pad_in_one_byte=0, pad_only_block=0)
    if mode != MODE_INTERNAL:
        c.update(prefix_on_boundary_empty_message=0, prefix_fill_135=0)
    for ctx, msg in ops_:
        P = prefix_len(mode, ctx)
        c["pad_in_one_byte"] += (P + len(msg)) % R == R - 1   # 0x1F and 0x80 land in one byte
        c["pad_only_block"] += (P + len(msg)) % R == 0
        if mode != MODE_INTERNAL:
            c["prefix_on_boundary_empty_message"] += P % R == 0 and len(msg) == 0
            c["prefix_fill_135"] += P % R == R - 1
    for ops, cuts in sched.values():
        for i, cs in zip(ops, cuts):
            P, L = prefix_len(mode, ops_[i][0]), len(ops_[i][1])
            assert cs[0] == 0 and cs[-1] == L and all(a <= b for a, b in zip(cs, cs[1:])), (i, cs[:4])
            for u in range(len(cs) - 1):
                fill, plen = (P + cs[u]) % R, cs[u + 1] - cs[u]
                c["fill_135_nonempty"] += fill == R - 1 and plen > 0
                c["completes_exactly"] += fill > 0 and fill + plen == R
                c["completes_then_2_blocks"] += fill > 0 and plen >= (R - fill) + 2 * R
                c["empty_piece"] += plen == 0
                c["one_byte"] += plen == 1
            c["final_update_empty"] += len(cs) > 2 and cs[-1] == cs[-2] and cs[-1] > 0
    return c


def pieces_of(ops_, ops, cuts, u):
    """update u of a schedule as byte strings, one per op of the schedule"""
    return piece_schedules.pieces_of([msg for _, msg in ops_], ops, cuts, u)


def hashlib_incremental(ops_, trs, mode, ops, cuts, upto=None):
    """hashlib.shake_256 fed tr, the prefix and the same pieces (the first `upto` updates): the mu rows the device must reach"""
    out = []
    for i, cs in zip(ops, cuts):
        ctx, msg = ops_[i]
        h = hashlib.shake_256()
        h.update(trs[i])
        h.update(m_prime_prefix(mode, ctx))
        for u in range(len(cs) - 1 if upto is None else upto):
            h.update(msg[cs[u]:cs[u + 1]])
        out.append(h.digest(64))
    return out


def pack_at(pieces, shift):
    """(flat uint8, uint64 offsets[n + 1]): the pieces back to back, the first at byte `shift` of the buffer -- every alignment occurs"""
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    off += np.uint64(shift)
    return np.frombuffer(bytes(shift) + b"".join(pieces) + bytes(8), dtype=np.uint8), off
