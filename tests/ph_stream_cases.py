"""Inputs of the incremental pre-hash tests (mldsa_ph_init / _update / _final): messages, the ways they are cut into
pieces, and the conditions those inputs must meet.  Pure numpy / hashlib: test_prehash_stream_cpu.py checks the generator
here, test_gpu_prehash_stream.py feeds the same schedules to the device.

A schedule is (ops, cuts): `ops` the indices of the messages that take part, `cuts[j]` the cut positions of message
ops[j], 0 = c_0 <= c_1 <= ... <= c_U = len -- update u absorbs msg[c_u : c_{u + 1}]; every op of a schedule has U pieces."""
import hashlib

import numpy as np

from piece_schedules import gather_pieces, pieces_of, random_cuts  # noqa: F401

PHS = ("SHA256", "SHA512", "SHAKE128")
BLOCK = {"SHA256": 64, "SHA512": 128, "SHAKE128": 168}
EDGES = {"SHA256": (0, 1, 55, 56, 63, 64, 65, 119, 120), "SHA512": (111, 112, 127, 128, 239, 240), "SHAKE128": (167, 168, 169, 335, 336)}


def seam_messages():
    """the messages of test_prehash_seam_matches_hashlib: every padding edge of the three PH, 200 random lengths < 3000, two 4 MiB
    messages among short ones"""
    rng = np.random.default_rng(7)
    lens = [n for p in PHS for n in EDGES[p]]
    lens += list(rng.integers(0, 3000, 200)) + [4 << 20, 5, 4 << 20, 0]
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


def schedules(msgs, ph):
    """name -> (ops, cuts) for the block size of `ph`: (a) one piece, (b) a cut at k BLOCK + d around the first three block
    boundaries, (c) 1-byte pieces for the messages of <= 300 bytes, (d) seeded random pieces with empty pieces in between"""
    B = BLOCK[ph]
    n = len(msgs)
    every = list(range(n))
    out = {"one_piece": (every, [[0, len(m)] for m in msgs])}
    for k in (1, 2, 3):
        for d in (-1, 0, 1):
            p = k * B + d
            out[f"cut_{k}B{d:+d}"] = (every, [[0, min(p, len(m)), len(m)] for m in msgs])
    small = [i for i in every if len(msgs[i]) <= 300]
    out["bytes"] = (small, [list(range(len(msgs[i]) + 1)) + [len(msgs[i])] * (300 - len(msgs[i])) for i in small])
    for seed in (1, 2, 3):
        rng = np.random.default_rng(1000 + seed)
        U = 9
        cuts = []
        for j, m in enumerate(msgs):
            inner = sorted(int(x) for x in rng.integers(0, len(m) + 1, U - 1))
            for u in rng.choice(U - 1, 2, replace=False):  # two empty pieces somewhere in the middle
                inner[u] = inner[u - 1] if u else 0
            inner.sort()
            if j % 3 == 0:
                inner[-1] = len(m)                          # the last update is empty
            cuts.append([0] + inner + [len(m)])
        out[f"random_{seed}"] = (every, cuts)
    return out


def coverage(msgs, sched, ph):
    """what the schedules exercise, counted over (op, update): the conditions the GPU test asserts before it runs"""
    B = BLOCK[ph]
    c = dict(tail_block_minus_1=0, completes_exactly=0, completes_then_2_blocks=0, final_update_empty=0, empty_piece=0, one_byte=0)
    for ops, cuts in sched.values():
        for i, cs in zip(ops, cuts):
            assert cs[0] == 0 and cs[-1] == len(msgs[i]) and all(a <= b for a, b in zip(cs, cs[1:])), (i, cs[:4])
            for u in range(len(cs) - 1):
                fill, plen = cs[u] % B, cs[u + 1] - cs[u]
                c["tail_block_minus_1"] += fill == B - 1 and plen > 0
                c["completes_exactly"] += fill > 0 and fill + plen == B
                c["completes_then_2_blocks"] += fill > 0 and plen >= (B - fill) + 2 * B
                c["empty_piece"] += plen == 0
                c["one_byte"] += plen == 1
            c["final_update_empty"] += len(cs) > 2 and cs[-1] == cs[-2] and cs[-1] > 0
    return c


def hashlib_incremental(msgs, ops, cuts, ph):
    """hashlib fed the same pieces: the digests the device must reach"""
    new = {"SHA256": hashlib.sha256, "SHA512": hashlib.sha512, "SHAKE128": hashlib.shake_128}[ph]
    out = []
    for i, cs in zip(ops, cuts):
        h = new()
        for u in range(len(cs) - 1):
            h.update(msgs[i][cs[u]:cs[u + 1]])
        out.append(h.digest(32) if ph == "SHAKE128" else h.digest())
    return out
