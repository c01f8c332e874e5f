"""Private keys whose t0 makes the signer's ||c t0||inf < gamma2 test (FIPS 204 Algorithm 7, ml_dsa.rs:312) DECIDE signatures, the batches
signed with them and the oracle's per-attempt trace of those batches.  Shared by test_ct0_cases_cpu.py (the inputs do what they claim,
on the oracle alone) and test_gpu_ct0_bound.py (every device route signs them like the oracle).  No GPU import, no fixture file:
everything is derived from the seeds below.

An honest ML-DSA-44 key fails the test in about 1e-7 of the attempts.  PrivateKey::try_from_bytes takes any t0 field (every 13-bit
pattern decodes into [-4095, 4096]), and with rows of +-v under random signs every coefficient of c t0 is v times an odd integer m,
|m| <= tau = 39 (a 39-step +-1 walk): v m can be put just below gamma2 = 95 232, just above it, or on it.

    v = 3809   25 v = 95 225 = gamma2 - 7: |m| = 25 passes the test itself but not the bound ||c t0 - c s2||inf + beta < gamma2
    v = 3810   25 v = 95 250 = gamma2 + 18: |m| = 25 fails it
    v = 3072   31 v = gamma2 exactly (the only such pair: 95 232 = 2^10 * 3 * 31): |m| = 31, 3e-7 per coefficient, is the equality case

Rows 0 and K - 1 are crafted and the others are zero: all K rows at that magnitude would put the hint weight over omega in almost
every attempt.

Further keys: v = 3809 with every s2 field all-ones (s2 = -5: the device's route for out-of-range s2, which has c t0 itself and adds
no beta); for ML-DSA-65 / 87, where the device compiles the test out on tau * 2^12 < gamma2, two rows of {+4096, -4095} (the largest
encodable |t0|); per set the honest key with row 0, and with every row, all +4096: coherent rows make c t0 large in whole runs of
coefficients and with it the hint weight -- far past omega, and with every row past 255 (ML-DSA-44 and 87), where the running hint
count no longer fits the byte HintBitPack writes per row.  For ML-DSA-65 no encodable t0 gets there in a test: a coefficient gives a
hint with probability ~|c t0| / (2 gamma2) <= 49 * 4096 / 523 776 = 0.38, so 256 hints among the 1 536 coefficients need a mean |c t0| of
~21 * 4096, which every-row-coherent t0 (the largest runs there are) reaches only when the challenge's 49 signs sum to ~35 or more,
5 standard deviations, ~1e-6 per attempt; 256 ops reach 195.  The last family of every set is the honest key itself.

Classes (of an op, by the FIRST attempt that passes ml_dsa.rs:280 and has at most omega hints -- the first one the t0 test can decide):

    reject_decided      ct0_norm >= gamma2                       the test rejects an attempt nothing else rejects
    accept_by_exact     ct0_norm <  gamma2 <= d_norm + beta      the bound cannot decide, c t0 proper accepts
    accept_needs_beta   d_norm   >= gamma2 >  ct0_norm           ... and d = c t0 - c s2 alone, without beta, is already over gamma2
    equal_gamma2        ct0_norm == gamma2                       `>` for `>=` accepts it
    reject_needs_beta   ct0_norm >= gamma2 >  d_norm             the bound WITHOUT beta (max|d| < gamma2) would accept it unseen by c t0 proper
    oor_in_beta_margin  gamma2 - beta <= ct0_norm < gamma2       (the key with out-of-range s2: there the device has c t0 itself, and
                                                                  adding beta would reject these)
"""
import functools
import hashlib
import os

import numpy as np

from oracle import oracle as orc

XI = bytes(range(3, 35))      # the honest key every crafted key starts from
TRACE_CAP = 96                # attempts recorded per op (the honest loop takes ~4.5 on average; an op that takes more keeps its first 96)
CLASSES = ("reject_decided", "accept_by_exact", "accept_needs_beta", "equal_gamma2", "reject_needs_beta", "oor_in_beta_margin")
THREADS = min(16, os.cpu_count() or 1)

# family -> (t0 recipe, sign-pattern seeds = one key each, ops per key).  The equality family gave 1 op in 4 096 with the first seed:
# the union over EQ_SEEDS (consecutive from the same 7, EQ_OPS each) is where the condition `equal_gamma2 >= 4` holds (1 + 2 + 0 + 1;
# seeds 7 ... 46 give 28 in 163 840 ops, one per ~5 900).
EQ_SEEDS, EQ_OPS = (7, 8, 9, 10), 4096
FAMILIES = {
    44: {
        "v3809": dict(v=3809, seeds=(7,), n=4096),
        "v3810": dict(v=3810, seeds=(7,), n=4096),
        "v3072": dict(v=3072, seeds=EQ_SEEDS, n=EQ_OPS),
        "v3809_s2_ones": dict(v=3809, seeds=(7,), n=4096, s2_ones=True),
        "coherent_row": dict(coherent=1, seeds=(0,), n=512),
        "coherent_all_rows": dict(coherent=4, seeds=(0,), n=256),
        "honest": dict(coherent=0, seeds=(0,), n=64),
    },
    65: {
        "two_rows_extreme": dict(extreme=True, seeds=(7,), n=1024),
        "coherent_row": dict(coherent=1, seeds=(0,), n=256),
        "coherent_all_rows": dict(coherent=6, seeds=(0,), n=256),
        "honest": dict(coherent=0, seeds=(0,), n=64),
    },
    87: {
        "two_rows_extreme": dict(extreme=True, seeds=(7,), n=1024),
        "coherent_row": dict(coherent=1, seeds=(0,), n=256),
        "coherent_all_rows": dict(coherent=8, seeds=(0,), n=256),
        "honest": dict(coherent=0, seeds=(0,), n=64),
    },
}
# What the inputs must give for the tests to mean anything (requirements on the inputs, not measurements): family -> class -> least
# number of ops.  tests/test_ct0_cases_cpu.py holds the batch to them; each GPU route holds the ops it signs to them.
CONDITIONS = {
    # reject_needs_beta: the device accepts on the bound and takes c t0 proper only where the bound fails, so a bound that forgot beta
    # shows on no accept_needs_beta op (those go to c t0 proper and are accepted there), only where c s2 pulls d under gamma2 at every
    # coefficient that has |c t0| >= gamma2.  c s2 is a sum of 39 terms of variance 2 (eta = 2), ~N(0, 78): it must be <= -19 against
    # the sign of 25 v = gamma2 + 18 (1.8 % of v3810's reject_decided ops: ~3 of the 158 its batch gives, at least 2 required), and
    # <= -1 against 31 v = gamma2 (48 % of v3072's equality ops: at least 1 of the 4 required).
    "v3810": {"reject_decided": 20, "reject_needs_beta": 2},
    "v3809": {"accept_by_exact": 50, "accept_needs_beta": 8},
    "v3072": {"equal_gamma2": 4, "reject_needs_beta": 1},
    # The key with out-of-range s2 has v3809's t0, so the same walks: "|m| = 25 is the largest" puts an op into oor_in_beta_margin as
    # it puts one into v3809's accept_by_exact (d + beta >= c always), hence the same 50; |m| >= 27 (reject_decided) is the rarer
    # event and gets the threshold of v3809's rarer class.
    "v3809_s2_ones": {"reject_decided": 8, "oor_in_beta_margin": 50},
}


def shake(tag, i, n=32):
    return hashlib.shake_256(tag + int(i).to_bytes(8, "little")).digest(n)


def layout(pset):
    """byte offsets of the wire private key's sections (encodings.rs sk_encode): (s1, s2, t0, end)"""
    p = orc.params(pset)
    eb = 3 if p.eta == 2 else 4
    s1 = 128
    s2 = s1 + p.l * 32 * eb
    t0 = s2 + p.k * 32 * eb
    return s1, s2, t0, t0 + p.k * 416


@functools.lru_cache(maxsize=None)
def honest_sk(pset):
    return orc.sk_into_bytes(pset, orc.keygen_from_seed(pset, XI)[1])


def encode_t0(t0):
    """BitPack(t0, 2^12 - 1, 2^12) per row: 416 bytes each"""
    return b"".join(orc.bit_pack(row, 4095, 4096, 416) for row in np.asarray(t0, dtype=np.int32))


def decode_t0(pset, sk_bytes):
    _, _, off, end = layout(pset)
    assert end == len(sk_bytes)
    rows = []
    for i in range(orc.params(pset).k):
        ok, row = orc.bit_unpack(sk_bytes[off + 416 * i: off + 416 * (i + 1)], 4095, 4096)
        assert ok
        rows.append(row)
    return np.stack(rows)


def crafted_t0(pset, recipe, seed):
    k = orc.params(pset).k
    if "coherent" in recipe:  # the honest rows, the first `coherent` of them all +4096 (none: the honest key itself, the control)
        t0 = decode_t0(pset, honest_sk(pset)).copy()
        t0[:recipe["coherent"]] = 4096
        return t0
    t0 = np.zeros((k, 256), dtype=np.int32)
    rng = np.random.default_rng(seed)
    vals = [-4095, 4096] if recipe.get("extreme") else [-recipe["v"], recipe["v"]]
    t0[0] = rng.choice(vals, 256)
    t0[k - 1] = rng.choice(vals, 256)
    return t0


def crafted_sk(pset, recipe, seed):
    s1, s2, t0, end = layout(pset)
    sk = bytearray(honest_sk(pset))
    if recipe.get("s2_ones"):  # every s2 field all-ones: s2 = eta - (2^bits - 1), out of range
        sk[s2:t0] = b"\xff" * (t0 - s2)
    sk[t0:end] = encode_t0(crafted_t0(pset, recipe, seed))
    return bytes(sk)


@functools.lru_cache(maxsize=None)
def batch(pset):
    """The set's batch: keys (wire bytes, one per family and seed), and per op its key, message (32 bytes) and rnd.  Ops of a family
    are contiguous: slices[family] = (first op, one past the last)."""
    keys, names, kidx, slices, msgs, rnd = [], [], [], {}, [], []
    for fam, recipe in FAMILIES[pset].items():
        lo = len(kidx)
        for seed in recipe["seeds"]:
            tag = b"ct0-%d-%s-%d-" % (pset, fam.encode(), seed)  # (a key's ops do not depend on where the batch puts them)
            kidx += [len(keys)] * recipe["n"]
            msgs += [shake(tag + b"msg", i) for i in range(recipe["n"])]
            rnd += [shake(tag + b"rnd", i) for i in range(recipe["n"])]
            keys.append(crafted_sk(pset, recipe, seed))
            names.append((fam, seed))
        slices[fam] = (lo, len(kidx))
    return dict(pset=pset, n=len(kidx), keys=keys, names=names, kidx=np.array(kidx, dtype=np.uint32), slices=slices, msgs=msgs, rnd=rnd)


@functools.lru_cache(maxsize=None)
def oracle_keys(pset):
    return [orc.sk_try_from_bytes(pset, sk) for sk in batch(pset)["keys"]]


@functools.lru_cache(maxsize=None)
def traced(pset):
    """the oracle's signatures of the batch (pure mode, empty ctx) with the trace: (sigs uint8 [n, SIG_LEN], iterations [n], trace [n, CAP])"""
    b = batch(pset)
    sigs, iters, trace = orc.sign_trace_batch_mt(pset, oracle_keys(pset), b["kidx"], b["msgs"], b["rnd"], THREADS, mode=0, cap=TRACE_CAP)
    for a in (sigs, iters, trace):
        a.setflags(write=False)
    return sigs, iters, trace


def classify(pset, iters, trace):
    """class name -> bool [n]: membership by the first recorded attempt that reached the t0 test with hsum <= omega"""
    p = orc.params(pset)
    n, cap = trace.shape
    recorded = np.arange(cap)[None, :] < np.minimum(iters, cap)[:, None]
    qual = recorded & (trace["ct0_norm"] >= 0) & (trace["hsum"] <= p.omega)
    has = qual.any(axis=1)
    first = trace[np.arange(n), qual.argmax(axis=1)]
    c, d = first["ct0_norm"], first["d_norm"]
    g2, beta = p.gamma2, p.beta
    return {
        "reject_decided": has & (c >= g2),
        "accept_by_exact": has & (c < g2) & (d + beta >= g2),
        "accept_needs_beta": has & (d >= g2) & (c < g2),
        "equal_gamma2": has & (c == g2),
        "reject_needs_beta": has & (c >= g2) & (d < g2),
        "oor_in_beta_margin": has & (c >= g2 - beta) & (c < g2),
    }


@functools.lru_cache(maxsize=None)
def classes(pset):
    _, iters, trace = traced(pset)
    return classify(pset, iters, trace)


def counts(pset, ops=None):
    """family -> class -> number of ops (restricted to the op indices `ops` if given)"""
    b, cl = batch(pset), classes(pset)
    sel = np.ones(b["n"], dtype=bool)
    if ops is not None:
        sel[:] = False
        sel[np.asarray(ops, dtype=np.int64)] = True
    return {fam: {c: int((cl[c][lo:hi] & sel[lo:hi]).sum()) for c in CLASSES} for fam, (lo, hi) in b["slices"].items()}


def unmet(cnt):
    """the CONDITIONS a counts() result misses: list of (family, class, got, need)"""
    return [(fam, c, cnt[fam][c], need) for fam, cond in CONDITIONS.items() if fam in cnt for c, need in cond.items() if cnt[fam][c] < need]
