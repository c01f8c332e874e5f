"""The long-running signing ops of long_tail_cases.py are what they claim -- on the oracle alone.  The device side is
tests/test_gpu_sign_long_tail.py.

The numbers of long ops are conditions on the inputs, not measurements: without an op above 32 iterations no one-op call at default
options is left unfinished by its planned round, and the GPU tests would compare signatures no re-sign leg ever produced."""
import numpy as np
import pytest

import long_tail_cases as lt
from oracle import oracle as orc


@pytest.mark.parametrize("pset", lt.SETS)
def test_fixture_is_what_the_oracle_computes_from_the_seeds(pset):
    """tests/golden/long_tail_ops.json lists, per set, the ops of the 16 384-op batch with more than 25 iterations and their counts,
    the number above 14 and the maximum: equal to the oracle's trace of the batch derived from the seeds; the conditions hold (at least
    1 op above 32 = MLDSA_OPT_SPEC_MAX's default, at least 8 above 25); a listed op signed on its own takes that many iterations."""
    sigs, iters, _ = lt.traced(pset)
    assert iters.shape == (lt.N_BATCH,) and iters.min() >= 1
    got = lt.summary(iters)
    print(pset, "ops above 14 / 25 / 32:", got["over_14"], len(got["ops"]), int((iters > 32).sum()), "max", got["max"])
    assert got == lt.fixture()[str(pset)]
    assert lt.unmet(iters) == []
    assert lt.CONDITIONS == {32: 1, 25: 8} and lt.SPEC_MAX_DEFAULT == 32
    ops, it = lt.long_ops(pset, 32)
    assert len(ops) >= 1 and np.array_equal(iters[ops], it) and (it > 32).all()
    for i in ops[:2]:
        sig, n_it = lt.oracle_sig(pset, int(i))
        assert sig == sigs[i].tobytes() and n_it == iters[i], (pset, int(i))
    pad = lt.padded(pset)
    assert pad.size == 64 and np.unique(pad).size == 64 and (iters[pad] > lt.LONG).sum() == min(64, len(got["ops"]))
    assert iters[pad].max() == iters.max() and set(lt.long_ops(pset, 32)[0]) <= set(pad)


def test_fixture_has_the_counts_the_cases_were_chosen_for():
    """the figures the GPU cases lean on: ML-DSA-44 one op above 32 (op 6192, 50 iterations), ML-DSA-65 fourteen, ML-DSA-87 two"""
    assert [list(map(int, lt.long_ops(s, 32)[0])) for s in (44, 87)] == [[6192], [156, 4285]]
    assert list(map(int, lt.long_ops(44, 32)[1])) == [50]
    assert list(map(int, lt.long_ops(65, 32)[0][:6])) == [535, 4056, 5635, 7084, 8341, 8342] and len(lt.long_ops(65, 32)[0]) == 14
    assert [len(lt.long_ops(s)[0]) for s in lt.SETS] == [26, 82, 8]
    assert [lt.fixture()[str(s)]["over_14"] for s in lt.SETS] == [409, 811, 271]
    assert [lt.fixture()[str(s)]["max"] for s in lt.SETS] == [50, 47, 36]


@pytest.mark.parametrize("pset", lt.SETS)
def test_unfinished_after_r_rounds_is_what_the_trace_shows(pset):
    """unfinished_after(iterations, r): with one candidate per round an op is unsigned after r rounds exactly when none of its first
    r attempts was accepted -- read off the oracle's per-attempt trace of the first 261 ops (r = 1 ... 8: both outcomes occur for each)
    and, for per_round candidates a round, off the same trace in blocks."""
    cap = 8
    _, iters, trace = lt.traced(pset, lt.N_FORCED, cap)
    accepted = trace["accept"] == 1
    assert (accepted.sum(axis=1) == (iters <= cap)).all()
    for r in range(1, cap + 1):
        want = ~accepted[:, :r].any(axis=1)
        assert np.array_equal(lt.unfinished_after(iters, r), want), r
        assert 0 < want.sum() < lt.N_FORCED
    for rounds, per in ((1, 4), (2, 4), (2, 3), (4, 2)):
        assert np.array_equal(lt.unfinished_after(iters, rounds, per), ~accepted[:, :rounds * per].any(axis=1))
    assert np.array_equal(iters, lt.traced(pset)[1][:lt.N_FORCED])  # (a prefix of the batch: the same ops)


def test_forced_variants_are_the_oracles_own_signatures():
    """variant(): per op the key (by key_idx over 6 keys, or key i), the ctx (0 ... 8 bytes, or none), the message (or the empty one);
    its signatures verify under the matching public key, its iteration counts differ from the batch's (other keys), and the
    HashML-DSA form signs OID || SHA-512(M) in pre-hash mode."""
    n = 24
    pk = lt.op_keys(44, n)[0]
    for with_kidx, with_ctx, empty, ph in ((True, True, False, None), (False, False, True, None), (True, True, False, "SHA512")):
        v = lt.variant(44, n, with_kidx, with_ctx, empty, ph=ph)
        assert v["sk"].shape[0] == (lt.NK_FORCED if with_kidx else n)
        if with_kidx:
            assert v["kidx"].max() < lt.NK_FORCED and np.unique(v["kidx"]).size == lt.NK_FORCED
        for i in range(n):
            pk_o = orc.pk_try_from_bytes(44, pk[int(v["kidx"][i]) if with_kidx else i].tobytes())
            ctx = v["ctxs"][i] if with_ctx else b""
            assert len(ctx) == (i % 9 if with_ctx else 0) and len(v["msgs"][i]) == (0 if empty else 32)
            if ph:
                assert orc.hash_verify(44, pk_o, v["msgs"][i], v["sig"][i].tobytes(), ctx, ph), i
            else:
                assert orc.verify_internal(44, pk_o, v["msgs"][i], v["sig"][i].tobytes(), ctx=ctx, mode=0), i
        assert v["iters"].min() >= 1
    assert not np.array_equal(lt.variant(44, n, True, True, False)["iters"], lt.traced(44, lt.N_FORCED, 8)[1][:n])
