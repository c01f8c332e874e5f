"""The crafted-t0 keys of ct0_cases.py do what they claim -- on the oracle alone.  The device side is tests/test_gpu_ct0_bound.py.

Class sizes are conditions on the inputs, not measurements: with fewer ops in a class than required, the GPU tests would compare signatures
that the ||c t0||inf < gamma2 test (ml_dsa.rs:312) never decided."""
import numpy as np
import pytest

import ct0_cases as cc
from oracle import oracle as orc

SETS = (44, 65, 87)


def test_the_trace_observes_sign_internal_without_changing_it():
    """orc_sign_internal_trace signs what orc_sign_internal signs, in as many attempts, and its records are the loop's own decisions:
    only the last attempt is accepted, an attempt that stops at ml_dsa.rs:280 has no t0 figures, every other rejected one fails the
    t0 test or the hint weight, and d = c t0 - c s2 stays within ||c s2||inf <= beta of c t0 for a key with s2 in range."""
    for pset in SETS:
        p, b = orc.params(pset), cc.batch(pset)
        sigs, iters, trace = cc.traced(pset)
        keys = cc.oracle_keys(pset)
        for i in range(0, b["n"], b["n"] // 64):
            want, it = orc.sign_internal(pset, keys[b["kidx"][i]], b["msgs"][i], b["rnd"][i], mode=0, want_iters=True)
            assert sigs[i].tobytes() == want and iters[i] == it, (pset, i)
            one_sig, one_tr, one_it = orc.sign_internal_trace(pset, keys[b["kidx"][i]], b["msgs"][i], b["rnd"][i], mode=0, cap=cc.TRACE_CAP)
            assert one_sig == want and one_it == it and np.array_equal(one_tr, trace[i, :min(it, cc.TRACE_CAP)]), (pset, i)
        assert iters.min() >= 1
        for fam in cc.CONDITIONS:  # the classified families: every op's accepted attempt is on record (elsewhere a long op keeps its first CAP)
            if fam in b["slices"]:
                lo, hi = b["slices"][fam]
                assert iters[lo:hi].max() <= cc.TRACE_CAP, (fam, int(iters[lo:hi].max()))
        rec = np.arange(cc.TRACE_CAP)[None, :] < iters[:, None]
        last = np.arange(cc.TRACE_CAP)[None, :] == iters[:, None] - 1
        assert np.array_equal(trace["accept"] == 1, last)
        early = rec & ((trace["z_norm"] >= p.gamma1 - p.beta) | (trace["r0_norm"] >= p.gamma2 - p.beta))
        for f in ("ct0_norm", "d_norm", "hsum"):
            assert (trace[f][early] == -1).all() and (trace[f][rec & ~early] >= 0).all(), (pset, f)
        late_reject = rec & ~early & ~last
        assert ((trace["ct0_norm"] >= p.gamma2) | (trace["hsum"] > p.omega))[late_reject].all()
        assert ((trace["ct0_norm"] < p.gamma2) & (trace["hsum"] <= p.omega))[last].all()
        assert (last.any(axis=1) == (iters <= cc.TRACE_CAP)).all()
        for fam, (lo, hi) in b["slices"].items():
            if not cc.FAMILIES[pset][fam].get("s2_ones"):
                t = trace[lo:hi][(rec & ~early)[lo:hi]]
                assert (np.abs(t["d_norm"] - t["ct0_norm"]) <= p.beta).all(), (pset, fam)


def test_class_sizes_meet_their_conditions():
    """ML-DSA-44, per family over its whole batch (ct0_cases.CONDITIONS): reject_decided >= 20 on v = 3810, accept_by_exact >= 50 and
    accept_needs_beta >= 8 on v = 3809, equal_gamma2 >= 4 on v = 3072 (the union over ct0_cases.EQ_SEEDS), reject_needs_beta (what a bound
    without beta on the device would let through) >= 2 on v = 3810 and >= 1 on v = 3072, and the two conditions of the out-of-range-s2 key."""
    cnt = cc.counts(44)
    print("class sizes:", cnt)
    assert cc.unmet(cnt) == []
    assert set(cc.CONDITIONS) <= set(cnt)
    assert cc.CONDITIONS["v3810"]["reject_decided"] == 20 and cc.CONDITIONS["v3809"] == {"accept_by_exact": 50, "accept_needs_beta": 8} \
        and cc.CONDITIONS["v3072"]["equal_gamma2"] == 4


def test_classes_are_what_the_loop_did():
    """A reject_decided op's first attempt to reach the t0 test is NOT the accepted one and fails nothing else; an accept_by_exact op's
    IS the accepted one although d + beta is over gamma2; the sets nest as the definitions say."""
    p = orc.params(44)
    _, iters, trace = cc.traced(44)
    cl = cc.classes(44)
    rec = np.arange(cc.TRACE_CAP)[None, :] < iters[:, None]
    qual = rec & (trace["ct0_norm"] >= 0) & (trace["hsum"] <= p.omega)
    first = qual.argmax(axis=1)
    assert qual.any(axis=1).all()  # (the accepted attempt qualifies)
    accepted_first = first == iters - 1
    assert not accepted_first[cl["reject_decided"]].any()
    assert accepted_first[cl["accept_by_exact"]].all() and accepted_first[cl["oor_in_beta_margin"]].all()
    assert (cl["accept_needs_beta"] <= cl["accept_by_exact"]).all() and (cl["equal_gamma2"] <= cl["reject_decided"]).all()
    assert (cl["reject_needs_beta"] <= cl["reject_decided"]).all()
    at = trace[np.arange(len(iters)), first]
    assert (at["ct0_norm"][cl["equal_gamma2"]] == 95232).all()
    # the crafted magnitudes: every coefficient of c t0 is an odd multiple of v
    b = cc.batch(44)
    for fam in ("v3809", "v3810", "v3072"):
        lo, hi = b["slices"][fam]
        v = cc.FAMILIES[44][fam]["v"]
        c = at["ct0_norm"][lo:hi]
        assert (c % v == 0).all() and ((c // v) % 2 == 1).all() and (c // v).max() <= p.tau, fam


@pytest.mark.parametrize("pset", [65, 87])
def test_signing_with_extreme_t0_terminates_like_an_honest_key(pset):
    """Two rows of {+4096, -4095} (and one coherent row) keep the loop within 2x of the honest key's mean iterations; the test of
    ml_dsa.rs:312 never fails for these sets (tau * 2^12 < gamma2), whatever t0 is."""
    p, b = orc.params(pset), cc.batch(pset)
    _, iters, trace = cc.traced(pset)
    n = 1024
    honest = orc.sk_try_from_bytes(pset, cc.honest_sk(pset))
    _, it_h, _ = orc.sign_trace_batch_mt(pset, [honest], np.zeros(n, dtype=np.uint32), b["msgs"][:n], b["rnd"][:n], cc.THREADS, mode=0, cap=4)
    for fam in ("two_rows_extreme", "coherent_row"):
        lo, hi = b["slices"][fam]
        print(pset, fam, "mean iterations", iters[lo:hi].mean(), "honest", it_h.mean())
        assert iters[lo:hi].mean() <= 2 * it_h.mean(), (pset, fam)
    lo, hi = b["slices"]["two_rows_extreme"]
    worst = int(trace["ct0_norm"][lo:hi].max())
    assert p.gamma2 // 4 < worst < p.gamma2 and worst <= p.tau * 4096, (pset, worst)  # large, and still under gamma2
    assert not any(cc.counts(pset)[fam]["reject_decided"] for fam in b["slices"])


@pytest.mark.parametrize("pset", SETS)
def test_coherent_rows_drive_the_hint_weight_past_omega_and_255(pset):
    """One coherent row: attempts with more than omega hints (up to 132 / 75 / 88 for ML-DSA-44 / 65 / 87; it does NOT reach 255).
    Every row coherent: past 255 for ML-DSA-44 (358) and 87 (290), at ~3x the honest iterations.  ML-DSA-65 stops at 195: 255 is out of
    reach of any encodable t0 there (~1e-6 per attempt, see ct0_cases), so twice omega is what is required of it."""
    p, b = orc.params(pset), cc.batch(pset)
    _, iters, trace = cc.traced(pset)
    lo, hi = b["slices"]["coherent_row"]
    assert trace["hsum"][lo:hi].max() > p.omega
    lo, hi = b["slices"]["coherent_all_rows"]
    print(pset, "every row coherent: max hint weight", trace["hsum"][lo:hi].max(), "mean iterations", iters[lo:hi].mean())
    assert trace["hsum"][lo:hi].max() > (255 if pset != 65 else 2 * p.omega)


@pytest.mark.parametrize("pset", SETS)
def test_crafted_keys_are_canonical_wire_keys(pset):
    """Each key decodes to the t0 it was built from and re-encodes (PrivateKey::into_bytes) to the same t0 bytes; everything before
    the s2 section is the honest key's."""
    b = cc.batch(pset)
    s1, s2, t0, end = cc.layout(pset)
    assert end == orc.params(pset).sk_len
    for (fam, seed), sk in zip(b["names"], b["keys"]):
        recipe = cc.FAMILIES[pset][fam]
        want = cc.crafted_t0(pset, recipe, seed)
        assert want.min() >= -4095 and want.max() <= 4096
        assert np.array_equal(cc.decode_t0(pset, sk), want), (fam, seed)
        again = orc.sk_into_bytes(pset, orc.sk_try_from_bytes(pset, sk))
        assert again[t0:] == sk[t0:] and again[:s2] == sk[:s2] == cc.honest_sk(pset)[:s2], (fam, seed)
        if "v" in recipe:
            k = orc.params(pset).k
            assert set(np.unique(want[[0, k - 1]])) == {-recipe["v"], recipe["v"]} and not want[1:k - 1].any()
    assert len(set(b["keys"])) == len(b["keys"])
