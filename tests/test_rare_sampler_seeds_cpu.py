"""The searched seeds of tests/golden/rare_sampler_seeds.json.gz on the CPU: every entry has the property it is filed under, the
fixture keeps its quotas, the oracle equals the FIPS 204 restatement of rare_sampler_cases.py on every entry (the oracle has
never run these paths either, so a device-equals-oracle test alone would prove nothing), and the subtly wrong samplers are
caught by the searched seeds while the seeds of test_gpu_samplers.py cannot tell them from the right ones."""
import functools
import subprocess
import sys

import numpy as np
import pytest

import rare_sampler_cases as rc
from conftest import ROOT
from oracle import oracle as orc


@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


def test_fixture_quotas(fx):
    rc.check_quotas(fx)


def test_every_entry_has_its_property(fx):
    n = 0
    for cat, pset, e in rc.entries(fx):
        rc.check_entry(cat, pset, e)
        n += 1
    assert n >= 8 + 10 + 2 * 6 + 3 * (16 + 8)


def test_search_tool_is_self_contained():
    """hashlib and numpy only, and no import of the package, the oracle or the tests"""
    src = open(f"{ROOT}/tools/find_rare_sampler_seeds.py").read()
    mods = {ln.split()[1].split(".")[0] for ln in src.splitlines() if ln.startswith(("import ", "from "))}
    assert mods <= {"argparse", "gzip", "hashlib", "json", "os", "sys", "time", "numpy"}, mods


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_oracle_equals_restatement_expand_s(fx, pset):
    k, l, eta = (rc.SETS[pset][x] for x in ("k", "l", "eta"))
    streams = rc.es_streams(fx, pset)
    assert streams
    for rho_prime, stream in streams:
        want1, want2, infos = rc.expand_s(pset, rho_prime)
        got1, got2 = orc.expand_s(k, l, eta, rho_prime)
        assert np.array_equal(got1, want1) and np.array_equal(got2, want2), (rho_prime.hex(), stream)
        poly, used = orc.rej_bounded_poly(eta, rho_prime + stream.to_bytes(2, "little"))
        assert used == infos[stream]["bytes"] and np.array_equal(poly, np.concatenate([want1, want2])[stream]), (rho_prime.hex(), stream)


def test_oracle_third_block_byte_counts(fx):
    """every ES3 stream makes the oracle read past two blocks, every exactly-256 stream stops inside block two"""
    n3 = n2 = 0
    for e in fx["es3_seam"]:
        _, used = orc.rej_bounded_poly(4, bytes.fromhex(e["rho_prime"]) + e["stream"].to_bytes(2, "little"))
        if e["prop"] == "third_block":
            assert used > 272, e
            n3 += 1
        else:
            assert used <= 272, e
            n2 += 1
    for e in fx["es3_keys"]:
        rho_prime = rc.key_streams(65, bytes.fromhex(e["xi"]))[1]
        for st in e["streams"]:
            assert orc.rej_bounded_poly(4, rho_prime + st["stream"].to_bytes(2, "little"))[1] > 272, e
            n3 += 1
    assert n3 >= 16 and n2 >= 2


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_oracle_equals_restatement_expand_a(fx, pset):
    k, l = rc.SETS[pset]["k"], rc.SETS[pset]["l"]
    keys = rc.ea_keys(fx, pset)
    assert len(keys) >= 16
    for xi in keys:
        rho = rc.key_streams(pset, xi)[0]
        want, _ = rc.expand_a(pset, rho)
        assert 0 <= want.min() and want.max() < rc.Q
        assert np.array_equal(orc.expand_a(k, l, rho), want), xi.hex()


def _key_entries(fx, pset):
    keys = rc.ea_keys(fx, pset)
    if pset == 65:
        keys = [bytes.fromhex(e["xi"]) for e in fx["es3_keys"] + fx["es_exact_keys"]] + keys
    return keys


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_oracle_keygen_equals_restatement(fx, pset):
    for xi in _key_entries(fx, pset):
        pk, sk = orc.keygen_from_seed(pset, xi)
        want_pk, want_sk = rc.keygen(pset, xi)
        assert orc.pk_into_bytes(pset, pk) == want_pk, xi.hex()
        assert orc.sk_into_bytes(pset, sk) == want_sk, xi.hex()


def test_restatement_keygen_matches_acvp(acvp_keygen):
    """the restatement's key generation is FIPS 204's: the first three ACVP keyGen cases of each set"""
    for g in acvp_keygen["testGroups"]:
        pset = {"ML-DSA-44": 44, "ML-DSA-65": 65, "ML-DSA-87": 87}[g["parameterSet"]]
        for t in g["tests"][:3]:
            pk, sk = rc.keygen(pset, bytes.fromhex(t["seed"]))
            assert pk.hex().upper() == t["pk"].upper() and sk.hex().upper() == t["sk"].upper(), (pset, t["tcId"])


# ------------------------------------------------------------------------------ negative controls
def _differs_a(pset, rho, r, s, mutant):
    seed = rho + bytes([s, r])
    return mutant(seed)[0] != rc.rej_ntt_poly(seed)[0]


@functools.lru_cache(maxsize=None)
def _legacy_a(pset, rho):
    return rc.expand_a(pset, rho)[0]


# (pset, value, candidate index mod 4) of the boundary candidates the old seeds of test_gpu_samplers.py happen to hold
LEGACY_CELLS = [(65, "q-1", 1), (87, "q", 3)]


def _a_mutants():
    m = {"accepts_q": (rc.ntt_accepts_q, lambda e: e["value"] == "q"),
         "rejects_q_minus_1": (rc.ntt_rejects_q_minus_1, lambda e: e["value"] == "q-1")}
    for pos in range(4):
        for kind in ("q", "q-1"):
            m[f"wrong_at_{pos}_{kind}"] = (rc.ntt_wrong_at(pos, kind), lambda e, pos=pos, kind=kind: e["value"] == kind and e["pos"] == pos)
    return m


@pytest.mark.parametrize("name", sorted(_a_mutants()))
def test_wrong_rej_ntt_poly_is_caught_by_the_fixture_only(fx, name):
    mutant, aimed = _a_mutants()[name]
    for pset in (44, 65, 87):
        es = [e for e in fx["ea_boundary"][str(pset)] if aimed(e)]
        assert len(es) >= 2
        for e in es:   # EVERY entry of the cell shows the fault, in the stream it names
            assert _differs_a(pset, bytes.fromhex(e["rho"]), e["r"], e["s"], mutant), (name, e)
        one_pos = name.startswith("wrong_at")
        for e in fx["ea_boundary"][str(pset)]:
            if one_pos and not aimed(e) and len(rc.ea_profile(bytes.fromhex(e["rho"]), e["r"], e["s"])["boundary"]) == 1:
                # the one-position fault is invisible to the other cells: all eight are needed
                assert not _differs_a(pset, bytes.fromhex(e["rho"]), e["r"], e["s"], mutant), (name, e)
    # the seeds the GPU sampler tests have used so far.  They are NOT blind everywhere: two of their ~10 000 streams hold a boundary
    # candidate (LEGACY_CELLS), each on one seam form of one set, so the four mutants aimed at those two cells already differ
    # there and the claim is not made for them.  The other six one-position faults pass the old seeds unseen.
    seen = any(not np.array_equal(rc.expand_a(pset, rho, sampler=mutant)[0], _legacy_a(pset, rho)) for pset, rho in rc.legacy_expand_a_rho())
    value = {"accepts_q": "q", "rejects_q_minus_1": "q-1"}.get(name) or name.split("_")[3]
    reached = [c for c in LEGACY_CELLS if c[1] == value and (not one_pos or c[2] == int(name.split("_")[2]))]
    assert seen == bool(reached), (name, reached)


@pytest.mark.parametrize("name", ["two_blocks_only", "keeps_consuming"])
def test_wrong_rej_bounded_poly_is_caught_by_the_fixture_only(fx, name):
    mutant = {"two_blocks_only": rc.bounded_two_blocks_only, "keeps_consuming": rc.bounded_keeps_consuming}[name]

    def differs(eta, rho_prime, stream):
        seed = rho_prime + stream.to_bytes(2, "little")
        return mutant(eta, seed)[0] != rc.rej_bounded_poly(eta, seed)[0]

    if name == "two_blocks_only":
        aimed = [(4, rp, st) for rp, st in rc.es_streams(fx, 65)
                 if rc.es_profile(4, rp, st)["blocks"] == 3]
        assert len(aimed) >= 16
        assert all(differs(*a) for a in aimed)
        # exactly 256 in two blocks: the two-block form is still right there
        exact = [e for e in fx["es3_seam"] if e["prop"] == "exact_256_in_two"]
        assert exact and not any(differs(4, bytes.fromhex(e["rho_prime"]), e["stream"]) for e in exact)
    else:
        # a sampler that does not stop is right only where the last block it squeezed holds no accepted half-byte past the
        # 256th: the exactly-256 streams.  Every other entry shows it.
        for pset in (44, 65, 87):
            eta = rc.SETS[pset]["eta"]
            for rp, st in rc.es_streams(fx, pset):
                p = rc.es_profile(eta, rp, st)
                fills_exactly = (p["blocks"] == 1 and p["acc1"] == 256) or (p["blocks"] == 2 and p["acc2"] == 256)
                assert differs(eta, rp, st) == (not fills_exactly), (pset, rp.hex(), st)
        assert any(differs(4, rp, st) for rp, st in rc.es_streams(fx, 65))
    legacy_diff = 0
    for pset, rho_prime in rc.legacy_expand_s_rho():
        eta = rc.SETS[pset]["eta"]
        g1, g2, _ = rc.expand_s(pset, rho_prime, sampler=mutant)
        w1, w2, _ = rc.expand_s(pset, rho_prime)
        legacy_diff += not (np.array_equal(g1, w1) and np.array_equal(g2, w2))
    if name == "two_blocks_only":
        # no eta = 4 stream of the old seeds needs a third block, and eta = 2 never does
        assert legacy_diff == 0
    else:
        # NOT blind: nearly every ordinary stream has accepted half-bytes after its 256th in the block it stops in, so a sampler
        # that keeps consuming already differs on the old seeds -- the claim "the old inputs cannot see it" does not hold for
        # this mutant and is not made.  What the old seeds never did is run it across a third block.
        assert legacy_diff > 0
        assert not any(i["blocks"] == 3 for pset, rp in rc.legacy_expand_s_rho() if pset == 65 for i in rc.expand_s(65, rp)[2])


def test_what_the_old_seeds_reach():
    """the premise of the fixture, recomputed: no third ExpandS block under the old sampler seeds, and two of the eight
    boundary cells of RejNTTPoly, once each"""
    for pset, rho_prime in rc.legacy_expand_s_rho():
        assert all(i["blocks"] <= 2 for i in rc.expand_s(pset, rho_prime)[2])
    cells = []
    for pset, rho in rc.legacy_expand_a_rho():
        k, l = rc.SETS[pset]["k"], rc.SETS[pset]["l"]
        cells += [(pset, v, i % 4) for r in range(k) for s in range(l) for i, v in rc.ea_profile(rho, r, s)["boundary"]]
    assert cells == LEGACY_CELLS


def test_search_tool_reproduces_the_fixture():
    r = subprocess.run([sys.executable, f"{ROOT}/tools/find_rare_sampler_seeds.py", "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
