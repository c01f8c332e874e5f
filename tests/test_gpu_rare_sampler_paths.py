"""The searched seeds of tests/golden/rare_sampler_seeds.json.gz on the device: the third SHAKE256 block of ExpandS with eta = 4, the
block-one edges of eta = 2, RejNTTPoly candidates equal to q - 1 and q at each of the four positions of a candidate group, and
streams with many or awkwardly placed rejections -- through the sampler seams, key generation, signing and verification, on every
route an option selects.  Every comparison is exact; every fixture entry runs on every route (nothing is sampled).

Expected values of the rare rows come from the FIPS 204 restatement in rare_sampler_cases.py AND the oracle (asserted equal here
too); the ordinary rows that pad a call come from the oracle.

Placement.  The lane-per-state kernels give stream g = op * polys_per_op + r to lane g % 64 of wave g // 64.  A rare stream is put
in the lowest and the highest lane an op index can give it (lane 0 / 63 where polys_per_op is odd; ExpandA's 16, 30 and 56
polynomials per op leave g % 64 a fixed residue), in the last, partly filled wave of the grid (whose surplus lanes are done
before the first block), alone among ordinary streams (every other lane of its wave is done a block earlier) and with the other
rare streams in neighbouring ops (several in one wave)."""
import rare_sampler_cases as rc
from fips204_amd import _lib
from fips204_amd.ml_dsa import MODE_INTERNAL, MlDsaBatcher
from gpu_common import *

pytestmark = pytest.mark.gpu

COOP_RANGE = 4096   # polynomials: calls above it leave the cooperative forms whatever MLDSA_OPT_COOP_HASH says


@pytest.fixture(scope="module")
def fx():
    f = rc.load_fixture()
    rc.check_quotas(f)
    return f


class options:
    """force options, read them back, restore on exit"""

    def __init__(self, hp, **kw):
        self.hp, self.want = hp, {getattr(_lib, "OPT_" + k.upper()): v for k, v in kw.items()}

    def __enter__(self):
        self.old = {o: self.hp.get_option(o) for o in self.want}
        try:
            for o, v in self.want.items():
                self.hp.set_option(o, v)
                assert self.hp.get_option(o) == v, (o, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for o, v in self.old.items():
            self.hp.set_option(o, v)
            assert self.hp.get_option(o) == v


def test_defaults(hp):
    assert hp.get_option(_lib.OPT_COOP_HASH) == 1 and hp.get_option(_lib.OPT_SMALL_FUSED) == 256


# ------------------------------------------------------------------------------ placement
def lane_of(ppo, op, r):
    return (op * ppo + r) % 64


def op_for_lane(ppo, r, n_ops, high, taken=()):
    """the op of a call whose stream r sits in the lowest (highest) lane an op not yet taken can give it"""
    lane = lambda op: lane_of(ppo, op, r)
    return min((op for op in range(n_ops) if op not in taken), key=lambda op: (-lane(op) if high else lane(op), op))


def size_with_tail(n_min, ppo):
    """the smallest call >= n_min whose LAST op lies wholly in a last, partly filled wave"""
    n = n_min
    while (n * ppo) % 64 < ppo and not (n * ppo < 64):
        n += 1
    return n


def test_placement_arithmetic():
    assert lane_of(11, op_for_lane(11, 7, 64, False), 7) == 0 and lane_of(11, op_for_lane(11, 7, 64, True), 7) == 63
    assert lane_of(15, op_for_lane(15, 3, 64, False), 3) == 0 and lane_of(8, op_for_lane(8, 5, 64, True), 5) == 61
    for ppo in (8, 11, 15, 16, 30, 56):
        for n_min in (64, 300, 8192):
            n = size_with_tail(n_min, ppo)
            assert n_min <= n < n_min + 64 and (n - 1) * ppo >= (n * ppo) // 64 * 64 and (n * ppo) % 64


def layouts(ppo, entries, n_ops):
    """name -> (n_ops of the call, {op: entry index}) for the entries (each an (input, r) pair: r the rare stream of the op)"""
    out = {}
    if n_ops == 1:
        return {f"alone{j}": (1, {0: j}) for j in range(len(entries))}
    tail = size_with_tail(n_ops, ppo)
    for j, (_, r) in enumerate(entries):
        out[f"low_lane{j}"] = (n_ops, {op_for_lane(ppo, r, n_ops, False): j})
        out[f"high_lane{j}"] = (n_ops, {op_for_lane(ppo, r, n_ops, True): j})
        out[f"tail{j}"] = (tail, {tail - 1: j})
    # several rare streams in one wave: the entries in neighbouring ops from op 1 on, and again at the end of the call
    crowd = {1 + j: j for j in range(len(entries)) if 1 + j < n_ops}
    crowd.update({tail - 1 - j: j for j in range(min(len(entries), 8)) if tail - 1 - j not in crowd})
    out["crowd"] = (tail, crowd)
    return out


# ------------------------------------------------------------------------------ the sampler seams
def seam_entries(fx, pset, kind):
    """(seed, polynomial index within the op) per fixture entry"""
    if kind == "s":
        return rc.es_streams(fx, pset)
    l = rc.SETS[pset]["l"]
    return [(bytes.fromhex(e["rho"]), e["r"] * l + e["s"]) for cat in ("ea_boundary", "ea_shape") for e in fx[cat][str(pset)]]


def seam_call(hp, pset, kind, seeds):
    d = dev(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(len(seeds), -1))
    if kind == "a":
        return hp.expand_a(pset, d).flatten(1, 2)
    return torch.cat(hp.expand_s(pset, d), dim=1)


def seam_oracle(pset, kind, seed):
    k, l, eta = (rc.SETS[pset][x] for x in ("k", "l", "eta"))
    if kind == "a":
        return orc.expand_a(k, l, seed).reshape(k * l, 256)
    return np.concatenate(orc.expand_s(k, l, eta, seed))


def seam_restated(pset, kind, seed):
    if kind == "a":
        return rc.expand_a(pset, seed)[0].reshape(-1, 256)
    s1, s2, _ = rc.expand_s(pset, seed)
    return np.concatenate([s1, s2])


@pytest.mark.parametrize("coop", [0, 1])
@pytest.mark.parametrize("kind", ["s", "a"])
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_seams(hp, fx, pset, kind, coop):
    """mldsa_expand_s on every ES entry, mldsa_expand_a on every EA rho: calls of 1 op, 64 ops and beyond the cooperative range,
    the rare op placed as the module docstring says, every row of every call compared"""
    p = rc.SETS[pset]
    ppo = p["k"] * p["l"] if kind == "a" else p["k"] + p["l"]
    entries = seam_entries(fx, pset, kind)
    assert len(entries) >= (24 if kind == "a" else 9)
    rare = []
    for seed, r in entries:
        want = seam_restated(pset, kind, seed)
        assert np.array_equal(want, seam_oracle(pset, kind, seed))
        rare.append(dev(want))
    large = COOP_RANGE // ppo + 1
    n_max = size_with_tail(large, ppo)
    pad = [shake(b"rare-pad-%s%d" % (kind.encode(), pset), i, 32 if kind == "a" else 64) for i in range(n_max)]
    pad_want = dev(np.stack([seam_oracle(pset, kind, s) for s in pad]))
    n_calls = n_rows = 0
    t0 = time.time()
    with options(hp, coop_hash=coop):
        for size in (1, 64, large):
            assert (size * ppo > COOP_RANGE) == (size == large)
            for name, (n_ops, where) in layouts(ppo, entries, size).items():
                seeds = list(pad[:n_ops])
                want = pad_want[:n_ops].clone()
                for op, j in where.items():
                    seeds[op] = entries[j][0]
                    want[op] = rare[j]
                got = seam_call(hp, pset, kind, seeds)
                torch.cuda.synchronize()
                if not torch.equal(got, want):
                    bad = sorted({int(x) for x in (got != want).any(dim=2).nonzero()[:, 0].cpu()})
                    raise AssertionError(f"{kind} {pset} coop {coop} size {size} {name}: ops {bad[:8]} differ; rare ops {sorted(where)[:8]}, "
                                         f"entry {[(entries[where[o]][0].hex(), entries[where[o]][1]) for o in bad[:2] if o in where]}")
                n_calls += 1
                n_rows += got.shape[0] * got.shape[1]
    print(f"\ntest_seams {kind} {pset} coop {coop}: {len(entries)} entries, {n_calls} calls, {n_rows} polynomials compared in "
          f"{time.time() - t0:.2f} s on {torch.cuda.get_device_name(0)}")
    assert n_calls == len(entries) + 2 * (3 * len(entries) + 1) and n_rows > 2 * 3 * len(entries) * COOP_RANGE // 2


# ------------------------------------------------------------------------------ key generation
def rare_keys(fx, pset):
    """(xi, 's' | 'a', polynomial index of the rare stream within the op's ExpandS / ExpandA) per key-level entry"""
    l = rc.SETS[pset]["l"]
    out = []
    if pset == 65:
        out += [(bytes.fromhex(e["xi"]), "s", e["streams"][0]["stream"]) for e in fx["es3_keys"] + fx["es_exact_keys"]]
    out += [(bytes.fromhex(e["xi"]), "a", e["r"] * l + e["s"]) for cat in ("ea_boundary", "ea_shape") for e in fx[cat][str(pset)]]
    return out


_key_cache = {}


def oracle_keys(pset, xis):
    """wire keys of the oracle, computed once per seed (16 threads for the large batches)"""
    new = sorted({x for x in xis if (pset, x) not in _key_cache})
    if new:
        pk, sk = orc.keygen_batch_mt(pset, new, 16)
        for x, a, b in zip(new, pk, sk):
            _key_cache[(pset, x)] = (a.tobytes(), b.tobytes())
    got = [_key_cache[(pset, x)] for x in xis]
    return np.frombuffer(b"".join(g[0] for g in got), dtype=np.uint8).reshape(len(xis), -1), \
        np.frombuffer(b"".join(g[1] for g in got), dtype=np.uint8).reshape(len(xis), -1)


_checked = {"keys": 0}


def check_keys(pset, xis, pk, sk, what):
    _checked["keys"] += len(xis)
    want_pk, want_sk = oracle_keys(pset, xis)
    pk, sk = np.asarray(pk), np.asarray(sk)
    bad = np.nonzero((pk != want_pk).any(axis=1) | (sk != want_sk).any(axis=1))[0]
    assert bad.size == 0, f"{what}: keys {bad[:8].tolist()} of {len(xis)} differ, first xi {xis[int(bad[0])].hex()}"


def keygen_batch(pset, keys, n_min, tag):
    """the seeds of a call of >= n_min keys: every rare key low, high, in the tail and in a crowd (see layouts), ordinary seeds between"""
    p = rc.SETS[pset]
    n = n_min
    while (n * (p["k"] + p["l"])) % 64 == 0 or (n * p["k"] * p["l"]) % 64 == 0:
        n += 1
    xis = [shake(tag, i) for i in range(n)]
    taken = set()
    for j, (xi, kind, r) in enumerate(keys):
        ppo = p["k"] * p["l"] if kind == "a" else p["k"] + p["l"]
        for high in (False, True):
            op = op_for_lane(ppo, r, n, high, taken)
            taken.add(op)
            xis[op] = xi
    free = [op for op in range(n - 1, -1, -1) if op not in taken]
    for j, (xi, _, _) in enumerate(keys):          # the end of the call, neighbouring ops: the tail wave and a crowd at once
        xis[free[j]] = xi
        taken.add(free[j])
    free = [op for op in range(1, n) if op not in taken]
    for j, (xi, _, _) in enumerate(keys):          # a crowd inside the call
        xis[free[j]] = xi
    return xis


def test_restated_keys_are_the_oracles(fx):
    """the chain of evidence on this machine too: restatement = oracle for every rare key (the padding keys are the oracle's alone)"""
    for pset in (44, 65, 87):
        for xi in sorted({k[0] for k in rare_keys(fx, pset)}):
            pk, sk = oracle_keys(pset, [xi])
            assert (pk[0].tobytes(), sk[0].tobytes()) == rc.keygen(pset, xi)


@pytest.mark.parametrize("coop", [0, 1])
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_keygen_routes(hp, sets, fx, pset, coop):
    """pk and sk bytes of the rare keys and of every padding key equal the oracle's on: the batch pipeline (MLDSA_OPT_SMALL_FUSED = 0)
    at 1 key, a few hundred keys and >= 8192 keys; the single-launch key generation (the default, <= 137 keys here); mldsa_keygen_host; the
    batcher -- each with MLDSA_OPT_COOP_HASH 0 and 1"""
    m = sets[pset]
    keys = rare_keys(fx, pset)
    assert len(keys) >= 24 and len({k[0] for k in keys}) >= 16
    t0, before, launched = time.time(), _checked["keys"], hp.stats()["direct_calls"]
    with options(hp, coop_hash=coop):
        with options(hp, small_fused=0):
            for xi, _, _ in keys:
                pk, sk = m.keygen_from_seed([xi])
                check_keys(pset, [xi], host(pk), host(sk), f"pipeline 1 key coop {coop}")
            for n_min in (70, 8192):
                xis = keygen_batch(pset, keys, max(n_min, 8 * len(keys) + 2), b"rare-pad-key%d-%d" % (pset, n_min))
                assert (len(xis) >= 8192) == (n_min == 8192)
                pk, sk = m.keygen_from_seed(xis)
                check_keys(pset, xis, host(pk), host(sk), f"pipeline {len(xis)} keys coop {coop}")
        # single launch: the limit is 256 * 30 / (k l) keys and needs the cooperative hashes; with them off the same calls take the pipeline
        limit = 256 * 30 // (rc.SETS[pset]["k"] * rc.SETS[pset]["l"])
        assert hp.get_option(_lib.OPT_SMALL_FUSED) == 256
        for lo in range(0, len(keys), 24):
            part = keys[lo:lo + 24]
            xis = keygen_batch(pset, part, 4 * len(part) + 2, b"rare-pad-small%d" % pset)
            assert len(xis) <= min(limit, 256)
            pk, sk = m.keygen_from_seed(xis)
            check_keys(pset, xis, host(pk), host(sk), f"single launch {len(xis)} keys coop {coop}")
        for xi, _, _ in keys:
            pk, sk = m.keygen_from_seed([xi])
            check_keys(pset, [xi], host(pk), host(sk), f"single launch 1 key coop {coop}")
        # host-memory entry point
        xis = keygen_batch(pset, keys, 4 * len(keys) + 2, b"rare-pad-host%d" % pset)
        pk, sk = m.keygen_host(np.frombuffer(b"".join(xis), dtype=np.uint8).reshape(-1, 32))
        check_keys(pset, xis, pk, sk, f"keygen_host coop {coop}")
        # the batcher's one-key calls
        b = MlDsaBatcher(pset, hotpath=hp, max_batch=64)
        try:
            for xi, _, _ in keys:
                pk, sk = b.keygen_from_seed(xi)
                want_pk, want_sk = oracle_keys(pset, [xi])
                assert pk == want_pk[0].tobytes() and sk == want_sk[0].tobytes(), (xi.hex(), coop)
        finally:
            b.close()
    launched = hp.stats()["direct_calls"] - launched
    print(f"\ntest_keygen_routes {pset} coop {coop}: {len(keys)} rare keys, {_checked['keys'] - before} keys compared, "
          f"{launched} direct op-level calls in {time.time() - t0:.2f} s")
    assert _checked["keys"] - before >= 8192 + 2 * len(keys)


# ------------------------------------------------------------------------------ signing and verification under the EA keys
_corpus = {}


def ea_corpus(fx, pset):
    """per distinct EA key: wire keys, oracle keys, a message, rnd, the oracle's signature and a bit-flipped twin"""
    if pset not in _corpus:
        _corpus[pset] = _ea_corpus(fx, pset)
    return _corpus[pset]


def _ea_corpus(fx, pset):
    xis = rc.ea_keys(fx, pset)
    pkb, skb = oracle_keys(pset, xis)
    out = dict(xi=xis, pk=pkb, sk=skb, msg=[], rnd=[], sig=[], bad=[], opk=[], osk=[])
    for i, xi in enumerate(xis):
        opk, osk = orc.keygen_from_seed(pset, xi)
        msg, rnd = shake(b"rare-msg%d" % pset, i, 10 + 7 * i), (shake(b"rare-rnd%d" % pset, i) if i % 3 else bytes(32))
        sig = orc.sign_internal(pset, osk, msg, rnd)
        twin = bytearray(sig)
        twin[(131 * i + 5) % len(sig)] ^= 1 << (i % 8)
        assert orc.verify_internal(pset, opk, msg, sig)
        for k, v in (("msg", msg), ("rnd", rnd), ("sig", sig), ("bad", bytes(twin)), ("opk", opk), ("osk", osk)):
            out[k].append(v)
    return out


@pytest.mark.parametrize("coop", [0, 1])
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_sign_under_ea_keys(hp, sets, fx, pset, coop):
    """A_hat is expanded again when a key signs: the small fused call, the batch pipeline, sign_cached_a with A_hat from the seam,
    sign_host and the batcher give the oracle's signatures"""
    m = sets[pset]
    c = ea_corpus(fx, pset)
    n = len(c["xi"])
    want = np.frombuffer(b"".join(c["sig"]), dtype=np.uint8).reshape(n, -1)
    with options(hp, coop_hash=coop):
        sks = m.private_keys_from_bytes(dev(c["sk"]))
        for fused in (256, 0):
            with options(hp, small_fused=fused):
                got = host(m.try_sign_with_seed(sks, c["msg"], c["rnd"], mode=MODE_INTERNAL))
                assert np.array_equal(got, want), (fused, np.nonzero((got != want).any(axis=1))[0])
                a_hat = m.expand_a_for_keys(sks)
                got = host(m._sign_batch(sks, c["msg"], c["rnd"], None, None,
                                         lambda mb, mo, rn, sg, k, cb, co, ki, st: m.sign_device(sks, mb, mo, rn, sg, k, cb, co, ki, MODE_INTERNAL, st,
                                                                                                 a_hat=a_hat)))
                assert np.array_equal(got, want), ("cached_a", fused)
        got = m.sign_host(c["sk"], c["msg"], np.frombuffer(b"".join(c["rnd"]), dtype=np.uint8).reshape(n, 32), mode=MODE_INTERNAL)
        assert np.array_equal(got, want)
        b = MlDsaBatcher(pset, hotpath=hp, max_batch=64)
        try:
            for i in range(n):
                assert b.sign(c["sk"][i].tobytes(), c["msg"][i], c["rnd"][i], mode=MODE_INTERNAL) == c["sig"][i], i
        finally:
            b.close()


@pytest.mark.parametrize("coop", [0, 1])
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verify_under_ea_keys(hp, sets, fx, pset, coop):
    """the oracle's signatures and their bit-flipped twins under the EA keys: the verdicts of orc.verify_internal (the untouched ones
    accepted) from mldsa_verify small fused and not, a batch of >= 8192 ops each with a key row of its own, verify_cached_a,
    verify_pk, verify_host, verify_pk_dedup on both routes and the batcher"""
    m = sets[pset]
    c = ea_corpus(fx, pset)
    nk = len(c["xi"])
    msgs, sigs, kidx = c["msg"] * 2, c["sig"] + c["bad"], np.tile(np.arange(nk, dtype=np.uint32), 2)
    want = np.array([orc.verify_internal(pset, c["opk"][k], mm, s) for k, mm, s in zip(kidx, msgs, sigs)])
    assert want[:nk].all() and not want[nk:].all()
    sg = dev(np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(2 * nk, -1))
    pkd = dev(c["pk"])
    with options(hp, coop_hash=coop):
        pks = m.public_keys_from_bytes(pkd)
        for fused in (256, 0):
            with options(hp, small_fused=fused):
                assert np.array_equal(m.verify(pks, msgs, sg, key_idx=kidx, mode=MODE_INTERNAL), want), fused
                a_hat = m.expand_a_for_keys(pks)
                got = m._verify_batch(pks, msgs, sg, None, kidx, lambda *a: m.verify_device(pks, *a, mode=MODE_INTERNAL, a_hat=a_hat))
                assert np.array_equal(got, want), ("cached_a", fused)
                assert np.array_equal(m.verify_pk(pkd, msgs, sg, key_idx=kidx, mode=MODE_INTERNAL), want), ("verify_pk", fused)
        assert np.array_equal(m.verify_host(c["pk"], msgs, host(sg), key_idx=kidx, mode=MODE_INTERNAL), want)
        # verify_pk_dedup: the table of distinct keys (cached route) and the plain route
        from fips204_amd.ml_dsa import _cat_with_offsets
        mb, mo = _cat_with_offsets(msgs, m.device)
        kd = torch.from_numpy(kidx.view(np.int32)).cuda()
        for cap, route in ((nk, "cached"), (nk - 1, "plain")):
            ok, info = torch.zeros(2 * nk, dtype=torch.uint8, device="cuda"), {}
            m.verify_pk_dedup_device(pkd, mb, mo, sg, ok, 2 * nk, None, None, kd, MODE_INTERNAL, max_cached_keys=cap, info=info)
            assert info == {"n_rows": nk, "route": route}
            assert np.array_equal(host(ok).astype(bool), want), route
        # >= 8192 ops, op i with key row i: ExpandA runs once per op in the large-batch form, the rare streams in many lanes
        n = 8192 + 2 * nk
        rep = np.arange(n) % (2 * nk)
        big_pk = pkd[torch.from_numpy(kidx[rep].astype(np.int64)).cuda()].contiguous()
        big_sg = sg[torch.from_numpy(rep).cuda()].contiguous()
        big_msgs = [msgs[i] for i in rep]
        assert np.array_equal(m.verify(m.public_keys_from_bytes(big_pk), big_msgs, big_sg, mode=MODE_INTERNAL), want[rep])
        assert np.array_equal(m.verify_pk(big_pk, big_msgs, big_sg, mode=MODE_INTERNAL), want[rep])
        for cap, route in ((nk, "cached"), (nk - 1, "plain")):
            mb, mo = _cat_with_offsets(big_msgs, m.device)
            ok, info = torch.zeros(n, dtype=torch.uint8, device="cuda"), {}
            m.verify_pk_dedup_device(big_pk, mb, mo, big_sg, ok, n, None, None, None, MODE_INTERNAL, max_cached_keys=cap, info=info)
            assert info == {"n_rows": nk, "route": route}
            assert np.array_equal(host(ok).astype(bool), want[rep]), route
        b = MlDsaBatcher(pset, hotpath=hp, max_batch=64)
        try:
            for i in range(2 * nk):
                assert b.verify(c["pk"][kidx[i]].tobytes(), msgs[i], sigs[i], mode=MODE_INTERNAL) == want[i], i
        finally:
            b.close()
