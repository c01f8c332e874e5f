"""Signing ops that outlast the rounds their call plans (plan_sign_compute, csrc/pipeline.hip), on every route that handles them: mldsa_sign
adds rounds, mldsa_sign_async reports MLDSA_ERR_AGAIN with a zero signature, mldsa_sign_host signs every such op again, one op per
mldsa_sign call (the loop at the end of csrc/host_api.hip) -- and mldsa_hash_sign_host, mldsa_sign_host_group, the batcher, mldsa_sign_seed
and mldsa_sign_mu sit on top of these.  Inputs and the oracle's iteration counts: tests/long_tail_cases.py; every assertion is byte equality
with the oracle's signature for every op the call signs, plus the statuses.

That the leg RAN is read from the library's own record (mldsa_get_stats), never inferred.  With MLDSA_OPT_GRAPHS off, run_op
(csrc/pipeline.hip) counts every mldsa_sign / _async / sign_call it launches in `direct_calls`: a mldsa_sign_host call of S sub-batches
that re-signs R ops moves it by S + R.  sign_chunk_finish counts in `sign_extra_rounds` the rounds a SYNCHRONOUS call adds after its one
look at the device, two at a time: the re-signed op's own mldsa_sign moves it when the op outlasts that call's plan as well.  With
MLDSA_OPT_SPEC_MAX = 1 and MLDSA_OPT_SIGN_ROUNDS = r every planned round tests one candidate per op and there are r of them (the plans
of 1 ... 261 ops at the stop thresholds 0.05 and 1e-9 all have at least 10 rounds of one candidate: one_op_plan_rounds), so the ops left
over are exactly {i : iterations[i] > r}, and a synchronous call of ops with at most `top` iterations adds 2 ceil((top - r) / 2) rounds.

Options and the sub-batch size are changed on a context of this module's own (`own`), restored in `finally`."""
import contextlib

from gpu_common import *  # noqa: F401,F403

import long_tail_cases as lt

pytestmark = pytest.mark.gpu

OPT_GRAPHS, OPT_SPEC_MAX, OPT_SIGN_ROUNDS, OPT_ASYNC_EXP = 1, 3, 6, 9
AGAIN, CTX_LEN = -5, -2
COUNTERS = ("direct_calls", "sign_extra_rounds", "graph_replays", "graphs_captured")


@pytest.fixture(scope="module")
def own():
    """{set: MlDsa} on a context of this module's own whose mldsa_sign_host calls cut their batches 64 ops before the end (261 = 197 + 64),
    MLDSA_OPT_GRAPHS off (its default, set all the same: every signing call is then one `direct_calls`)"""
    from fips204_amd.hotpath import HotPath
    from fips204_amd.ml_dsa import MlDsa
    env = {"MLDSA_TUNING_ENV": "1", "MLDSA_HOST_SUB_SIGN": "64"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = HotPath(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        h.set_option(OPT_GRAPHS, 0)
        assert (h.get_option(OPT_SPEC_MAX), h.get_option(OPT_SIGN_ROUNDS), h.get_option(OPT_ASYNC_EXP)) == (lt.SPEC_MAX_DEFAULT, 0, 9)
        yield {s: MlDsa(s, hotpath=h) for s in lt.SETS}
    finally:
        h.close()


@contextlib.contextmanager
def forced(set_option, rounds):
    """one candidate per op and round, `rounds` planned rounds"""
    set_option(OPT_SPEC_MAX, 1)
    set_option(OPT_SIGN_ROUNDS, rounds)
    try:
        yield
    finally:
        set_option(OPT_SIGN_ROUNDS, 0)
        set_option(OPT_SPEC_MAX, lt.SPEC_MAX_DEFAULT)


class Moved:
    """how far the context's counters moved inside the block"""

    def __init__(self, hp):
        self.hp = hp

    def __enter__(self):
        self.s0 = self.hp.stats()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        s1 = self.hp.stats()
        self.ms = (time.perf_counter() - self.t0) * 1e3
        for c in COUNTERS:
            setattr(self, c, s1[c] - self.s0[c])
        return False

    def __str__(self):
        return f"direct_calls +{self.direct_calls} sign_extra_rounds +{self.sign_extra_rounds} graph_replays +{self.graph_replays} {self.ms:.1f} ms"


def extra_rounds(iters, planned):
    """rounds of one candidate a synchronous call adds (two at a time) until the op with the most iterations has met its accepted one"""
    left = max(0, int(np.max(iters)) - planned)
    return 2 * -(-left // 2)


def one_op_plan_rounds(pset, forced_rounds):
    """planned rounds of a synchronous ONE-op call under SPEC_MAX = 1: plan_sign_compute adds rounds of one candidate while the expected
    number of unfinished ops, q^rounds with q = 1 - accept_prob(set) = 1 - 1 / 4.25 | 5.1 | 3.85, is above 0.05 -- 12 / 14 / 10 rounds --
    and SIGN_ROUNDS cuts the plan where it is longer"""
    import math
    q = 1.0 - 1.0 / {44: 4.25, 65: 5.1, 87: 3.85}[pset]
    return min(forced_rounds, math.ceil(math.log(0.05) / math.log(q)))


def no_secret_left(m):
    scanned, nonzero = m.hp.secret_residue()
    assert scanned > 0 and nonzero == 0, f"{nonzero} non-zero bytes of {scanned} left behind"


def mem(a, pinned, keep):
    """a private copy of `a` in pageable or in page-locked host memory"""
    a = np.ascontiguousarray(a)
    if not pinned:
        return a.copy()
    t = torch.empty(max(a.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    keep.append(t)
    v = t.numpy()[:a.nbytes].view(a.dtype).reshape(a.shape)
    v[...] = a
    return v


def sign_host_raw(m, v, pinned=False, with_status=True, null_msgs=False, fn=None, handle=None, mode=0):
    """mldsa_sign_host itself (the Python mirror always passes msgs and status): -> (rc, sig [n, SIG_LEN], status [n] or None).  v: a
    long_tail_cases.variant(); msgs = NULL needs every message empty; ctxs = None passes ctxs = ctx_off = NULL.  Outputs start stale."""
    keep, n = [], len(v["msgs"])
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)
    sk = mem(v["sk"], pinned, keep)
    kidx = mem(v["kidx"], pinned, keep) if v["kidx"] is not None else None
    mflat, moff = m._cat_host(v["msgs"])
    if null_msgs:
        assert not moff.any()
        mflat = None
    else:
        mflat = mem(mflat, pinned, keep)
    moff = mem(moff, pinned, keep)
    cflat = coff = None
    if v["ctxs"] is not None:
        cflat, coff = m._cat_host(v["ctxs"])
        cflat, coff = mem(cflat, pinned, keep), mem(coff, pinned, keep)
    rnd = mem(np.frombuffer(b"".join(v["rnd"]), dtype=np.uint8).reshape(n, 32), pinned, keep)
    sig = mem(np.full((n, m.SIG_LEN), 0xA5, dtype=np.uint8), pinned, keep)
    st = mem(np.full(n, -7, dtype=np.int32), pinned, keep) if with_status else None
    rc = (fn or m.lib.mldsa_sign_host)(handle or m.hp._h, m.pset, mode, vp(sk), len(sk), vp(kidx), vp(mflat), vp(moff), vp(cflat), vp(coff), vp(rnd),
                                       vp(sig), vp(st), n)
    return rc, np.array(sig), (np.array(st) if with_status else None)


def batch_ops(pset, ops):
    """ops of the long-tail batch as a variant-shaped dict under the batch's one key (key_idx all 0), with the oracle's word on them"""
    ops = [int(i) for i in ops]
    got = [lt.oracle_sig(pset, i) for i in ops]
    return dict(sk=np.frombuffer(lt.key(pset)[3], dtype=np.uint8).reshape(1, -1), kidx=np.zeros(len(ops), dtype=np.uint32),
                msgs=[lt.message(pset, i) for i in ops], ctxs=None, rnd=[lt.rnd(pset, i) for i in ops],
                sig=np.stack([np.frombuffer(s, dtype=np.uint8) for s, _ in got]), iters=np.array([it for _, it in got], dtype=np.int32))


def on_device(m, v):
    """the device-resident arguments of a variant-shaped dict: (PrivateKeys, msg_buf, msg_off, ctx_buf, ctx_off, rnd, key_idx, sigs, status)"""
    from fips204_amd.ml_dsa import _cat_with_offsets
    n = len(v["msgs"])
    sks = m.private_keys_from_bytes(dev(v["sk"]))
    mb, mo = _cat_with_offsets(v["msgs"], m.device)
    cb, co = _cat_with_offsets(v["ctxs"], m.device) if v["ctxs"] is not None else (None, None)
    rn = dev(np.frombuffer(b"".join(v["rnd"]), dtype=np.uint8).reshape(n, 32))
    kidx = dev(v["kidx"].view(np.int32)) if v["kidx"] is not None else None
    sig = torch.full((n, m.SIG_LEN), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    return sks, mb, mo, cb, co, rn, kidx, sig, st


def short_neighbour(pset, op):
    """the first op after `op` that a one-op call finishes in its first round whatever the plan gives it (at most 8 iterations)"""
    i = op + 1
    while lt.oracle_sig(pset, i)[1] > 8:
        i += 1
    return i


# ------------------------------------------------------------------------------ default options: calls of one op
@pytest.mark.parametrize("pset", lt.SETS)
def test_one_op_sign_adds_rounds(own, pset):
    """mldsa_sign of ONE op with more than 32 iterations (every such op of the set's batch: 1 / 14 / 2), default options: a call of one
    op plans one round of at most MLDSA_OPT_SPEC_MAX = 32 candidates (q^19 < 0.05 already), so the op outlasts it and
    sign_chunk_finish adds rounds -- `sign_extra_rounds` moves by an even number >= 2, `direct_calls` by 1; status 0 and the oracle's
    bytes.  Control: a neighbour with at most 8 iterations moves `sign_extra_rounds` by 0."""
    m = own[pset]
    ops, its = lt.long_ops(pset, lt.SPEC_MAX_DEFAULT)
    assert len(ops) >= 1
    for op, it in list(zip(ops, its)) + [(short_neighbour(pset, int(ops[0])), 0)]:
        v = batch_ops(pset, [op])
        sks, mb, mo, _, _, rn, kidx, sig, st = on_device(m, v)
        with Moved(m.hp) as mv:
            m.sign_device(sks, mb, mo, rn, sig, 1, key_idx=kidx, status=st)
        print(f"ML-DSA-{pset} op {op} ({v['iters'][0]} iterations): mldsa_sign {mv}")
        assert np.array_equal(host(sig), v["sig"]) and host(st)[0] == 0, op
        assert mv.direct_calls == 1
        if it:
            assert v["iters"][0] == it and mv.sign_extra_rounds >= 2 and mv.sign_extra_rounds % 2 == 0, (op, str(mv))
        else:
            assert mv.sign_extra_rounds == 0, (op, str(mv))


@pytest.mark.parametrize("pset", lt.SETS)
def test_one_op_sign_async_reports_again_and_zeroes_the_signature(own, pset):
    """mldsa_sign_async of one op with more than 32 iterations.  With the plan mldsa_sign_host gives its calls -- stop planning at 0.1
    expected unfinished ops, MLDSA_OPT_SIGN_ASYNC_EXP = 1 (the host path passes 0.05: the same single round for one op) -- the op is
    left: status -5 and an all-zero signature over stale bytes; the same op through mldsa_sign then gives the oracle's bytes.
    At the DEFAULT exponent, 9, a one-op call plans rounds until q^candidates < 1e-9: at least 76 candidates for every set
    (ln 1e-9 / ln q = 77 / 95 / 69 for ML-DSA-44 / 65 / 87 and whole rounds), more than the 50 / 47 / 36 iterations of the longest
    op, so there the asynchronous call FINISHES the op: status 0, the oracle's bytes."""
    m = own[pset]
    ops, _ = lt.long_ops(pset, lt.SPEC_MAX_DEFAULT)
    for op in ops:
        v = batch_ops(pset, [op])
        sks, mb, mo, _, _, rn, kidx, sig, st = on_device(m, v)
        m.sign_device(sks, mb, mo, rn, sig, 1, key_idx=kidx, status=st, wait=False)
        assert host(st)[0] == 0 and np.array_equal(host(sig), v["sig"]), (op, "default exponent")
        m.hp.set_option(OPT_ASYNC_EXP, 1)
        try:
            sig.fill_(0xA5)
            st.fill_(-7)
            with Moved(m.hp) as mv:
                m.sign_device(sks, mb, mo, rn, sig, 1, key_idx=kidx, status=st, wait=False)
                got_sig, got_st = host(sig).copy(), host(st).copy()
            assert got_st[0] == AGAIN and not got_sig.any(), (op, got_st)
            assert mv.direct_calls == 1 and mv.sign_extra_rounds == 0
            with Moved(m.hp) as mv2:
                m.sign_device(sks, mb, mo, rn, sig, 1, key_idx=kidx, status=st)
            assert host(st)[0] == 0 and np.array_equal(host(sig), v["sig"]) and mv2.sign_extra_rounds >= 2, op
        finally:
            m.hp.set_option(OPT_ASYNC_EXP, 9)


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("pset", lt.SETS)
def test_one_op_sign_host_signs_the_left_over_op_again(own, pset, pinned):
    """mldsa_sign_host of one op with more than 32 iterations, every buffer pageable / every buffer page-locked (a one-op call is below
    the 16 385 ops of the round-by-round export: page-locked memory changes the copies -- DMA from and into the caller's arrays, no
    bounce buffers -- not the path).  The asynchronous sub-batch leaves the op (status -5 inside the call), the leg signs it again:
    RE-SIGNED OPS = 1, proven by `direct_calls` + 2 (one sub-batch, one mldsa_sign) and by `sign_extra_rounds` >= 2 (that mldsa_sign
    plans the same single round); status 0, the oracle's bytes, nothing secret left.  Control: a short neighbour -- `direct_calls` + 1."""
    m = own[pset]
    ops, _ = lt.long_ops(pset, lt.SPEC_MAX_DEFAULT)
    for op in list(ops) + [short_neighbour(pset, int(ops[0]))]:
        v = batch_ops(pset, [op])
        long_op = v["iters"][0] > lt.SPEC_MAX_DEFAULT
        with Moved(m.hp) as mv:
            rc, sig, st = sign_host_raw(m, v, pinned=pinned)
        no_secret_left(m)
        print(f"ML-DSA-{pset} op {op} ({v['iters'][0]} iterations) pinned={pinned}: mldsa_sign_host re-signed {mv.direct_calls - 1}; {mv}")
        assert rc == 0 and st[0] == 0 and np.array_equal(sig, v["sig"]), op
        assert mv.direct_calls == (2 if long_op else 1), (op, str(mv))
        assert mv.sign_extra_rounds >= 2 if long_op else mv.sign_extra_rounds == 0, (op, str(mv))


@pytest.mark.parametrize("pset", lt.SETS)
def test_host_call_of_64_ops_with_the_longest_op_in_the_middle(own, pset):
    """64 consecutive ops of the batch around its longest op (50 / 47 / 36 iterations), default options.  A call of this shape plans
    two rounds -- by the plan's own arithmetic 16 + 32 candidates for ML-DSA-44, 12 + 32 for ML-DSA-65, 19 + 32 for ML-DSA-87 -- which
    may or may not reach the op, so the leg is not REQUIRED here: every byte is the oracle's and every status 0; the number of re-signed
    ops is read from `direct_calls` and printed.  Measured on an MI355X: 1 / 1 / 0 -- the 48 and 44 candidates do not reach the 50- and
    47-iteration ops and the leg signs them again, 51 candidates reach ML-DSA-87's 36."""
    m = own[pset]
    ops, its = lt.long_ops(pset)
    mid = int(ops[int(np.argmax(its))])
    v = batch_ops(pset, range(mid - 32, mid + 32))
    assert v["iters"][32] == its.max()
    with Moved(m.hp) as mv:
        rc, sig, st = sign_host_raw(m, v)
    no_secret_left(m)
    print(f"ML-DSA-{pset} ops {mid - 32} ... {mid + 31}, longest {its.max()}: mldsa_sign_host re-signed {mv.direct_calls - 1}; {mv}")
    assert rc == 0 and not st.any() and np.array_equal(sig, v["sig"]), np.nonzero((sig != v["sig"]).any(axis=1))[0]
    assert mv.direct_calls - 1 in (0, 1)


# ------------------------------------------------------------------------------ forced: one candidate per round, r planned rounds
@pytest.mark.parametrize("rounds", [1, 2])
def test_forced_async_leaves_exactly_the_ops_above_r_iterations(own, rounds):
    """mldsa_sign_async, the first 261 ops of the ML-DSA-44 batch, SPEC_MAX = 1 and SIGN_ROUNDS = r: the statuses -5 are EXACTLY
    {i : iterations[i] > r} (one candidate per op and round whatever the count -- spec_of() is capped by SPEC_MAX -- and the plan of 261
    ops at 1e-9 has far more than 2 rounds to cut); those rows are zero, every other row is the oracle's with status 0."""
    m = own[44]
    v = batch_ops(44, range(lt.N_FORCED))
    want = lt.unfinished_after(v["iters"], rounds)
    sks, mb, mo, _, _, rn, kidx, sig, st = on_device(m, v)
    with forced(m.hp.set_option, rounds):
        with Moved(m.hp) as mv:
            m.sign_device(sks, mb, mo, rn, sig, lt.N_FORCED, key_idx=kidx, status=st, wait=False)
            got_sig, got_st = host(sig).copy(), host(st).copy()
    print(f"r = {rounds}: {want.sum()} of {lt.N_FORCED} ops left; {mv}")
    assert 0 < want.sum() < lt.N_FORCED
    assert np.array_equal(got_st == AGAIN, want), np.nonzero((got_st == AGAIN) != want)[0]
    assert not got_st[~want].any() and not got_sig[want].any() and np.array_equal(got_sig[~want], v["sig"][~want])
    assert mv.direct_calls == 1 and mv.sign_extra_rounds == 0


# (key_idx over 6 keys | op i under key i, ctxs of 0 ... 8 bytes | ctxs = ctx_off = NULL, msgs = NULL with every message empty, status given | NULL,
#  pageable | page-locked): every value of every argument, and every pair of the pointer arguments the leg indexes (key_idx x ctx_off x msgs)
HOST_VARIANTS = {
    "kidx-ctx-msgs-status-pageable": dict(with_kidx=True, with_ctx=True, null_msgs=False, with_status=True, pinned=False),
    "kidx-ctx-msgs-nostatus-pinned": dict(with_kidx=True, with_ctx=True, null_msgs=False, with_status=False, pinned=True),
    "kidx-noctx-nomsgs-status-pinned": dict(with_kidx=True, with_ctx=False, null_msgs=True, with_status=True, pinned=True),
    "kidx-ctx-nomsgs-nostatus-pageable": dict(with_kidx=True, with_ctx=True, null_msgs=True, with_status=False, pinned=False),
    "nokidx-ctx-msgs-status-pinned": dict(with_kidx=False, with_ctx=True, null_msgs=False, with_status=True, pinned=True),
    "nokidx-noctx-msgs-nostatus-pageable": dict(with_kidx=False, with_ctx=False, null_msgs=False, with_status=False, pinned=False),
    "nokidx-ctx-nomsgs-status-pageable": dict(with_kidx=False, with_ctx=True, null_msgs=True, with_status=True, pinned=False),
    "nokidx-noctx-nomsgs-nostatus-pinned": dict(with_kidx=False, with_ctx=False, null_msgs=True, with_status=False, pinned=True),
}


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("name", list(HOST_VARIANTS))
def test_forced_host_call_signs_every_left_over_op_again(own, name, rounds):
    """mldsa_sign_host, ML-DSA-44, 261 ops cut 197 + 64, SPEC_MAX = 1 and SIGN_ROUNDS = r: both sub-batches leave {i : iterations[i] >
    r} -- about 200 / 150 of the 261 ops, in both sub-batches, op 0 and op 260 among them in most variants -- and the leg signs each of
    them again from slot 0's buffers: two-entry offset tables, the key table indexed by key_idx[op] or by op, one signature and one
    status copied back.  Per variant (see HOST_VARIANTS): rc 0, every byte the oracle's, every status 0 (where the caller passes
    one), nothing secret left, and RE-SIGNED OPS = the predicted count, proven twice: `direct_calls` moves by 2 + count, and
    `sign_extra_rounds` by the sum over the re-signed ops of 2 ceil((iterations - r) / 2) (each one's mldsa_sign plans r rounds too)."""
    m, o = own[44], HOST_VARIANTS[name]
    v = lt.variant(44, lt.N_FORCED, o["with_kidx"], o["with_ctx"], o["null_msgs"])
    left = lt.unfinished_after(v["iters"], rounds)
    with forced(m.hp.set_option, rounds):
        with Moved(m.hp) as mv:
            rc, sig, st = sign_host_raw(m, v, pinned=o["pinned"], with_status=o["with_status"], null_msgs=o["null_msgs"])
        no_secret_left(m)
    print(f"{name} r = {rounds}: predicted {left.sum()} re-signed ops ({left[:197].sum()} + {left[197:].sum()}), counted {mv.direct_calls - 2}; {mv}")
    assert left[:197].any() and left[197:].any() and not left.all()
    assert rc == 0 and (st is None or not st.any())
    assert np.array_equal(sig, v["sig"]), np.nonzero((sig != v["sig"]).any(axis=1))[0]
    assert mv.direct_calls - 2 == left.sum(), str(mv)
    assert mv.sign_extra_rounds == sum(extra_rounds(it, rounds) for it in v["iters"][left]), str(mv)


@pytest.mark.parametrize("pinned", [False, True])
def test_forced_host_call_refuses_an_over_long_ctx_and_still_signs_the_left_over_ops(own, pinned):
    """An over-long ctx at ops 1 and 197 (first sub-batch, first op of the second) together with unfinished ops, r = 2.  A refused op is
    a per-op status: the signing calls return MLDSA_OK, so the leg is NOT skipped (it is only for a failed call) -- the call re-signs
    the other left-over ops and returns 0 with status -2 and zero rows at ops 1 and 197; every other row is the oracle's.  `direct_calls`
    moves by 2 + the predicted count over the ops that are not refused."""
    m = own[44]
    v = dict(lt.variant(44, lt.N_FORCED, True, True, False))
    bad = [1, 197]
    v["ctxs"] = [b"z" * 256 if i in bad else c for i, c in enumerate(v["ctxs"])]
    good = np.ones(lt.N_FORCED, dtype=bool)
    good[bad] = False
    left = lt.unfinished_after(v["iters"], 2) & good
    with forced(m.hp.set_option, 2):
        with Moved(m.hp) as mv:
            rc, sig, st = sign_host_raw(m, v, pinned=pinned)
        no_secret_left(m)
    print(f"over-long ctx, pinned={pinned}: predicted {left.sum()} re-signed ops, counted {mv.direct_calls - 2}; {mv}")
    assert rc == 0 and (st[bad] == CTX_LEN).all() and not st[good].any()
    assert not sig[bad].any() and np.array_equal(sig[good], v["sig"][good])
    assert mv.direct_calls - 2 == left.sum(), str(mv)
    with pytest.raises(ValueError):  # the mirror turns the statuses into the reference's error (lib.rs:274)
        with forced(m.hp.set_option, 2):
            m.sign_host(v["sk"], v["msgs"], np.frombuffer(b"".join(v["rnd"]), dtype=np.uint8), ctxs=v["ctxs"], key_idx=v["kidx"])


@pytest.mark.parametrize("pset", [65, 87])
def test_forced_host_call_of_the_larger_sets(own, pset):
    """ML-DSA-65 / 87, 64 ops in one sub-batch with key_idx over 6 keys and ctxs of 0 ... 8 bytes, r = 2: as the ML-DSA-44 cases"""
    m = own[pset]
    v = lt.variant(pset, 64, True, True, False)
    left = lt.unfinished_after(v["iters"], 2)
    with forced(m.hp.set_option, 2):
        with Moved(m.hp) as mv:
            rc, sig, st = sign_host_raw(m, v)
        no_secret_left(m)
    print(f"ML-DSA-{pset}: predicted {left.sum()} re-signed ops, counted {mv.direct_calls - 1}; {mv}")
    assert 0 < left.sum() < 64
    assert rc == 0 and not st.any() and np.array_equal(sig, v["sig"])
    assert mv.direct_calls - 1 == left.sum() and mv.sign_extra_rounds == sum(extra_rounds(it, 2) for it in v["iters"][left]), str(mv)


def test_forced_direct_path_signs_the_left_over_ops_again(own):
    """The round-by-round export (page-locked signatures, more than 16 384 ops: ONE signing call for the whole batch, finished
    signatures stored into the caller's array by the device, slot 0 holding the whole call's inputs) and the leg behind it.  ML-DSA-44,
    16 500 ops -- the batch and its first 116 ops once more -- SPEC_MAX = 1 and SIGN_ROUNDS = 30 (the plan of 16 500 ops at 0.05 has
    ln(16 500 / 0.05) / ln(1 / q) = 47 rounds of one candidate to cut): the ops above 30 iterations get a zero row and status -5 from
    the call and are signed again.  Every byte the oracle's, every status 0, nothing secret left; RE-SIGNED OPS = the predicted count:
    `direct_calls` moves by 1 + count (the sub-batch path of this context would make it 2 + count: 16 436 + 64) while
    `sign_extra_rounds` moves by the re-signed ops' own 2 ceil((iterations - 12) / 2): a one-op mldsa_sign plans 12 rounds of one
    candidate here (one_op_plan_rounds), fewer than the 30 it may have."""
    m, n, r = own[44], 16500, 30
    sigs, iters, _ = lt.traced(44)
    ops = np.concatenate([np.arange(lt.N_BATCH), np.arange(n - lt.N_BATCH)])
    v = dict(sk=np.frombuffer(lt.key(44)[3], dtype=np.uint8).reshape(1, -1), kidx=np.zeros(n, dtype=np.uint32),
             msgs=[lt.message(44, i) for i in ops], ctxs=None, rnd=[lt.rnd(44, i) for i in ops])
    want, it = sigs[ops], iters[ops]
    left = lt.unfinished_after(it, r)
    assert np.array_equal(np.nonzero(left)[0], lt.long_ops(44, r)[0]) and left.sum() >= 1  # (none of them among the first 116)
    with forced(m.hp.set_option, r):
        with Moved(m.hp) as mv:
            rc, sig, st = sign_host_raw(m, v, pinned=True)
        no_secret_left(m)
    print(f"direct path, r = {r}: predicted {left.sum()} re-signed ops, counted {mv.direct_calls - 1}; {mv}")
    assert rc == 0 and not st.any()
    assert np.array_equal(sig, want), np.nonzero((sig != want).any(axis=1))[0]
    assert one_op_plan_rounds(44, r) == 12
    assert mv.sign_extra_rounds == sum(extra_rounds(i, 12) for i in it[left]) and mv.direct_calls == 1 + left.sum(), str(mv)


# ------------------------------------------------------------------------------ routes on top (forced, 64 ops, ML-DSA-65)
def test_hash_sign_host_on_top_of_the_leg(own):
    """mldsa_hash_sign_host (SHA-512 on the device, then mldsa_sign_host in pre-hash mode on the same context), r = 2: the oracle's
    HashML-DSA signatures of the same inputs, whose own iteration counts predict the re-signed ops -- `direct_calls` + 1 + count."""
    m = own[65]
    v = lt.variant(65, 64, True, True, False, ph="SHA512")
    left = lt.unfinished_after(v["iters"], 2)
    sig, st = np.full((64, m.SIG_LEN), 0xA5, dtype=np.uint8), np.full(64, -7, dtype=np.int32)
    with forced(m.hp.set_option, 2):
        with Moved(m.hp) as mv:
            m.hash_sign_host(v["sk"], v["msgs"], np.frombuffer(b"".join(v["rnd"]), dtype=np.uint8), ctxs=v["ctxs"], ph="SHA512", key_idx=v["kidx"],
                             out=(sig, st))
        no_secret_left(m)
    print(f"hash_sign_host: predicted {left.sum()} re-signed ops, counted {mv.direct_calls - 1}; {mv}")
    assert 0 < left.sum() < 64 and not st.any() and np.array_equal(sig, v["sig"])
    assert mv.direct_calls - 1 == left.sum(), str(mv)


def test_sign_host_group_on_top_of_the_leg():
    """mldsa_sign_host_group over three contexts on GPU 0 (slices of 22, 22 and 20 ops, each its own mldsa_sign_host with key_idx + a,
    ctx_off + a, status + a), r = 2 on every context: the oracle's bytes, statuses 0, and per context `direct_calls` + 1 + the predicted
    count of ITS slice."""
    from fips204_amd.hotpath import HotPath
    from fips204_amd.ml_dsa import MlDsaGroup
    devices = [0, 0, 0]
    g = MlDsaGroup(65, devices)
    try:
        v = lt.variant(65, 64, True, True, False)
        left = lt.unfinished_after(v["iters"], 2)
        hps = [HotPath.from_handle(g.ctx(i), 0) for i in range(len(g))]
        with forced(g.set_option, 2):
            g.set_option(OPT_GRAPHS, 0)
            s0 = [h.stats() for h in hps]
            rc, sig, st = sign_host_raw(g, v, fn=g.lib.mldsa_sign_host_group, handle=g._g)
            s1 = [h.stats() for h in hps]
            assert all(h.secret_residue()[1] == 0 for h in hps)
        assert rc == 0 and not st.any() and np.array_equal(sig, v["sig"])
        for i in range(len(g)):
            a, c = g.shard(64, i)
            moved = s1[i]["direct_calls"] - s0[i]["direct_calls"]
            print(f"group context {i}: ops {a} ... {a + c - 1}, predicted {left[a:a + c].sum()} re-signed ops, counted {moved - 1}")
            assert c > 0 and moved - 1 == left[a:a + c].sum(), i
    finally:
        g.close()


def test_sign_group_without_waiting_reports_the_left_over_ops():
    """mldsa_sign_group(wait = 0) signs each device-resident slice with mldsa_sign_async: r = 2, the statuses -5 are exactly the
    predicted ops of each slice, zero rows there, the oracle's bytes elsewhere; with wait = 1 (mldsa_sign) every op is the oracle's
    and each context's `sign_extra_rounds` moves by what its slice's longest op needs."""
    from fips204_amd.hotpath import HotPath
    from fips204_amd.ml_dsa import MlDsaGroup
    g = MlDsaGroup(65, [0, 0, 0])
    try:
        v = lt.variant(65, 64, True, True, False)
        left = lt.unfinished_after(v["iters"], 2)
        slices, parts = [], []
        for i in range(len(g)):
            a, c = g.shard(64, i)
            vi = dict(v, kidx=v["kidx"][a:a + c], msgs=v["msgs"][a:a + c], ctxs=v["ctxs"][a:a + c], rnd=v["rnd"][a:a + c])
            sks, mb, mo, cb, co, rn, kidx, sig, st = on_device(g.on_device(i), vi)
            slices.append(dict(sks=sks, msg_buf=mb, msg_off=mo, ctx_buf=cb, ctx_off=co, rnd=rn, key_idx=kidx, sigs=sig, status=st, n_ops=c))
            parts.append((a, c))
        torch.cuda.synchronize()
        hps = [HotPath.from_handle(g.ctx(i), 0) for i in range(len(g))]
        with forced(g.set_option, 2):
            g.sign_group(slices, wait=False)
            g.sync()
            got_sig = np.concatenate([host(s["sigs"]) for s in slices])
            got_st = np.concatenate([host(s["status"]) for s in slices])
            assert np.array_equal(got_st == AGAIN, left) and not got_st[~left].any(), got_st
            assert not got_sig[left].any() and np.array_equal(got_sig[~left], v["sig"][~left])
            s0 = [h.stats() for h in hps]
            g.sign_group(slices, wait=True)
            s1 = [h.stats() for h in hps]
        assert np.array_equal(np.concatenate([host(s["sigs"]) for s in slices]), v["sig"])
        assert not np.concatenate([host(s["status"]) for s in slices]).any()
        for i, (a, c) in enumerate(parts):
            assert s1[i]["sign_extra_rounds"] - s0[i]["sign_extra_rounds"] == extra_rounds(v["iters"][a:a + c], 2), i
    finally:
        g.close()


def test_batcher_signs_a_long_op(own):
    """One single-op signature through the batcher (mldsa_sign_cached_a, synchronous, a batch of one) of the longest ML-DSA-65 op of
    the batch, default options: the oracle's bytes, and the context's `sign_extra_rounds` moved (>= 2)."""
    from fips204_amd.ml_dsa import MlDsaBatcher
    m = own[65]
    ops, its = lt.long_ops(65, lt.SPEC_MAX_DEFAULT)
    op = int(ops[int(np.argmax(its))])
    b = MlDsaBatcher(65, hotpath=m.hp, max_batch=4)
    try:
        with Moved(m.hp) as mv:
            sig = b.sign(lt.key(65)[3], lt.message(65, op), lt.rnd(65, op))
        print(f"batcher, op {op} ({its.max()} iterations): {mv}")
        assert sig == lt.oracle_sig(65, op)[0]
        assert mv.sign_extra_rounds >= 2 and mv.sign_extra_rounds % 2 == 0, str(mv)
    finally:
        b.close()


def test_sign_from_seeds_on_top_of_the_extra_rounds(own):
    """mldsa_sign_seed (the keys expanded from their seeds into the scratch, then mldsa_sign), 64 ops with key_idx and ctxs, r = 2: the
    oracle's bytes, and `sign_extra_rounds` moves by 2 ceil((longest - 2) / 2)."""
    m = own[65]
    v = lt.variant(65, 64, True, True, False)
    _, mb, mo, cb, co, rn, kidx, sig, st = on_device(m, v)
    xi = dev(np.frombuffer(b"".join(lt.op_key_seed(65, i) for i in range(lt.NK_FORCED)), dtype=np.uint8).reshape(lt.NK_FORCED, 32))
    with forced(m.hp.set_option, 2):
        with Moved(m.hp) as mv:
            m.sign_from_seeds_device(xi, mb, mo, rn, sig, 64, ctx_buf=cb, ctx_off=co, key_idx=kidx, status=st)
    print(f"sign_from_seeds_device: longest op {v['iters'].max()} iterations; {mv}")
    assert np.array_equal(host(sig), v["sig"]) and not host(st).any()
    assert mv.sign_extra_rounds == extra_rounds(v["iters"], 2) > 0, str(mv)


# ------------------------------------------------------------------------------ mldsa_sign_mu: its own loop
@pytest.mark.parametrize("pset", lt.SETS)
def test_sign_mu_on_the_ops_above_25_iterations(own, pset):
    """mldsa_sign_mu, default options, 64 ops: the batch's ops above 25 iterations (26 / the longest 64 of 82 / 8) padded with their
    neighbours.  Its loop tests one candidate per live op and round, looks at the device after each and compacts the rows whenever
    half of them are done -- down to one row, for 50 / 47 / 36 rounds here, more compactions than any other case runs.  The oracle's
    bytes (mu computed on the host from tr = H(pk, 64) and the message, pure mode, empty ctx)."""
    from fips204_amd.ml_dsa import external_mu
    m = own[pset]
    ops = lt.padded(pset)
    v = batch_ops(pset, ops)
    assert (v["iters"] > lt.LONG).sum() >= 8 and v["iters"].max() > lt.SPEC_MAX_DEFAULT
    tr = hashlib.shake_256(lt.key(pset)[2]).digest(64)
    sks, _, _, _, _, rn, kidx, sig, st = on_device(m, v)
    mu = dev(np.frombuffer(b"".join(external_mu(tr, msg) for msg in v["msgs"]), dtype=np.uint8).reshape(64, 64))
    t0 = time.perf_counter()
    m.sign_mu_device(sks, mu, rn, sig, 64, key_idx=kidx, status=st)
    got = host(sig)
    print(f"ML-DSA-{pset} sign_mu_device: {(v['iters'] > lt.LONG).sum()} ops above 25 iterations, longest {v['iters'].max()}, {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert np.array_equal(got, v["sig"]), np.nonzero((got != v["sig"]).any(axis=1))[0]
    assert not host(st).any()
