"""Incremental mu on the device and mu from host memory (include/mldsa_mus.h): mldsa_mus_init / _update / _final against hashlib fed the
same pieces and against mldsa_mu_compute on the whole messages, in both kernel forms; refusals per op; the compositions with
mldsa_verify_mu / mldsa_sign_mu; mldsa_mus_host_compute against the core's host-memory calls.  mu is compared byte for byte."""
from gpu_common import *  # noqa: F401,F403
from gpu_common import C, dev, dev_off, hashlib, host, kidx_dev, np, orc, pytest, torch

import mus_cases
from conftest import PSET
from fips204_amd import _lib, _mus_lib, _ph_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PREHASH, MODE_PURE, MlDsa, PublicKeys, _cat_with_offsets, external_mu
from mus_cases import HOST_LENS, hashlib_incremental, pieces_of

pytestmark = pytest.mark.gpu

NULL = C.c_void_p(0)
MODES = (MODE_PURE, MODE_INTERNAL, MODE_PREHASH)
WAVE_MAX = _mus_lib.wave_max_ops()
# the lane-form leg pads the batch with copies of its first op to this many ops more than the threshold; not run when the macro is 0
# (the natural n runs in the lane form already) or so large that the padding would be
PAD_LEG = 0 < WAVE_MAX <= 65536
N_KEYS = 7


@pytest.fixture(scope="module")
def trs(sets):
    """tr of 7 generated keys: (device tensor [7, 64], list of 7 byte strings)"""
    m = sets[44]
    pk, _ = m.keygen_from_seed([hashlib.sha256(b"mus-key" + bytes([j])).digest() for j in range(N_KEYS)])
    tr = m.public_keys_from_bytes(pk).tr.clone()
    return tr, [r.tobytes() for r in host(tr)]


def packed(items, pad, shift):
    """(flat uint8, uint64 offsets): the byte strings back to back from byte `shift` on, then `pad` copies of the first"""
    lens = np.array([len(b) for b in items] + [len(items[0])] * pad, dtype=np.uint64)
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    off += np.uint64(shift)
    return np.frombuffer(bytes(shift) + b"".join(items) + items[0] * pad + bytes(8), dtype=np.uint8), off


_CASES = {}


def case_set(m, mode, trs):
    """the operations of a mode, their schedules and, computed once, mldsa_mu_compute's rows on the whole messages"""
    if mode not in _CASES:
        ops = mus_cases.cases(mode)
        sched = mus_cases.schedules(ops, mode)
        for name, count in mus_cases.coverage(ops, sched, mode).items():
            assert count > 0, name
        n = len(ops)
        kidx = np.arange(n, dtype=np.uint32) % N_KEYS
        mb, mo = _cat_with_offsets([x for _, x in ops], m.device)
        cb, co = _cat_with_offsets([c for c, _ in ops], m.device)
        mu, flag = m.mu_device(trs[0], mb, mo, n, cb, co, kidx_dev(kidx), mode)
        whole = [r.tobytes() for r in host(mu)]
        assert not host(flag).any()
        op_tr = [trs[1][i % N_KEYS] for i in range(n)]
        assert whole == [external_mu(op_tr[i], x, c, mode) for i, (c, x) in enumerate(ops)]
        _CASES[mode] = dict(ops=ops, sched=sched, whole=whole, op_tr=op_tr)
    return _CASES[mode]


def stream(m, mode, tr_d, ops, idx, cuts, pad=0, upto=None, keep=None):
    """ops idx of `ops` streamed by their cuts through a MuStream (keep: an open one to go on with): (stream, mu, flag) of the first
    len(idx) ops; the pieces of update u lie at byte u % 4 of their buffer"""
    n = len(idx)
    s, first = keep if keep else (None, 0)
    if s is None:
        kidx = np.array([i % N_KEYS for i in idx] + [idx[0] % N_KEYS] * pad, dtype=np.uint32)
        cflat, coff = packed([ops[i][0] for i in idx], pad, 1)
        s = m.mu_stream(tr_d, n + pad, dev(cflat), dev_off(coff), kidx_dev(kidx), mode)
    last = len(cuts[0]) - 1 if upto is None else upto
    for u in range(first, last):
        flat, off = packed(pieces_of(ops, idx, cuts, u), pad, u % 4)
        s.update(dev(flat), dev_off(off))
    mu, flag = s.final()
    mu_h, flag_h = host(mu), host(flag)
    if pad:  # the copies of op 0 are op 0
        assert (mu_h[n:] == mu_h[0]).all() and not flag_h[n:].any()
    return (s, last), [r.tobytes() for r in mu_h[:n]], flag_h[:n]


# ------------------------------------------------------------------------------------------------------------------ 1. seam
@pytest.mark.parametrize("form", ["wave", "lane"])
@pytest.mark.parametrize("mode", MODES)
def test_every_schedule_gives_the_mu_of_the_whole_message(sets, trs, mode, form):
    if form == "lane" and not PAD_LEG:
        pytest.skip("MLDSA_MUS_WAVE_MAX_OPS is 0 (the natural batch runs in the lane form) or above 65 536 (the padding would be too large)")
    m = sets[44]
    cs = case_set(m, mode, trs)
    ops = cs["ops"]
    assert WAVE_MAX == 0 or len(ops) <= WAVE_MAX  # the natural n is below the threshold
    for name, (idx, cuts) in cs["sched"].items():
        pad = WAVE_MAX + 65 - len(idx) if form == "lane" else 0
        _, mu, flag = stream(m, mode, trs[0], ops, idx, cuts, pad)
        assert not flag.any(), name
        want = hashlib_incremental(ops, cs["op_tr"], mode, idx, cuts)
        assert want == [cs["whole"][i] for i in idx], name
        bad = [i for i, a, b in zip(idx, mu, want) if a != b]
        assert not bad, (name, bad[:8])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(sets, trs, n):
    m = sets[44]
    for mode in MODES:
        cs = case_set(m, mode, trs)
        for name in ("random_1", "cut_1R+0", "one_piece"):
            idx, cuts = cs["sched"][name]
            idx, cuts = idx[-n:], cuts[-n:]  # the end of the list: both long messages are in it from n = 63 on
            _, mu, flag = stream(m, mode, trs[0], cs["ops"], idx, cuts)
            assert not flag.any() and mu == [cs["whole"][i] for i in idx], (mode, name)


# -------------------------------------------------------------------------------------------------- 2. final leaves the state alone
@pytest.mark.parametrize("form", ["wave", "lane"])
def test_final_leaves_the_state_alone(sets, trs, form):
    if form == "lane" and not PAD_LEG:
        pytest.skip("no padded leg for this MLDSA_MUS_WAVE_MAX_OPS")
    m = sets[44]
    for mode in MODES:
        cs = case_set(m, mode, trs)
        ops = cs["ops"]
        idx, cuts = cs["sched"]["random_2"]
        pad = WAVE_MAX + 65 - len(idx) if form == "lane" else 0
        keep, mu7, flag = stream(m, mode, trs[0], ops, idx, cuts, pad, upto=7)
        assert not flag.any() and mu7 == hashlib_incremental(ops, cs["op_tr"], mode, idx, cuts, upto=7)
        assert mu7 == [external_mu(cs["op_tr"][i], ops[i][1][:c[7]], ops[i][0], mode) for i, c in zip(idx, cuts)]  # the mu of the prefix
        assert mu7 != [cs["whole"][i] for i in idx]
        _, mu7_again, _ = stream(m, mode, trs[0], ops, idx, cuts, pad, upto=7, keep=keep)  # no update in between: the same rows
        assert mu7_again == mu7
        _, mu9, flag = stream(m, mode, trs[0], ops, idx, cuts, pad, keep=keep)  # two more updates
        assert not flag.any() and mu9 == [cs["whole"][i] for i in idx]


# ------------------------------------------------------------------------------------------------------------- 3. refusals
GUARD = 4096


def guarded(payload_bytes, pattern):
    """a device buffer [guard | payload | guard], the guards filled with `pattern`: (whole tensor, the payload's view)"""
    body = (payload_bytes + 255) // 256 * 256
    t = torch.full((GUARD + body + GUARD,), pattern, dtype=torch.uint8, device="cuda")
    return t, t[GUARD:GUARD + body]


def guards_intact(t, pattern):
    h = host(t)
    return bool((h[:GUARD] == pattern).all() and (h[-GUARD:] == pattern).all())


def pair_ok(off, i):
    lo, hi, a, b = int(off[0]), int(off[-1]), int(off[i]), int(off[i + 1])
    return lo <= a <= b <= hi


@pytest.mark.parametrize("form", ["wave", "lane"])
def test_refusals_are_per_op_sticky_and_stay_inside_state_and_pieces(sets, form):
    if form == "lane" and not PAD_LEG:
        pytest.skip("no padded leg for this MLDSA_MUS_WAVE_MAX_OPS")
    m = sets[44]
    lib = _mus_lib.load()
    rng = np.random.default_rng(77)
    n, nk = 40, 5
    pad = WAVE_MAX + 65 - n if form == "lane" else 0
    N = n + pad
    xi = [hashlib.sha256(b"mus-refuse" + bytes([j])).digest() for j in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    tr_h = [r.tobytes() for r in host(pks.tr)]
    msgs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(30, 700, n)]
    ctxs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 40, n)]
    ctxs[3] = bytes(256)                                  # flag 1
    kidx = np.arange(N, dtype=np.uint32) % nk
    kidx[n:] = 0
    kidx[9] = nk                                          # flag 2: the key index is n_keys
    cflat, coff = packed(ctxs, pad, 2)
    coff[6] = coff[5] - np.uint64(1)                      # a decreasing ctx pair: op 5 refused, op 6 starts a byte early
    coff[15] = np.uint64(1) << np.uint64(63)              # overshooting: ops 14 and 15 refused
    thirds = [[0, len(x) // 3, 2 * len(x) // 3, len(x)] for x in msgs]
    ups = []
    for u in range(3):
        flat, off = packed([x[c[u]:c[u + 1]] for x, c in zip(msgs, thirds)], pad, u + 1)
        ups.append([flat, off])
    ups[1][1][21] = ups[1][1][20] - np.uint64(1)          # update 2 of 3: op 20's pair decreases; op 21 starts a byte early
    ups[1][1][31] = np.uint64(2 ** 64 - 1)                # ... and ops 30 and 31 overshoot
    null_off = np.zeros(N + 1, dtype=np.uint64)           # a last update with NULL pieces: only ops 34 and 35 name bytes of it
    null_off[35:] += np.uint64(4)
    null_off[36:] += np.uint64(1)
    ups.append([None, null_off])

    # the reference: the rules of the header applied to these tables
    flag = np.zeros(n, dtype=np.int64)
    h = [None] * n
    for i in range(n):
        if not pair_ok(coff, i):
            flag[i] = 2
        else:
            ctx = cflat[int(coff[i]):int(coff[i + 1])].tobytes()
            flag[i] = 1 if len(ctx) > 255 else 2 if kidx[i] >= nk else 0
            if flag[i] == 0:
                h[i] = hashlib.shake_256(tr_h[kidx[i]] + bytes([0, len(ctx)]) + ctx)
    for flat, off in ups:
        for i in range(n):
            a, b = int(off[i]), int(off[i + 1])
            bad = not pair_ok(off, i) or (a != b and flat is None)
            if flag[i] == 0:
                if bad:
                    flag[i] = 2
                elif b > a:
                    h[i].update(flat[a:b].tobytes())
    assert [int(flag[i]) for i in (3, 5, 9, 14, 15, 20, 30, 31, 34, 35)] == [1, 2, 2, 2, 2, 2, 2, 2, 2, 2]
    assert flag[6] == 0 and flag[21] == 0 and int((flag == 0).sum()) == n - 10 >= n // 2  # at least half of the batch is unflagged
    want = [bytes(64) if flag[i] else h[i].digest(64) for i in range(n)]

    sb = lib.mldsa_mus_state_bytes(N)
    st_all, st = guarded(sb, 0xC3)
    st.fill_(0x5A)
    cb_d, co_d, k_d = dev(cflat), dev_off(coff), kidx_dev(kidx)
    s = _stream(m.device)
    _mus_lib.check(lib.mldsa_mus_init(m.hp._h, MODE_PURE, _ptr(pks.tr), nk, _ptr(k_d), _ptr(cb_d), _ptr(co_d), _ptr(st), sb, N, s))
    held = []
    for flat, off in ups:
        o_d = dev_off(off)
        p_ptr = NULL
        if flat is not None:
            p_all, p = guarded(flat.size, 0x3C)
            p[:flat.size] = dev(flat)
            held.append(p_all)
            p_ptr = _ptr(p)
        held.append(o_d)
        _mus_lib.check(lib.mldsa_mus_update(m.hp._h, _ptr(st), sb, p_ptr, _ptr(o_d), N, s))
    mu = torch.full((N + 2, 64), 0xA5, dtype=torch.uint8, device="cuda")
    fl = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
    _mus_lib.check(lib.mldsa_mus_final(m.hp._h, _ptr(st), sb, _ptr(mu[1:]), _ptr(fl[1:]), N, s))
    mu_h, fl_h = host(mu), host(fl)
    assert guards_intact(st_all, 0xC3), "the state's guard regions were written"
    assert (mu_h[0] == 0xA5).all() and (mu_h[-1] == 0xA5).all() and fl_h[0] == -7 and fl_h[-1] == -7
    assert fl_h[1:n + 1].tolist() == flag.tolist()
    for i in range(n):
        assert mu_h[1 + i].tobytes() == want[i], i  # all zero where flagged, the reference elsewhere
    if pad:
        assert not fl_h[n + 1:-1].any() and (mu_h[n + 1:-1] == mu_h[1]).all()

    # the streamed rows as verify_mu / sign_mu take them: the flagged ops fail, exactly they
    mu_d, fl_d = mu[1:n + 1].contiguous(), fl[1:n + 1].contiguous()
    k_n = kidx_dev(kidx[:n])
    rnd = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    sigs = torch.full((n, m.SIG_LEN), 0x77, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    m.sign_mu_device(sks, mu_d, rnd, sigs, n, k_n, mu_flag=fl_d, status=status)
    st_h, sg_h = host(status), host(sigs)
    assert st_h.tolist() == [_lib.ERR_CTX_LEN if f == 1 else _lib.ERR_PARAM if f else _lib.OK for f in flag]
    assert all(not sg_h[i].any() for i in range(n) if flag[i]) and all(sg_h[i].any() for i in range(n) if not flag[i])
    ok = torch.full((n,), 5, dtype=torch.uint8, device="cuda")
    k_v = kidx.copy()[:n]
    m.verify_mu_device(pks, mu_d, sigs, ok, n, kidx_dev(k_v), mu_flag=fl_d)
    assert host(ok).tolist() == [0 if f else 1 for f in flag]
    del held


# ----------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_sign_and_verify_from_streamed_mu(sets, pset):
    m = sets[pset]
    n, nk = 24, 3
    ops = mus_cases.cases(MODE_PURE)
    pick = [i for i, (c, x) in enumerate(ops) if 2 <= len(x) < 5000][:n]
    idx_all, cuts_all = mus_cases.schedules(ops, MODE_PURE)["random_1"]
    cuts = [cuts_all[i] for i in pick]
    ctxs, msgs = [ops[i][0] for i in pick], [ops[i][1] for i in pick]
    pk, sk = m.keygen_from_seed([hashlib.sha256(b"mus-e2e" + bytes([pset, j])).digest() for j in range(nk)])
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    kidx = np.arange(n, dtype=np.uint32) % nk
    rnd = [hashlib.sha256(b"mus-rnd" + bytes([i])).digest() for i in range(n)]
    want = m.try_sign_with_seed(sks, msgs, rnd, ctxs, kidx, mode=MODE_PURE)

    def streamed(messages):
        cb, co = _cat_with_offsets(ctxs, m.device)
        s = m.mu_stream(sks.tr, n, cb, co, kidx_dev(kidx))
        for u in range(len(cuts[0]) - 1):
            s.update(*_cat_with_offsets([x[c[u]:c[u + 1]] for x, c in zip(messages, cuts)], m.device))
        return s.final()

    mu, flag = streamed(msgs)
    assert not host(flag).any()
    rn = torch.frombuffer(bytearray(b"".join(rnd)), dtype=torch.uint8).cuda().view(n, 32)
    sigs = torch.zeros((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
    m.sign_mu_device(sks, mu, rn, sigs, n, kidx_dev(kidx), mu_flag=flag)
    assert torch.equal(sigs, want)
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    m.verify_mu_device(pks, mu, sigs, ok, n, kidx_dev(kidx), mu_flag=flag)
    assert host(ok).all()
    # one message byte flipped inside the second piece of every op that has one
    second = [(c[1], c[2]) for c in cuts]
    hit = [i for i, (a, b) in enumerate(second) if b > a]
    assert len(hit) >= n // 2
    damaged = list(msgs)
    for i in hit:
        a, b = second[i]
        p = (a + b) // 2
        damaged[i] = msgs[i][:p] + bytes([msgs[i][p] ^ 0x10]) + msgs[i][p + 1:]
    mu_bad, _ = streamed(damaged)
    ok.zero_()
    m.verify_mu_device(pks, mu_bad, sigs, ok, n, kidx_dev(kidx))
    assert host(ok).tolist() == [0 if i in hit else 1 for i in range(n)]


def test_acvp_sigver_with_the_messages_cut_in_three(sets, acvp_sigver):
    total = 0
    for g in acvp_sigver["testGroups"]:
        m = sets[PSET[g["parameterSet"]]]
        pk = orc.pk_try_from_bytes(m.pset, bytes.fromhex(g["pk"]))
        k = m.params.k
        d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[None], dtype=dt)).cuda()
        pks = PublicKeys(m.pset, d(np.frombuffer(bytes(pk.rho), dtype=np.uint8), np.uint8), d(np.frombuffer(bytes(pk.tr), dtype=np.uint8), np.uint8),
                         d(np.ctypeslib.as_array(pk.t1_d2_hat_mont)[:k].copy(), np.int32))
        msgs = [bytes.fromhex(t["message"]) for t in g["tests"]]
        n = len(msgs)
        s = m.mu_stream(pks.tr, n, key_idx=kidx_dev(np.zeros(n, dtype=np.uint32)), mode=MODE_INTERNAL)
        for u in range(3):
            s.update(*_cat_with_offsets([x[u * len(x) // 3:(u + 1) * len(x) // 3] for x in msgs], m.device))
        mu, flag = s.final()
        assert not host(flag).any()
        got = m.verify_mu(pks, mu, [bytes.fromhex(t["signature"]) for t in g["tests"]])
        assert got.tolist() == [t["testPassed"] for t in g["tests"]]
        total += n
    assert total == 45


# -------------------------------------------------------------------------------------------------------------- 5. host-fed
_HOST = {}


def host_batch(m):
    if not _HOST:
        rng = np.random.default_rng(11)
        n, nk = len(HOST_LENS), 3
        msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in HOST_LENS]
        ctxs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in [0, 255, 1, 17, 64, 0, 200, 3] * 3]
        rnd = np.frombuffer(b"".join(hashlib.sha256(b"mus-host-rnd" + bytes([i])).digest() for i in range(n)), dtype=np.uint8)
        pk, sk = m.keygen_from_seed([hashlib.sha256(b"mus-host" + bytes([j])).digest() for j in range(nk)])
        pk_h, sk_h = host(pk).copy(), host(sk).copy()
        kidx = (np.arange(n) % nk).astype(np.uint32)
        tr_d = m.public_keys_from_bytes(pk).tr.clone()
        tr_h = [r.tobytes() for r in host(tr_d)]
        big = int(np.argmax(HOST_LENS))
        damaged = list(msgs)
        p = len(msgs[big]) // 2 + 1234  # deep inside the message of many chunks
        damaged[big] = msgs[big][:p] + bytes([msgs[big][p] ^ 1]) + msgs[big][p + 1:]
        sig = m.sign_host(sk_h, msgs, rnd, ctxs, kidx)
        want_ok = m.verify_host(pk_h, msgs, sig, ctxs, kidx)
        want_bad = m.verify_host(pk_h, damaged, sig, ctxs, kidx)
        assert want_ok.all() and want_bad.tolist() == [i != big for i in range(n)]
        _HOST.update(n=n, nk=nk, msgs=msgs, ctxs=ctxs, rnd=rnd, pk=pk_h, sk=sk_h, kidx=kidx, tr_d=tr_d, damaged=damaged, sig=sig.copy(), big=big,
                     want_bad=want_bad, mu=[external_mu(tr_h[kidx[i]], msgs[i], ctxs[i]) for i in range(n)])
    return _HOST


def in_host_memory(items, pinned, keep):
    """(flat, offsets) of the byte strings, in page-locked memory if asked"""
    flat = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in items], out=off[1:])
    if pinned:
        t = torch.empty(flat.size, dtype=torch.uint8, pin_memory=True)
        keep.append(t)
        a = t.numpy()
        a[:] = flat
        flat = a
    return flat, off


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("staging", [4096, 0])
def test_host_fed(sets, staging, pinned):
    m = sets[44]
    b = host_batch(m)
    n = b["n"]
    off = np.concatenate([[0], np.cumsum(HOST_LENS)])
    if staging == 4096:  # what the sizes guarantee: a message in more than 40 chunks, a chunk with more than 3 messages
        assert max((off[i + 1] - 1) // 4096 - off[i] // 4096 + 1 for i in range(n) if HOST_LENS[i]) > 40
        assert max(sum(1 for i in range(n) if HOST_LENS[i] and off[i] < c + 4096 and off[i + 1] > c) for c in range(0, int(off[-1]), 4096)) > 3
    keep = []
    messages = in_host_memory(b["msgs"], pinned, keep)
    mu, flag = m.mu_host(b["tr_d"], messages, b["ctxs"], b["kidx"], MODE_PURE, staging)
    assert not host(flag).any() and [r.tobytes() for r in host(mu)] == b["mu"]
    assert m.verify_host_streamed(b["pk"], messages, b["sig"], b["ctxs"], b["kidx"], staging_bytes=staging).all()
    got_bad = m.verify_host_streamed(b["pk"], in_host_memory(b["damaged"], pinned, keep), b["sig"], b["ctxs"], b["kidx"], staging_bytes=staging)
    assert got_bad.tolist() == b["want_bad"].tolist() and not got_bad[b["big"]]
    assert np.array_equal(m.sign_host_streamed(b["sk"], messages, b["rnd"], b["ctxs"], b["kidx"], staging_bytes=staging), b["sig"])


def test_host_fed_refusals(sets):
    m = sets[44]
    b = host_batch(m)
    n = b["n"]
    lib = _mus_lib.load()
    flat, off = in_host_memory(b["msgs"], False, [])
    ctxs = list(b["ctxs"])
    ctxs[4] = bytes(256)                      # flag 1 on that op alone
    mu, flag = m.mu_host(b["tr_d"], (flat, off), ctxs, b["kidx"], MODE_PURE, 4096)
    assert host(flag).tolist() == [1 if i == 4 else 0 for i in range(n)]
    assert [r.tobytes() for r in host(mu)] == [bytes(64) if i == 4 else b["mu"][i] for i in range(n)]
    ctxs[4] = bytes(70000)                    # of a long ctx the device sees 256 bytes: the same flag, the same rows
    mu2, flag2 = m.mu_host(b["tr_d"], (flat, off), ctxs, b["kidx"], MODE_PURE, 4096)
    assert torch.equal(mu2, mu) and torch.equal(flag2, flag)
    # without ctxs every ctx is empty; key_idx NULL: op i uses key i, and the ops past the table are refused
    mu3, flag3 = m.mu_host(b["tr_d"], (flat, off), None, b["kidx"], MODE_INTERNAL, 4096)
    tr_h = [r.tobytes() for r in host(b["tr_d"])]
    assert [r.tobytes() for r in host(mu3)] == [external_mu(tr_h[b["kidx"][i]], b["msgs"][i], mode=MODE_INTERNAL) for i in range(n)]
    # a malformed msg_off fails the whole call before a byte is read, and mu is untouched
    bad = off.copy()
    bad[7] = bad[6] - np.uint64(1)
    out = torch.full((n, 64), 0xA5, dtype=torch.uint8, device="cuda")
    fl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kd = kidx_dev(b["kidx"])
    torch.cuda.synchronize()
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc = lib.mldsa_mus_host_compute(m._mus_host(4096), MODE_PURE, _ptr(b["tr_d"]), b["nk"], _ptr(kd), ptr(flat), ptr(bad), NULL, NULL, _ptr(out),
                                    _ptr(fl), n)
    assert rc == _lib.ERR_PARAM and b"mldsa_check_offsets(msg_off)" in lib.mldsa_mus_last_error()
    assert (host(out) == 0xA5).all() and (host(fl) == -7).all()
    rc = lib.mldsa_mus_host_compute(m._mus_host(4096), MODE_PURE, _ptr(b["tr_d"]), b["nk"], NULL, ptr(flat), ptr(off), NULL, NULL, _ptr(out),
                                    _ptr(fl), n)
    assert rc == _lib.OK and host(fl).tolist() == [0] * b["nk"] + [2] * (n - b["nk"]) and not host(out)[b["nk"]:].any()
    assert [r.tobytes() for r in host(out)[:b["nk"]]] == [external_mu(tr_h[i], b["msgs"][i]) for i in range(b["nk"])]


# The smallest shape that puts chunk ends on message ends, through both host-memory feeds (mu here, HashML-DSA in the pre-hash layer).
# With 256-byte staging the chunks are [0, 256) [256, 512) [512, 768) [768, 777): message 1 ends exactly on a chunk end, two empty
# messages sit on that boundary, message 4 starts on it and spans three chunks, an empty message ends the batch.  256 is at least every
# pre-hash block or rate, so nothing below one block per chunk is relied on.
EDGE_LENS = [0, 256, 0, 0, 520, 1, 0]


@pytest.mark.parametrize("pinned", [False, True])
def test_host_feeds_with_chunk_ends_on_message_ends(sets, pinned):
    m = MlDsa(44, hotpath=sets[44].hp)  # an object of its own: the handles below are created here and grow here
    staging, n, nk = 256, len(EDGE_LENS), 3
    rng = np.random.default_rng(256)
    msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in EDGE_LENS]
    rnd = [hashlib.sha256(b"edge-rnd" + bytes([i])).digest() for i in range(n)]
    rn = np.frombuffer(b"".join(rnd), dtype=np.uint8)
    pk, sk = m.keygen_from_seed([hashlib.sha256(b"edge-key" + bytes([j])).digest() for j in range(nk)])
    pk_h, sk_h = host(pk).copy(), host(sk).copy()
    kidx = (np.arange(n) % nk).astype(np.uint32)
    tr_d = m.public_keys_from_bytes(pk).tr.clone()
    tr_h = [r.tobytes() for r in host(tr_d)]
    sks = m.private_keys_from_bytes(sk)
    want_mu = [external_mu(tr_h[kidx[i]], msgs[i]) for i in range(n)]
    want_sig = {ph: [r.tobytes() for r in host(m.try_hash_sign_with_seed(sks, msgs, rnd, ph=ph, key_idx=kidx, prehash="host"))]
                for ph in ("SHA512", "SHAKE128")}
    keep = []
    flat, off = in_host_memory(msgs, pinned, keep)
    assert off.tolist() == [0, 0, 256, 256, 256, 776, 777, 777]

    def this_call(ops=n):
        """the first `ops` ops through mu_host, hash_sign_host and hash_verify_host: (mu rows, {ph: signatures})"""
        o = off[:ops + 1]
        mu, flag = m.mu_host(tr_d, (flat, o), None, kidx[:ops], MODE_PURE, staging)
        assert not host(flag).any()
        sigs = {}
        for ph in want_sig:
            sig = m.hash_sign_host(sk_h, (flat, o), rn[:32 * ops], ph=ph, key_idx=kidx[:ops], staging_bytes=staging)
            assert m.hash_verify_host(pk_h, (flat, o), sig, ph=ph, key_idx=kidx[:ops], staging_bytes=staging).all(), ph
            sigs[ph] = [r.tobytes() for r in sig]
        return [r.tobytes() for r in host(mu)], sigs

    # a call of 3 ops first, then the whole batch on the same handles: the per-call buffers grow
    mu3, sig3 = this_call(3)
    assert mu3 == want_mu[:3] and all(sig3[ph] == want_sig[ph][:3] for ph in want_sig)
    first = this_call()
    assert first[0] == want_mu and first[1] == want_sig
    # a call refused for a decreasing msg_off on each handle, then the batch again: identical results
    bad = off.copy()
    bad[5] = bad[4] - np.uint64(1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    mus, ph_lib = _mus_lib.load(), _ph_lib.load()
    out = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    kd = kidx_dev(kidx)
    torch.cuda.synchronize()
    assert mus.mldsa_mus_host_compute(m._mus_host(staging), MODE_PURE, _ptr(tr_d), nk, _ptr(kd), ptr(flat), ptr(bad), NULL, NULL, _ptr(out), NULL,
                                      n) == _lib.ERR_PARAM
    sg, okb = np.frombuffer(b"".join(want_sig["SHA512"]), dtype=np.uint8), np.full(n, 7, dtype=np.uint8)
    assert ph_lib.mldsa_hash_verify_host(m._ph_host(staging), 44, m._ph_arg("SHA512"), ptr(pk_h), nk, ptr(kidx), ptr(flat), ptr(bad), NULL, NULL,
                                         ptr(sg), ptr(okb), n) == _lib.ERR_PARAM
    assert not host(out).any() and (okb == 7).all()
    assert this_call() == first


# ----------------------------------------------------------------------------------------------------------- 6. many ops
def test_8192_ops_in_1_3_and_16_updates_and_two_streams_interleaved(sets, trs):
    m = sets[44]
    rng = np.random.default_rng(8192)
    n = 8192
    lens = rng.integers(0, 2001, n)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    kidx = kidx_dev(np.arange(n, dtype=np.uint32) % N_KEYS)
    want, flag = m.mu_device(trs[0], dev(buf), dev_off(off), n, key_idx=kidx)
    assert not host(flag).any()
    h = host(want)
    for i in (0, 1, n // 2, n - 1):
        assert h[i].tobytes() == external_mu(trs[1][i % N_KEYS], buf[int(off[i]):int(off[i + 1])].tobytes())
    for updates in (1, 3, 16):
        cuts = mus_cases.random_cuts(lens, updates, rng)
        s = m.mu_stream(trs[0], n, key_idx=kidx)
        for u in range(updates):
            flat, poff = mus_cases.gather_pieces(buf, off, cuts, u)
            s.update(dev(flat) if flat.size else None, dev_off(poff))
        mu, flag = s.final()
        assert torch.equal(mu, want) and not host(flag).any(), updates
    # two MuStreams on two torch streams, their updates issued alternately: A hashes the messages, B the messages reversed
    rbuf = np.ascontiguousarray(buf[::-1])
    roff = (off[-1] - off[::-1]).astype(np.uint64)
    rlens = lens[::-1].copy()
    rkidx = kidx_dev((np.arange(n, dtype=np.uint32)[::-1] % N_KEYS).copy())
    want_b, _ = m.mu_device(trs[0], dev(rbuf), dev_off(roff), n, key_idx=rkidx)
    cuts_a, cuts_b = mus_cases.random_cuts(lens, 4, rng), mus_cases.random_cuts(rlens, 4, rng)
    ups_a = [mus_cases.gather_pieces(buf, off, cuts_a, u) for u in range(4)]
    ups_b = [mus_cases.gather_pieces(rbuf, roff, cuts_b, u) for u in range(4)]
    dev_a = [(dev(f), dev_off(o)) for f, o in ups_a]
    dev_b = [(dev(f), dev_off(o)) for f, o in ups_b]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = m.mu_stream(trs[0], n, key_idx=kidx)
    with torch.cuda.stream(sb):
        b = m.mu_stream(trs[0], n, key_idx=rkidx)
    for u in range(4):
        with torch.cuda.stream(sa):
            a.update(*dev_a[u])
        with torch.cuda.stream(sb):
            b.update(*dev_b[u])
    with torch.cuda.stream(sa):
        mu_a, _ = a.final()
    with torch.cuda.stream(sb):
        mu_b, _ = b.final()
    torch.cuda.synchronize()
    assert torch.equal(mu_a, want) and torch.equal(mu_b, want_b)
