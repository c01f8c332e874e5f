"""The nine pre-hash functions beyond the reference's three (SHA-224/384, SHA-512/224, SHA-512/256, SHA3-224/256/384/512,
SHAKE256) on the device, through every path of include/mldsa_ph.h: the seam against hashlib in both kernel forms (one message
per lane; one per wave for Keccak-family calls of at most MLDSA_PH_COOP_MAX_OPS operations), HashML-DSA signatures and verdicts
against the oracle on rows from this suite's own table, the incremental and the host-memory paths, and the per-op refusals."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

import ph_fips_list_cases as cases
import ph_stream_cases as stream_cases
from fips204_amd import _lib, _ph_lib
from fips204_amd.hotpath import _ptr
from fips204_amd.ml_dsa import _cat_with_offsets

pytestmark = pytest.mark.gpu

NEW = cases.NEW
NULL = C.c_void_p(0)
T = cases.coop_max_ops()  # calls of <= T ops take the wave form for the Keccak family (0: there is none)
# HOST_LENS of test_gpu_prehash_stream.py
HOST_LENS = (0, 1, 63, 64, 65, 167, 168, 4095, 4096, 4097, 5000, 12289, 200 << 10, 3, 9000, 128, 100, 2, 70000, 31, 8192, 777, 1, 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows_in_calls(m, d_buf, off, n, ph, max_ops):
    """prehash_device over ops [0, n) in calls of at most max_ops ops, each with its own slice of the table: (rows, bad) on the host"""
    rows, bad = [], []
    for a in range(0, n, max_ops):
        b = min(n, a + max_ops)
        r, x = m.prehash_device(d_buf, dev_off(off[a:b + 1]), b - a, ph)
        rows.append(host(r))
        bad.append(host(x))
    return np.concatenate(rows), np.concatenate(bad)


def _filler(k, tag):
    """k short messages (0 .. 400 bytes) that lift a batch above the small-call threshold"""
    return [shake(tag, i, 401)[:(i * 37) % 401] for i in range(k)]


def test_own_table_agrees_with_the_header_and_the_front_end():
    for name, (code, _, dlen, _, _) in cases.ALL.items():
        assert _ph_lib.load().mldsa_ph_row_len(code) == 11 + dlen, name
        from fips204_amd.ml_dsa import _ph_code
        assert _ph_code(name) == code, name


@pytest.mark.parametrize("ph", NEW)
def test_seam_matches_hashlib_in_both_kernel_forms(sets, ph):
    """every padding edge of every family in one batch, 200 random lengths, two 4 MiB messages among short ones, no message
    dword-aligned: rows = OID || hashlib digest, byte for byte, in calls of at most MLDSA_PH_COOP_MAX_OPS ops and in one call
    above it"""
    m = sets[65]
    msgs = cases.seam_messages()
    assert {len(x) for x in msgs} >= set(cases.EDGES) and sum(len(x) == 4 << 20 for x in msgs) == 2
    big = msgs + _filler(max(0, T + 1 - len(msgs)), b"seam-fill")
    assert len(big) > T
    want = [cases.own_row(x, ph) for x in big]
    for base in (1, 2, 3):
        flat, off = cases.skewed_table(big, base)
        assert int(off[0]) % 2 == 1
        d = dev(flat)[base:]
        n_small = len(msgs)
        forms = [("one call above the threshold", len(big), len(big))]
        if T > 0:
            forms.append(("calls of at most the threshold", n_small, min(T, n_small)))
        for label, n, step in forms:
            rows, bad = _rows_in_calls(m, d, off, n, ph, step)
            assert not bad.any(), (ph, base, label)
            assert rows.shape == (n, cases.row_len(ph))
            for i in range(n):
                assert rows[i].tobytes() == want[i], (ph, base, label, i, len(big[i]))


@pytest.mark.parametrize("ph", NEW)
def test_seam_call_sizes_around_a_wave_and_the_threshold(sets, ph):
    m = sets[44]
    sizes = sorted({1, 2, 63, 64, 65, max(T, 1), T + 1})
    msgs = _filler(max(sizes), b"size-" + ph.encode())
    msgs[0] = b""
    want = [cases.own_row(x, ph) for x in msgs]
    flat, off = cases.skewed_table(msgs, 1)
    d = dev(flat)[1:]
    for n in sizes:
        rows, bad = m.prehash_device(d, dev_off(off[:n + 1]), n, ph)
        rows = host(rows)
        assert not host(bad).any()
        assert [r.tobytes() for r in rows] == want[:n], (ph, n)


@pytest.mark.parametrize("ph", NEW)
def test_seam_65536_random_lengths(sets, ph):
    m = sets[44]
    rng = np.random.default_rng(11)
    n = 65536
    assert n > T
    lens = rng.integers(0, 2049, n)
    buf = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    rows, bad = m.prehash_device(dev(buf), dev_off(off), n, ph)
    rows = host(rows)
    assert not host(bad).any()
    raw = buf.tobytes()
    for i in range(n):
        assert rows[i].tobytes() == cases.own_row(raw[int(off[i]):int(off[i + 1])], ph), (ph, i)


@pytest.mark.parametrize("ph", NEW)
def test_nothing_is_written_behind_the_rows(sets, ph):
    """rows go into a buffer pre-filled with 0x77 with 16 guard bytes behind it: the 28- and 48-byte digests end their rows, in
    mldsa_prehash (both forms) and in mldsa_ph_final"""
    m = sets[44]
    lib, code = _ph_lib.load(), cases.ALL[ph][0]
    rl = cases.row_len(ph)
    for n in sorted({1, 7, 64, max(T, 1), T + 1, T + 130}):
        msgs = _filler(n, b"guard")
        buf, off = table(msgs)
        d_buf, d_off = dev(buf), dev_off(off)
        want = b"".join(cases.own_row(x, ph) for x in msgs)
        out = torch.full((n * rl + 16,), 0x77, dtype=torch.uint8, device="cuda")
        bad = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
        _ph_lib.check(lib.mldsa_prehash(m.hp._h, code, _ptr(d_buf), _ptr(d_off), _ptr(out), _ptr(bad), n, _stream()))
        o, b = host(out), host(bad)
        assert o[:n * rl].tobytes() == want, (ph, n)
        assert (o[n * rl:] == 0x77).all() and not b[:n].any() and (b[n:] == 0x77).all(), (ph, n)
        st = m.prehash_stream(n, ph).update(d_buf, d_off)
        out2 = torch.full((n * rl + 16,), 0x77, dtype=torch.uint8, device="cuda")
        _ph_lib.check(lib.mldsa_ph_final(m.hp._h, code, _ptr(st.state), st.state_bytes, _ptr(out2), NULL, NULL, n, _stream()))
        o2 = host(out2)
        assert o2[:n * rl].tobytes() == want and (o2[n * rl:] == 0x77).all(), (ph, n)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_hash_sign_device_matches_the_oracle_on_own_rows(sets, pset):
    m = sets[pset]
    rng = np.random.default_rng(700 + pset)
    keys = [orc.keygen_from_seed(pset, bytes([pset, k + 3]) * 16) for k in range(2)]
    sks = m.private_keys_from_bytes([orc.sk_into_bytes(pset, sk) for _, sk in keys])
    n = 6
    kidx = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint32)
    msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 1, 71, 135, 1000, 5000)]
    hedged = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    ctx_sets = (None, [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 255, 3, 17, 1, 63)])
    for ph in NEW:
        rows = [cases.own_row(x, ph) for x in msgs]
        for ctxs in ctx_sets:
            for rnd in ([bytes(32)] * n, hedged):  # deterministic and hedged
                got = host(m.try_hash_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, ph=ph, key_idx=kidx, prehash="device"))
                for i in range(n):
                    ctx = ctxs[i] if ctxs else b""
                    want = orc.sign_internal(pset, keys[kidx[i]][1], rows[i], rnd[i], ctx=ctx, mode=2)
                    assert got[i].tobytes() == want, (pset, ph, i, ctxs is None)
        # the host route reaches the same bytes through hashlib
        ref = host(m.try_hash_sign_with_seed(sks, msgs, hedged, ctxs=ctx_sets[1], ph=ph, key_idx=kidx, prehash="host"))
        assert np.array_equal(got, ref), (pset, ph)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_hash_verify_device_verdicts_are_the_oracles(sets, pset):
    m = sets[pset]
    rng = np.random.default_rng(800 + pset)
    pk_o, sk_o = orc.keygen_from_seed(pset, bytes(range(2, 34)))
    pks = m.public_keys_from_bytes([orc.pk_into_bytes(pset, pk_o)])
    pk_bytes = torch.from_numpy(np.frombuffer(orc.pk_into_bytes(pset, pk_o), dtype=np.uint8).copy()).cuda().view(1, -1)
    for ph in NEW:
        siblings = [s for grp in cases.SAME_LENGTH if ph in grp for s in grp if s != ph]
        assert siblings
        n = 8 + len(siblings)
        msgs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 400, n)]
        ctxs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 20, n)]
        signed_ph = [ph] * 8 + siblings  # the last ops are signed under another function whose digest has the same length
        sigs = [bytearray(orc.sign_internal(pset, sk_o, cases.own_row(msgs[i], signed_ph[i]), bytes(32), ctx=ctxs[i], mode=2)) for i in range(n)]
        v_msgs, v_ctxs = list(msgs), list(ctxs)
        sigs[1][10] ^= 1                                                   # damaged signature
        v_ctxs[4] = v_ctxs[4] + b"x"                                       # wrong ctx
        v_msgs[5] = bytes([v_msgs[5][0] ^ 0x80]) + v_msgs[5][1:]           # damaged message byte
        exp = [bool(orc.verify_internal(pset, pk_o, cases.own_row(v_msgs[i], ph), bytes(sigs[i]), ctx=v_ctxs[i], mode=2)) for i in range(n)]
        assert exp[:8] == [True, False, True, True, False, False, True, True], (pset, ph, exp)
        assert not any(exp[8:]), (pset, ph, siblings)                      # only the OID byte differs: the verdict is false
        sg = torch.from_numpy(np.frombuffer(b"".join(bytes(s) for s in sigs), dtype=np.uint8).copy()).cuda().view(n, -1)
        got = m.hash_verify(pks, v_msgs, sg, ctxs=v_ctxs, ph=ph, key_idx=np.zeros(n, np.uint32), prehash="device")
        assert list(got) == exp, (pset, ph)
        mb, mo = _cat_with_offsets(v_msgs, m.device)
        cb, co = _cat_with_offsets(v_ctxs, m.device)
        ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        m.hash_verify_pk_device(pk_bytes, mb, mo, sg, ok, n, ph, cb, co, key_idx=torch.zeros(n, dtype=torch.int32, device="cuda"))
        assert list(host(ok).astype(bool)) == exp, (pset, ph)
        # the same ops in a call above the small-call threshold (the lane form): pad with copies of op 0
        reps = T + 1
        if T > 0:
            big_msgs, big_ctxs = v_msgs + [v_msgs[0]] * reps, v_ctxs + [v_ctxs[0]] * reps
            sg_big = torch.cat([sg, sg[0:1].expand(reps, -1)]).contiguous()
            got = m.hash_verify(pks, big_msgs, sg_big, ctxs=big_ctxs, ph=ph, key_idx=np.zeros(n + reps, np.uint32), prehash="device")
            assert list(got) == exp + [True] * reps, (pset, ph)


@pytest.mark.parametrize("ph", NEW)
def test_incremental_rows_are_the_one_shot_rows_for_every_cut(sets, ph):
    m = sets[65]
    msgs = cases.seam_messages()
    want = [cases.own_row(x, ph) for x in msgs]
    buf, off = table(msgs)
    one_shot, bad1 = m.prehash_device(dev(buf), dev_off(off), len(msgs), ph)
    one_shot = host(one_shot)
    assert not host(bad1).any()
    sched = cases.cut_schedules(msgs, ph)
    assert {"random_1", "random_3", "random_16", "cut_1B-1", "cut_1B+0", "cut_1B+1"} <= set(sched)
    ops = list(range(len(msgs)))
    for k, (name, cuts) in enumerate(sched.items()):
        base = k % 4
        st = m.prehash_stream(len(msgs), ph)
        for u in range(len(cuts[0]) - 1):
            flat, poff = cases.skewed_table(stream_cases.pieces_of(msgs, ops, cuts, u), base)
            st.update(dev(flat)[base:], dev_off(poff))
        rows, bad = st.final()
        rows = host(rows)
        assert not host(bad).any(), (ph, name)
        for i in ops:
            assert rows[i].tobytes() == want[i], (ph, name, i, len(msgs[i]), cuts[i][:4])
        assert np.array_equal(rows, one_shot), (ph, name)
    rows, bad = m.prehash_stream(70, ph).final()  # init then final: the empty message
    assert not host(bad).any() and all(r.tobytes() == cases.own_row(b"", ph) for r in host(rows))


@pytest.mark.parametrize("ph", NEW)
def test_incremental_65536_ops_and_sticky_refusals(sets, ph):
    m = sets[44]
    rng = np.random.default_rng(13)
    n = 65536
    lens = rng.integers(0, 1025, n)
    buf = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    want, _ = m.prehash_device(dev(buf), dev_off(off), n, ph)  # tied to hashlib by test_seam_65536_random_lengths
    want = host(want)
    for i in (0, 1, 777, n - 1):
        assert want[i].tobytes() == cases.own_row(buf[int(off[i]):int(off[i + 1])].tobytes(), ph)
    for U in (3, 16):
        cuts = stream_cases.random_cuts(lens, U, np.random.default_rng(100 + U))
        st = m.prehash_stream(n, ph)
        for u in range(U):
            flat, poff = stream_cases.gather_pieces(buf, off, cuts, u)
            st.update(dev(np.concatenate([flat, np.zeros(8, np.uint8)])), dev_off(poff))
        rows, bad = st.final()
        rows = host(rows)
        assert not host(bad).any()
        diff = np.nonzero((rows != want).any(axis=1))[0]
        assert diff.size == 0, (ph, U, diff[:8], lens[diff[:8]])
    # a malformed piece pair marks its own op, stays through the later updates, and leaves the other ops alone
    n = 4096
    parts = [[rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 200, n)] for _ in range(3)]
    tabs = [table(p) for p in parts]
    t = tabs[1][1].copy()
    k1, k2, k3 = 1000, 2000, 3000
    t[k1 + 1] = t[k1] - np.uint64(1)                                    # decreasing
    t[k2 + 1] = np.uint64(1) << np.uint64(60)                           # overshooting
    t[k3] = np.uint64(2 ** 64 - 8); t[k3 + 1] = np.uint64(2 ** 64 - 1)  # wrapping
    okp = pairs_ok(t)
    assert 3 <= (~okp).sum() <= 8 and not okp[k1] and not okp[k2] and not okp[k3]
    named = [tabs[1][0][int(t[i]):int(t[i + 1])].tobytes() if okp[i] else b"" for i in range(n)]
    st = m.prehash_stream(n, ph)
    for u in range(3):
        st.update(dev(tabs[u][0]), dev_off(t if u == 1 else tabs[u][1]))
    rows, bad = st.final()
    rows, bad = host(rows), host(bad)
    assert np.array_equal(bad.astype(bool), ~okp) and not rows[~okp].any()
    for i in np.nonzero(okp)[0]:
        assert rows[i].tobytes() == cases.own_row(parts[0][i] + named[i] + parts[2][i], ph), (ph, i)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_hash_host_calls_match_the_host_prehash_route(sets, pset):
    """messages, keys and signatures in host memory, staging smaller than the largest message and the default, pageable and
    page-locked buffers: signatures and verdicts are those of the prehash="host" route (hashlib + the core)"""
    m = sets[pset]
    rng = np.random.default_rng(900 + pset)
    n, nk = len(HOST_LENS), 3
    msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in HOST_LENS]
    ctxs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in [0, 255, 1, 17, 64, 0, 200, 3] * 3]
    rnd = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    assert max(HOST_LENS) > 4096
    keys = [orc.keygen_from_seed(pset, bytes([pset, k + 11]) * 16) for k in range(nk)]
    pk_b = np.frombuffer(b"".join(orc.pk_into_bytes(pset, pk) for pk, _ in keys), dtype=np.uint8)
    sk_b = np.frombuffer(b"".join(orc.sk_into_bytes(pset, sk) for _, sk in keys), dtype=np.uint8)
    kidx = (np.arange(n) * 2 % nk).astype(np.uint32)
    sks_dev = m.private_keys_from_bytes([orc.sk_into_bytes(pset, sk) for _, sk in keys])
    pks_dev = m.public_keys_from_bytes([orc.pk_into_bytes(pset, pk) for pk, _ in keys])
    mflat, moff = m._cat_host(msgs)
    rn = np.frombuffer(b"".join(rnd), dtype=np.uint8)
    for ph in NEW:
        want = host(m.try_hash_sign_with_seed(sks_dev, msgs, rnd, ctxs=ctxs, ph=ph, key_idx=kidx, prehash="host"))
        i0 = 9  # one op against the oracle on this suite's own row, so that the host route itself is anchored
        assert want[i0].tobytes() == orc.sign_internal(pset, keys[kidx[i0]][1], cases.own_row(msgs[i0], ph), rnd[i0], ctx=ctxs[i0], mode=2)
        v_sigs = want.copy()
        v_msgs = list(msgs)
        v_sigs[2, 40] ^= 4
        big = bytearray(v_msgs[18]); big[4096 * 9 + 5] ^= 0x40  # a byte deep inside a message of many chunks
        v_msgs[18] = bytes(big)
        v_msgs[0] = b"\x00"
        exp = m.hash_verify(pks_dev, v_msgs, torch.from_numpy(v_sigs).cuda(), ctxs=ctxs, ph=ph, key_idx=kidx, prehash="host")
        assert exp.sum() == n - 3 and not any(exp[i] for i in (0, 2, 18))
        vflat, voff = m._cat_host(v_msgs)
        pin_m, mflat_p = _host_alloc(m, mflat)
        pin_v, vflat_p = _host_alloc(m, vflat)
        try:
            for staging in (4096, 0):
                for pinned in (False, True):
                    got = m.hash_sign_host(sk_b, (mflat_p if pinned else mflat, moff), rn, ctxs=ctxs, ph=ph, key_idx=kidx, staging_bytes=staging)
                    assert np.array_equal(got, want), (pset, ph, staging, pinned)
                    ok = m.hash_verify_host(pk_b, (vflat_p if pinned else vflat, voff), v_sigs.reshape(-1), ctxs=ctxs, ph=ph, key_idx=kidx,
                                            staging_bytes=staging)
                    assert list(ok) == list(exp), (pset, ph, staging, pinned)
        finally:
            m.lib.mldsa_host_free(pin_m)
            m.lib.mldsa_host_free(pin_v)


@pytest.mark.parametrize("ph", ("SHA224", "SHA384", "SHA3_512", "SHAKE256"))
def test_refusals_touch_only_their_own_ops_in_both_kernel_forms(sets, ph):
    """malformed message pairs and |ctx| > 255: one function of each family (SHA-2 with 32- and with 64-bit words, SHA-3, SHAKE),
    a call of at most MLDSA_PH_COOP_MAX_OPS ops and one above it"""
    m = sets[44]
    nk = 4
    xi = [shake(b"phl-bnd", i) for i in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    for n in sorted({min(max(T, 64), 512), max(T + 64, 2048)}):
        kidx = (np.arange(n) % nk).astype(np.uint32)
        kd = torch.from_numpy(kidx.view(np.int32)).cuda()
        msgs = [shake(b"phl-bnd-msg", i, 1 + i % 97) for i in range(n)]
        rnd = [shake(b"phl-bnd-rnd", i) for i in range(n)]
        buf, off = table(msgs)
        t = off.copy()
        k1, k2, k3 = n // 4, n // 2, 3 * n // 4
        t[k1 + 1] = t[k1] - np.uint64(1)           # decreasing
        t[k2 + 1] = np.uint64(1) << np.uint64(60)  # past the end
        okp = pairs_ok(t)
        assert (~okp).sum() >= 3 and okp.sum() > n - 6 and okp[k3]
        ctxs = [b"c" * (i % 5) for i in range(n)]
        ctxs[k3] = bytes(256)                      # one ctx too long, on an op whose message pair is fine
        cb, co = _cat_with_offsets(ctxs, m.device)
        long_ctx = np.zeros(n, dtype=bool)
        long_ctx[k3] = True
        good = okp & ~long_ctx
        mb, mo = dev(buf), dev_off(t)
        rn = torch.from_numpy(np.frombuffer(b"".join(rnd), dtype=np.uint8).copy()).cuda().view(n, 32)
        sg = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        m.hash_sign_device(sks, mb, mo, rn, sg, n, ph, cb, co, key_idx=kd, status=st)
        sg_h, st_h = host(sg), host(st)
        named = [buf[int(t[i]):int(t[i + 1])].tobytes() if good[i] else b"" for i in range(n)]
        ref_ctxs = [c if good[i] else b"" for i, c in enumerate(ctxs)]
        ref = host(m.try_hash_sign_with_seed(sks, named, rnd, ctxs=ref_ctxs, ph=ph, key_idx=kidx, prehash="host"))
        assert (st_h[good] == 0).all() and np.array_equal(sg_h[good], ref[good]), (ph, n)
        assert (st_h[~okp] == _lib.ERR_PARAM).all() and st_h[k3] == _lib.ERR_CTX_LEN and not sg_h[~good].any(), (ph, n)
        i0 = k1 - 1  # a neighbour of a refused op, against the oracle on this suite's own row
        sk0 = orc.sk_try_from_bytes(44, host(sk)[kidx[i0]].tobytes())
        assert sg_h[i0].tobytes() == orc.sign_internal(44, sk0, cases.own_row(named[i0], ph), rnd[i0], ctx=ctxs[i0], mode=2)
        ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        m.hash_verify_device(pks, mb, mo, torch.from_numpy(ref).cuda(), ok, n, ph, cb, co, key_idx=kd)
        ok_h = host(ok)
        assert (ok_h[good] == 1).all() and (ok_h[~good] == 0).all(), (ph, n)
        rows, bad = m.prehash_device(mb, mo, n, ph)
        assert np.array_equal(host(bad).astype(bool), ~okp) and not host(rows)[~okp].any(), (ph, n)
