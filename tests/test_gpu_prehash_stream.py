"""The incremental pre-hash on the device (mldsa_ph_init / _update / _final) and HashML-DSA from host memory
(mldsa_hash_verify_host / mldsa_hash_sign_host): every way of cutting messages against hashlib and the one-shot kernel, the
per-op refusals, the host calls against the oracle and the existing paths, and stream behaviour."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

import ph_stream_cases as cases
from fips204_amd import _lib, _ph_lib
from fips204_amd.hotpath import _ptr
from fips204_amd.ml_dsa import hash_message

pytestmark = pytest.mark.gpu

PHS = cases.PHS
NULL = C.c_void_p(0)


def _run_schedule(m, msgs, ops, cuts, ph, base=0):
    """init, one update per piece column, final: (rows, bad) on the host.  The pieces of an update lie back to back behind
    `base` + 5 bytes, so that with base = 1, 2, 3 they start at every byte alignment."""
    st = m.prehash_stream(len(ops), ph)
    for u in range(len(cuts[0]) - 1):
        pieces = cases.pieces_of(msgs, ops, cuts, u)
        skew = 5
        flat = np.frombuffer(bytes(base + skew) + b"".join(pieces) + bytes(8), dtype=np.uint8)
        off = np.zeros(len(ops) + 1, dtype=np.uint64)
        off[0] = skew
        np.cumsum([len(p) for p in pieces], out=off[1:])
        off[1:] += np.uint64(skew)
        st.update(dev(flat)[base:], dev_off(off))
    rows, bad = st.final()
    return host(rows), host(bad)


@pytest.mark.parametrize("ph", PHS)
def test_stream_seam_matches_hashlib_for_adversarial_splits(sets, ph):
    m = sets[65]
    msgs = cases.seam_messages()
    sched = cases.schedules(msgs, ph)
    # the inputs reach every head / tail case of the update kernel (a quiet generator bug must not empty this test)
    cov = cases.coverage(msgs, sched, ph)
    print(ph, "coverage", cov)
    for key in ("tail_block_minus_1", "completes_exactly", "completes_then_2_blocks", "final_update_empty"):
        assert cov[key] >= 1, (ph, key)
    assert len(sched) == 14 and sum(len(x) > 300 for x in msgs) > 100 and sum(len(x) == 4 << 20 for x in msgs) == 2
    want = [hash_message(x, ph) for x in msgs]
    buf, off = table(msgs)
    one_shot, bad1 = m.prehash_device(dev(buf), dev_off(off), len(msgs), ph)
    one_shot = host(one_shot)
    assert not host(bad1).any()
    for name, (ops, cuts) in sched.items():
        base = int(name[-1]) if name.startswith("random_") else 0
        rows, bad = _run_schedule(m, msgs, ops, cuts, ph, base=base)
        assert not bad.any(), (ph, name)
        for j, i in enumerate(ops):
            assert rows[j].tobytes() == want[i], (ph, name, i, len(msgs[i]), cuts[j][:4])
            assert np.array_equal(rows[j], one_shot[i]), (ph, name, i)
    # init then final: the empty message
    rows, bad = m.prehash_stream(70, ph).final()
    assert not host(bad).any() and all(r.tobytes() == hash_message(b"", ph) for r in host(rows))


@pytest.mark.parametrize("ph", PHS)
def test_stream_65536_ops_random_lengths_1_3_16_updates(sets, ph):
    m = sets[44]
    rng = np.random.default_rng(11)
    n = 65536
    lens = rng.integers(0, 2049, n)
    buf = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    want, bad1 = m.prehash_device(dev(buf), dev_off(off), n, ph)  # tied to hashlib by test_prehash_seam_65536_random_lengths
    want = host(want)
    assert not host(bad1).any()
    for i in (0, 1, 777, n - 1):
        assert want[i].tobytes() == hash_message(buf[int(off[i]):int(off[i + 1])].tobytes(), ph)
    for U in (1, 3, 16):
        cuts = cases.random_cuts(lens, U, np.random.default_rng(100 + U))
        st = m.prehash_stream(n, ph)
        for u in range(U):
            flat, poff = cases.gather_pieces(buf, off, cuts, u)
            st.update(dev(np.concatenate([flat, np.zeros(8, np.uint8)])), dev_off(poff))
        rows, bad = st.final()
        rows = host(rows)
        assert not host(bad).any()
        diff = np.nonzero((rows != want).any(axis=1))[0]
        assert diff.size == 0, (ph, U, diff[:8], lens[diff[:8]], cuts[diff[:8]])


@pytest.mark.parametrize("ph", PHS)
def test_stream_refusals_are_per_op_sticky_and_stay_inside_state_and_pieces(sets, ph):
    m = sets[44]
    lib, code = _ph_lib.load(), m._ph_arg(ph)
    n = 4096
    rng = np.random.default_rng(21)
    parts = [[rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(1, 200, n)] for _ in range(3)]
    tabs = [table(p) for p in parts]
    t = tabs[1][1].copy()
    k1, k2, k3 = 1000, 2000, 3000
    t[k1 + 1] = t[k1] - np.uint64(1)                                   # decreasing
    t[k2 + 1] = np.uint64(1) << np.uint64(60)                          # overshooting
    t[k3] = np.uint64(2 ** 64 - 8); t[k3 + 1] = np.uint64(2 ** 64 - 1)  # wrapping
    okp = pairs_ok(t)
    assert 3 <= (~okp).sum() <= 8 and not okp[k1] and not okp[k2] and not okp[k3]
    named = [tabs[1][0][int(t[i]):int(t[i + 1])].tobytes() if okp[i] else b"" for i in range(n)]
    # state and pieces inside canary-filled over-allocations
    G = 4096
    nb = lib.mldsa_ph_state_bytes(code, n)
    state = torch.full((nb + 2 * G,), 0xC3, dtype=torch.uint8, device="cuda")
    sptr = C.c_void_p(state.data_ptr() + G)
    strm = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pbufs = []
    for u in range(3):
        body = tabs[u][0][:int(tabs[u][1][-1])]
        pbufs.append(dev(np.concatenate([np.full(G, 0x3C, np.uint8), body, np.full(G, 0x3C, np.uint8)])))
    _ph_lib.check(lib.mldsa_ph_init(m.hp._h, code, sptr, nb, n, strm))
    for u in range(3):
        table_u = t if u == 1 else tabs[u][1]
        _ph_lib.check(lib.mldsa_ph_update(m.hp._h, code, sptr, nb, C.c_void_p(pbufs[u].data_ptr() + G), _ptr(dev_off(table_u)), n, strm))
    rows = torch.full((n, lib.mldsa_ph_row_len(code)), 0x77, dtype=torch.uint8, device="cuda")
    bad = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    _ph_lib.check(lib.mldsa_ph_final(m.hp._h, code, sptr, nb, _ptr(rows), _ptr(out_off), _ptr(bad), n, strm))
    rows, bad, state_h = host(rows), host(bad), host(state)
    assert np.array_equal(bad.astype(bool), ~okp)
    assert not rows[~okp].any()                                   # bad in update 2 stays bad through update 3
    for i in np.nonzero(okp)[0]:
        assert rows[i].tobytes() == hash_message(parts[0][i] + named[i] + parts[2][i], ph), (ph, i)
    assert np.array_equal(host(out_off), np.arange(n + 1, dtype=np.int64) * rows.shape[1])
    assert (state_h[:G] == 0xC3).all() and (state_h[G + nb:] == 0xC3).all()  # nothing outside state_bytes was written
    assert (state_h[G:G + nb] != 0xC3).any()
    for u in range(3):
        p = host(pbufs[u])
        assert (p[:G] == 0x3C).all() and (p[-G:] == 0x3C).all()
        assert np.array_equal(p[G:-G], tabs[u][0][:int(tabs[u][1][-1])])
    # a NULL `pieces` with a non-empty pair marks the op bad and reads nothing; short state_bytes is refused before a launch
    st = m.prehash_stream(4, ph)
    st.update(None, dev_off(np.array([0, 0, 3, 3, 3], dtype=np.uint64)))
    r, b = st.final()
    assert list(host(b)) == [0, 1, 0, 0] and not host(r)[1].any() and host(r)[0].tobytes() == hash_message(b"", ph)
    assert lib.mldsa_ph_update(m.hp._h, code, sptr, nb - 1, C.c_void_p(pbufs[0].data_ptr() + G), _ptr(dev_off(tabs[0][1])), n, strm) == _lib.ERR_PARAM
    assert lib.mldsa_ph_update(m.hp._h, code, sptr, nb, C.c_void_p(pbufs[0].data_ptr() + G), NULL, n, strm) == _lib.ERR_PARAM
    assert lib.mldsa_ph_final(m.hp._h, code, sptr, nb, NULL, NULL, NULL, n, strm) == _lib.ERR_PARAM


HOST_LENS = (0, 1, 63, 64, 65, 167, 168, 4095, 4096, 4097, 5000, 12289, 200 << 10, 3, 9000, 128, 100, 2, 70000, 31, 8192, 777, 1, 0)
STAGINGS = (4096, 64 << 20, 0)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_hash_host_calls_match_oracle_and_existing_paths(sets, pset):
    m = sets[pset]
    rng = np.random.default_rng(500 + pset)
    n, nk = len(HOST_LENS), 3
    msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in HOST_LENS]
    ctx_lens = [0, 255, 1, 17, 64, 0, 200, 3] * 3
    ctxs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in ctx_lens]
    rnd = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    # the sizes guarantee what the 4 096-byte staging is meant to exercise
    offs = np.concatenate([[0], np.cumsum(HOST_LENS)])
    assert any((offs[i + 1] - 1) // 4096 - offs[i] // 4096 >= 2 for i in range(n) if HOST_LENS[i])          # a message in >= 3 chunks
    for blk in (64, 128, 168):                                                                              # a chunk boundary strictly
        assert any((c - offs[i]) % blk for i in range(n) for c in range(4096, int(offs[-1]), 4096) if offs[i] < c < offs[i + 1]), blk
    keys = [orc.keygen_from_seed(pset, bytes([pset, k + 7]) * 16) for k in range(nk)]
    pk_b = np.frombuffer(b"".join(orc.pk_into_bytes(pset, pk) for pk, _ in keys), dtype=np.uint8)
    sk_b = np.frombuffer(b"".join(orc.sk_into_bytes(pset, sk) for _, sk in keys), dtype=np.uint8)
    kidx = (np.arange(n) * 2 % nk).astype(np.uint32)
    sks_dev = m.private_keys_from_bytes([orc.sk_into_bytes(pset, sk) for _, sk in keys])
    mflat, moff = m._cat_host(msgs)
    rn = np.frombuffer(b"".join(rnd), dtype=np.uint8)
    for ph in PHS:
        want = [orc.hash_sign(pset, keys[kidx[i]][1], msgs[i], rnd[i], ctxs[i], ph) for i in range(n)]
        existing = host(m.try_hash_sign_with_seed(sks_dev, msgs, rnd, ctxs=ctxs, ph=ph, key_idx=kidx, prehash="host"))
        assert [r.tobytes() for r in existing] == want
        # verify batch: good, damaged signatures, damaged messages, one |ctx| = 256
        v_sigs = [bytearray(s) for s in want]
        v_msgs, v_ctxs = list(msgs), list(ctxs)
        v_sigs[2][40] ^= 4
        v_sigs[12][-1] ^= 0x80
        v_msgs[4] = v_msgs[4][:-1] + bytes([v_msgs[4][-1] ^ 1])
        big = bytearray(v_msgs[18]); big[4096 * 9 + 5] ^= 0x40       # a byte deep inside a message of many chunks
        v_msgs[18] = bytes(big)
        v_msgs[0] = b"\x00"                                          # the empty message replaced
        v_ctxs[6] = bytes(256)
        exp = [orc.hash_verify(pset, keys[kidx[i]][0], v_msgs[i], bytes(v_sigs[i]), v_ctxs[i], ph) for i in range(n)]
        assert sum(exp) == n - 6 and not any(exp[i] for i in (0, 2, 4, 6, 12, 18))
        sg = np.frombuffer(b"".join(bytes(s) for s in v_sigs), dtype=np.uint8)
        vflat, voff = m._cat_host(v_msgs)
        pin_m, mflat_p = _host_alloc(m, mflat)
        pin_v, vflat_p = _host_alloc(m, vflat)
        try:
            for staging in STAGINGS:
                for pinned in (False, True):
                    got = m.hash_sign_host(sk_b, (mflat_p if pinned else mflat, moff), rn, ctxs=ctxs, ph=ph, key_idx=kidx, staging_bytes=staging)
                    assert [r.tobytes() for r in got] == want, (pset, ph, staging, pinned)
                    ok = m.hash_verify_host(pk_b, (vflat_p if pinned else vflat, voff), sg, ctxs=v_ctxs, ph=ph, key_idx=kidx, staging_bytes=staging)
                    assert list(ok) == exp, (pset, ph, staging, pinned)
        finally:
            m.lib.mldsa_host_free(pin_m)
            m.lib.mldsa_host_free(pin_v)
    # identity mapping (op i uses key i) and no ctxs, on the last PH
    pk_i, sk_i = pk_b.reshape(nk, -1)[kidx[:8]].copy(), sk_b.reshape(nk, -1)[kidx[:8]].copy()
    want8 = [orc.hash_sign(pset, keys[kidx[i]][1], msgs[i], rnd[i], b"", ph) for i in range(8)]
    got = m.hash_sign_host(sk_i, msgs[:8], rn[:8 * 32], ph=ph, staging_bytes=4096)
    assert [r.tobytes() for r in got] == want8
    assert m.hash_verify_host(pk_i, msgs[:8], got, ph=ph, staging_bytes=4096).all()
    # a |ctx| = 256 op in a signing batch is the core's MLDSA_ERR_CTX_LEN
    with pytest.raises(ValueError):
        m.hash_sign_host(sk_b, msgs[:2], rn[:64], ctxs=[b"", bytes(256)], ph=ph, key_idx=kidx[:2])
    # a malformed msg_off fails the whole call before a message byte is read
    lib = _ph_lib.load()
    bad_off = moff.copy()
    bad_off[5] = bad_off[4] - np.uint64(1)
    okb = np.full(n, 7, dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    h = m._ph_host(0)
    sg = np.frombuffer(b"".join(want), dtype=np.uint8)
    assert lib.mldsa_hash_verify_host(h, pset, 0, vp(pk_b), nk, vp(kidx), vp(mflat), vp(bad_off), NULL, NULL, vp(sg), vp(okb), n) == _lib.ERR_PARAM
    assert lib.mldsa_ph_last_error() and (okb == 7).all()
    sgo, sto = np.full(n * m.SIG_LEN, 7, dtype=np.uint8), np.full(n, 7, dtype=np.int32)
    assert lib.mldsa_hash_sign_host(h, pset, 0, vp(sk_b), nk, vp(kidx), vp(mflat), vp(bad_off), NULL, NULL, vp(rn), vp(sgo), vp(sto),
                                    n) == _lib.ERR_PARAM
    assert (sgo == 7).all() and (sto == 7).all()
    with pytest.raises(ValueError):
        m.hash_verify_host(pk_b, (mflat, bad_off), sg, ph="SHA256", key_idx=kidx)


def test_hash_verify_host_65536_ops_of_1_kib(sets):
    m = sets[65]
    rng = np.random.default_rng(9)
    n, nk = 65536, 16
    xi = np.frombuffer(b"".join(shake(b"phs-key", i) for i in range(nk)), dtype=np.uint8)
    pk, sk = m.keygen_host(xi)
    kidx = (np.arange(n) % nk).astype(np.uint32)
    mflat = rng.integers(0, 256, n * 1024, dtype=np.uint8)
    moff = (np.arange(n + 1, dtype=np.uint64) * np.uint64(1024))
    rn = np.zeros(n * 32, dtype=np.uint8)
    sig = m.hash_sign_host(sk, (mflat, moff), rn, ph="SHA256", key_idx=kidx).copy()
    damaged = rng.choice(n, 300, replace=False)
    sig[damaged, rng.integers(0, m.SIG_LEN, 300)] ^= 0x10
    bad_msg = np.setdiff1d(rng.choice(n, 200, replace=False), damaged)
    mflat[bad_msg * 1024 + rng.integers(0, 1024, bad_msg.size)] ^= 1
    got = m.hash_verify_host(pk, (mflat, moff), sig, ph="SHA256", key_idx=kidx)
    raw = mflat.tobytes()
    msgs = [raw[i * 1024:(i + 1) * 1024] for i in range(n)]
    ref = m.hash_verify(m.public_keys_from_bytes(torch.from_numpy(pk).cuda()), msgs, torch.from_numpy(sig).cuda(), ph="SHA256", key_idx=kidx,
                        prehash="host")
    assert np.array_equal(got, ref) and (~got).sum() == 300 + bad_msg.size


def test_two_prehash_streams_interleaved_and_no_host_synchronisation(sets):
    m = sets[65]
    n = 4096
    rng = np.random.default_rng(31)
    phs = ("SHA512", "SHAKE128")
    data = []
    for j in range(2):
        halves = [[rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 700, n)] for _ in range(2)]
        tabs = [table(h) for h in halves]
        data.append((halves, [(dev(t[0]), dev_off(t[1])) for t in tabs]))
    want = [[hash_message(data[j][0][0][i] + data[j][0][1][i], phs[j]) for i in range(n)] for j in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    st = [None, None]
    for j in range(2):
        with torch.cuda.stream(streams[j]):
            st[j] = m.prehash_stream(n, phs[j])
    for u in range(2):              # interleaved: a0 b0 a1 b1
        for j in range(2):
            with torch.cuda.stream(streams[j]):
                st[j].update(*data[j][1][u])
    out = []
    for j in range(2):
        with torch.cuda.stream(streams[j]):
            out.append(st[j].final())
    for j in range(2):
        streams[j].synchronize()
        assert not out[j][1].cpu().numpy().any()
        assert [r.tobytes() for r in out[j][0].cpu().numpy()] == want[j], phs[j]
    # update only enqueues: behind a long spin on its stream it returns while that stream is still busy
    s = streams[0]
    with torch.cuda.stream(s):
        torch.cuda._sleep(1_000_000_000)
        st2 = m.prehash_stream(n, phs[0])
        st2.update(*data[0][1][0])
        st2.update(*data[0][1][1])
        rows, bad = st2.final()
        busy = not s.query()
    s.synchronize()
    assert busy and [r.tobytes() for r in rows.cpu().numpy()] == want[0]
