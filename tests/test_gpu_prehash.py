"""HashML-DSA with the pre-hash on the GPU (include/mldsa_ph.h): the seam against hashlib, signatures and verdicts against the
oracle and the host pre-hash path, the per-op boundary and stream behaviour."""
import ctypes as C

from gpu_common import *  # noqa: F401,F403

from fips204_amd import _lib, _ph_lib
from fips204_amd.hotpath import _ptr
from fips204_amd.ml_dsa import _cat_with_offsets, hash_message

pytestmark = pytest.mark.gpu

PHS = ("SHA256", "SHA512", "SHAKE128")
EDGES = {"SHA256": (0, 1, 55, 56, 63, 64, 65, 119, 120), "SHA512": (111, 112, 127, 128, 239, 240), "SHAKE128": (167, 168, 169, 335, 336)}
NULL = C.c_void_p(0)


def _rows(m, buf, off, n, ph, base=0):
    """prehash_device over buf[base:] with the table `off` (numpy uint64): (rows, bad) on the host"""
    d = dev(buf)
    rows, bad = m.prehash_device(d[base:], dev_off(off), n, ph)
    return host(rows), host(bad)


def _expected(msgs, ph):
    return [hash_message(x, ph) for x in msgs]


@pytest.mark.parametrize("ph", PHS)
def test_prehash_seam_matches_hashlib(sets, ph):
    """every padding edge of the three PH, lanes of one wave with very different lengths, no message dword-aligned, two 4 MiB
    messages among short ones: rows = hash_message(m, ph) byte for byte"""
    m = sets[65]
    rng = np.random.default_rng(7)
    lens = [n for p in PHS for n in EDGES[p]]
    lens += list(rng.integers(0, 3000, 200)) + [4 << 20, 5, 4 << 20, 0]
    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    want = _expected(msgs, ph)
    for base in (1, 2, 3):
        skew = 5  # off[0] odd: the messages start at base + 5 + ...
        flat = bytes(base + skew) + b"".join(msgs) + bytes(8)
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        off[0] = skew
        np.cumsum([len(x) for x in msgs], out=off[1:])
        off[1:] += np.uint64(skew)
        rows, bad = _rows(m, np.frombuffer(flat, dtype=np.uint8), off, len(msgs), ph, base=base)
        assert not bad.any()
        for i, w in enumerate(want):
            assert rows[i].tobytes() == w, (ph, base, i, lens[i])


@pytest.mark.parametrize("ph", PHS)
def test_prehash_seam_65536_random_lengths(sets, ph):
    m = sets[44]
    rng = np.random.default_rng(11)
    n = 65536
    lens = rng.integers(0, 2049, n)
    buf = rng.integers(0, 256, int(lens.sum()) + 16, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    rows, bad = _rows(m, buf, off, n, ph)
    assert not bad.any()
    raw = buf.tobytes()
    for i in range(n):
        assert rows[i].tobytes() == hash_message(raw[int(off[i]):int(off[i + 1])], ph), (ph, i)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_hash_sign_device_matches_oracle_and_host_path(sets, pset):
    m = sets[pset]
    rng = np.random.default_rng(100 + pset)
    keys = [orc.keygen_from_seed(pset, bytes([pset, k]) * 16) for k in range(2)]
    sks = m.private_keys_from_bytes([orc.sk_into_bytes(pset, sk) for _, sk in keys])
    n = 6
    kidx = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint32)
    msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 1, 64, 135, 1000, 5000)]
    rnd = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    for ctxs in (None, [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 255, 3, 17, 1, 64)]):
        for ph in PHS:
            got = host(m.try_hash_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, ph=ph, key_idx=kidx, prehash="device"))
            ref = host(m.try_hash_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, ph=ph, key_idx=kidx, prehash="host"))
            assert np.array_equal(got, ref), (ph, ctxs is None)
            for i in range(n):
                ctx = ctxs[i] if ctxs else b""
                want = orc.sign_internal(pset, keys[kidx[i]][1], hash_message(msgs[i], ph), rnd[i], ctx=ctx, mode=2)
                assert got[i].tobytes() == want, (ph, i)
    # the reference's own case (src/lib.rs:539-540)
    message1 = bytes([0, 1, 2, 3, 4, 5, 6, 7])
    pk_o, sk_o = orc.keygen_from_seed(pset, bytes([0x11] * 32))
    sks1 = m.private_keys_from_bytes([orc.sk_into_bytes(pset, sk_o)])
    pks1 = m.public_keys_from_bytes([orc.pk_into_bytes(pset, pk_o)])
    sig = m.try_hash_sign_with_seed(sks1, [message1], [bytes([34] * 32)], ctxs=[b""], ph="SHA256", prehash="device")
    assert host(sig)[0].tobytes() == orc.hash_sign(pset, sk_o, message1, bytes([34] * 32), b"", "SHA256")
    assert m.hash_verify(pks1, [message1], sig, ctxs=[b""], ph="SHA256", prehash="device").all()


@pytest.mark.parametrize("pset", [44, 87])
def test_hash_verify_device_matches_oracle(sets, pset):
    m = sets[pset]
    rng = np.random.default_rng(300 + pset)
    pk_o, sk_o = orc.keygen_from_seed(pset, bytes(range(1, 33)))
    pks = m.public_keys_from_bytes([orc.pk_into_bytes(pset, pk_o)])
    pk_bytes = torch.from_numpy(np.frombuffer(orc.pk_into_bytes(pset, pk_o), dtype=np.uint8).copy()).cuda().view(1, -1)
    n = 12
    msgs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 400, n)]
    ctxs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 20, n)]
    signed_ph = ["SHA256", "SHA512", "SHAKE128"] * 4
    sigs = [bytearray(orc.hash_sign(pset, sk_o, msgs[i], bytes(32), ctxs[i], signed_ph[i])) for i in range(n)]
    v_ph, v_msgs, v_ctxs = list(signed_ph), list(msgs), list(ctxs)
    sigs[1][10] ^= 1                                       # damaged signature
    v_ph[2] = "SHA512" if signed_ph[2] != "SHA512" else "SHA256"  # wrong PH
    v_ctxs[4] = v_ctxs[4] + b"x"                           # wrong ctx
    v_msgs[5] = (bytes([v_msgs[5][0] ^ 0x80]) + v_msgs[5][1:]) if v_msgs[5] else b"\x01"  # damaged message byte
    want = [orc.hash_verify(pset, pk_o, v_msgs[i], bytes(sigs[i]), v_ctxs[i], v_ph[i]) for i in range(n)]
    assert want[0] and not any(want[j] for j in (1, 2, 4, 5))
    # one call per PH with every op in it: an op signed under another PH must come out false
    for ph in PHS:
        exp = [orc.hash_verify(pset, pk_o, v_msgs[i], bytes(sigs[i]), v_ctxs[i], ph) for i in range(n)]
        sg = torch.from_numpy(np.frombuffer(b"".join(bytes(s) for s in sigs), dtype=np.uint8).copy()).cuda().view(n, -1)
        got = m.hash_verify(pks, v_msgs, sg, ctxs=v_ctxs, ph=ph, key_idx=np.zeros(n, np.uint32), prehash="device")
        assert list(got) == exp, ph
        mb, mo = _cat_with_offsets(v_msgs, m.device)
        cb, co = _cat_with_offsets(v_ctxs, m.device)
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        m.hash_verify_pk_device(pk_bytes, mb, mo, sg, ok, n, ph, cb, co, key_idx=torch.zeros(n, dtype=torch.int32, device="cuda"))
        assert list(host(ok).astype(bool)) == exp, ph


def test_hash_verify_65536_ops_against_host_path(sets):
    m = sets[44]
    rng = np.random.default_rng(5)
    n, nk = 65536, 16
    xi = [shake(b"ph-key", i) for i in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    kidx = (np.arange(n) % nk).astype(np.uint32)
    lens = rng.integers(0, 300, n)
    raw = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
    off = np.concatenate([[0], np.cumsum(lens)])
    msgs = [raw[off[i]:off[i + 1]] for i in range(n)]
    rnd = [bytes(32)] * n
    sig = m.try_hash_sign_with_seed(sks, msgs, rnd, ph="SHAKE128", key_idx=kidx, prehash="device")
    sig_h = host(sig).copy()
    damaged = rng.choice(n, 500, replace=False)
    sig_h[damaged, rng.integers(0, m.SIG_LEN, 500)] ^= 0x10
    sg = torch.from_numpy(sig_h).cuda()
    got = m.hash_verify(pks, msgs, sg, ph="SHAKE128", key_idx=kidx, prehash="device")
    ref = m.hash_verify(pks, msgs, sg, ph="SHAKE128", key_idx=kidx, prehash="host")
    assert np.array_equal(got, ref) and (~got).sum() == 500


def test_malformed_message_pairs_refuse_only_their_own_ops(sets):
    m = sets[44]
    n, nk = 4096, 4
    xi = [shake(b"ph-bnd", i) for i in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    kidx = (np.arange(n) % nk).astype(np.uint32)
    kd = torch.from_numpy(kidx.view(np.int32)).cuda()
    msgs = [shake(b"ph-bnd-msg", i, 1 + i % 97) for i in range(n)]
    rnd = [shake(b"ph-bnd-rnd", i) for i in range(n)]
    buf, off = table(msgs)
    t = off.copy()
    k1, k2 = 1000, 3000
    t[k1 + 1] = t[k1] - np.uint64(1)           # decreasing
    t[k2 + 1] = np.uint64(1) << np.uint64(60)  # past the end
    okp = pairs_ok(t)
    assert (~okp).sum() >= 3 and okp.sum() > n - 6
    mb, mo = dev(buf), dev_off(t)
    rn = torch.from_numpy(np.frombuffer(b"".join(rnd), dtype=np.uint8).copy()).cuda().view(n, 32)
    for ph in ("SHA256", "SHAKE128"):
        sg = torch.full((n, m.SIG_LEN), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        m.hash_sign_device(sks, mb, mo, rn, sg, n, ph, key_idx=kd, status=st)
        sg_h, st_h = host(sg), host(st)
        # the ops whose pair is well formed sign the bytes it names
        named = [buf[int(t[i]):int(t[i + 1])].tobytes() if okp[i] else b"" for i in range(n)]
        ref = host(m.try_hash_sign_with_seed(sks, named, rnd, ph=ph, key_idx=kidx, prehash="host"))
        assert np.array_equal(st_h[okp], np.zeros(okp.sum(), np.int32))
        assert np.array_equal(sg_h[okp], ref[okp])
        assert (st_h[~okp] == _lib.ERR_PARAM).all() and not sg_h[~okp].any()
        pk0 = orc.pk_try_from_bytes(44, host(pk)[kidx[k1 - 1]].tobytes())
        assert orc.hash_verify(44, pk0, named[k1 - 1], sg_h[k1 - 1].tobytes(), b"", ph)
        ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        m.hash_verify_device(pks, mb, mo, torch.from_numpy(ref).cuda(), ok, n, ph, key_idx=kd)
        ok_h = host(ok)
        assert (ok_h[okp] == 1).all() and (ok_h[~okp] == 0).all()
        rows, bad = m.prehash_device(mb, mo, n, ph)
        assert np.array_equal(host(bad).astype(bool), ~okp) and not host(rows)[~okp].any()


def test_ctx_too_long_and_argument_errors(sets):
    m = sets[44]
    lib = _ph_lib.load()
    xi = [shake(b"ph-arg", 0)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    n = 3
    big = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    off = np.array([0, 10, (64 << 20) - 1, 64 << 20], dtype=np.uint64)  # op 1 names a 64 MiB region
    ctxs = [b"a", bytes(256), b""]
    cb, co = _cat_with_offsets(ctxs, m.device)
    rn = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    sg = torch.full((n, m.SIG_LEN), 1, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    mo = dev_off(off)
    kd = torch.zeros(n, dtype=torch.int32, device="cuda")
    m.hash_sign_device(sks, big, mo, rn, sg, n, "SHA512", cb, co, key_idx=kd, status=st)
    st_h, sg_h = host(st), host(sg)
    assert list(st_h) == [0, _lib.ERR_CTX_LEN, 0] and not sg_h[1].any()
    ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    m.hash_verify_device(pks, big, mo, sg, ok, n, "SHA512", cb, co, key_idx=kd)
    assert list(host(ok)) == [1, 0, 1]
    # argument errors: MLDSA_ERR_PARAM before a launch; n_ops = 0 is MLDSA_OK
    scratch = torch.empty(lib.mldsa_ph_scratch_bytes(1, n), dtype=torch.uint8, device="cuda")
    strm = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda ph, sc, nb, msgs=big: (m.hp._h, 44, ph, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), 1, _ptr(kd),
                                         _ptr(msgs) if msgs is not None else NULL, _ptr(mo), _ptr(cb), _ptr(co), _ptr(sg), _ptr(ok), n, sc, nb, strm)
    assert lib.mldsa_hash_verify(*args(9, _ptr(scratch), scratch.numel())) == _lib.ERR_PARAM
    assert lib.mldsa_hash_verify(*args(1, _ptr(scratch), scratch.numel() - 1)) == _lib.ERR_PARAM
    assert lib.mldsa_hash_verify(*args(1, NULL, scratch.numel())) == _lib.ERR_PARAM
    a = list(args(1, _ptr(scratch), scratch.numel()))
    a[3] = NULL
    assert lib.mldsa_hash_verify(*a) == _lib.ERR_PARAM
    a = list(args(1, _ptr(scratch), scratch.numel()))
    a[14] = 0
    assert lib.mldsa_hash_verify(*a) == _lib.OK
    assert lib.mldsa_hash_sign(m.hp._h, 44, 1, *([NULL] * 6), 1, NULL, NULL, _ptr(mo), NULL, NULL, NULL, _ptr(sg), NULL, n,
                               _ptr(scratch), scratch.numel(), strm) == _lib.ERR_PARAM
    assert lib.mldsa_prehash(m.hp._h, 3, _ptr(big), _ptr(mo), _ptr(sg), NULL, n, strm) == _lib.ERR_PARAM
    assert lib.mldsa_prehash(m.hp._h, 0, _ptr(big), NULL, _ptr(sg), NULL, n, strm) == _lib.ERR_PARAM
    with pytest.raises(ValueError):
        m.try_hash_sign_with_seed(sks, [b"x"], [bytes(32)], ctxs=[bytes(256)], ph="SHA256", prehash="device")
    with pytest.raises(ValueError):
        m.hash_verify(pks, [b"x"], [bytes(m.SIG_LEN)], ph="SHA256", prehash="gpu")
    # the context still signs and verifies
    sig = m.try_hash_sign_with_seed(sks, [b"after"], [bytes(32)], ph="SHA256", prehash="device")
    assert m.hash_verify(pks, [b"after"], sig, ph="SHA256", prehash="device").all()
    assert m.verify(pks, [b"after"], m.try_sign_with_seed(sks, [b"after"], [bytes(32)])).all()


def test_two_streams_and_no_host_synchronisation(sets):
    m = sets[65]
    n, nk = 2048, 4
    xi = [shake(b"ph-strm", i) for i in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    kd = torch.from_numpy((np.arange(n) % nk).astype(np.int32)).cuda()
    batches = []
    for j in range(2):
        msgs = [shake(b"ph-strm-msg%d" % j, i, 50 + (i * 7) % 900) for i in range(n)]
        mb, mo = _cat_with_offsets(msgs, m.device)
        rn = torch.from_numpy(np.frombuffer(b"".join(shake(b"r%d" % j, i) for i in range(n)), dtype=np.uint8).copy()).cuda().view(n, 32)
        batches.append((mb, mo, rn))
    ph = ["SHA512", "SHAKE128"]
    seq = []
    for j in range(2):
        sg = torch.zeros((n, m.SIG_LEN), dtype=torch.uint8, device="cuda")
        m.hash_sign_device(sks, *batches[j][:2], batches[j][2], sg, n, ph[j], key_idx=kd)
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        m.hash_verify_device(pks, *batches[j][:2], sg, ok, n, ph[j], key_idx=kd)
        torch.cuda.synchronize()
        seq.append((sg, ok))
        assert host(ok).all()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    out = []
    for j in range(2):
        with torch.cuda.stream(streams[j]):
            ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
            m.hash_verify_device(pks, *batches[j][:2], seq[j][0], ok, n, ph[j], key_idx=kd)
            out.append(ok)
    for j in range(2):
        streams[j].synchronize()
        assert torch.equal(out[j], seq[j][1])
    # a verify call only enqueues: behind a long spin on its stream it returns while that stream is still busy
    s = streams[0]
    with torch.cuda.stream(s):
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda._sleep(1_000_000_000)
        m.hash_verify_device(pks, *batches[0][:2], seq[0][0], ok, n, ph[0], key_idx=kd)
        busy = not s.query()
    s.synchronize()
    assert busy and torch.equal(ok, seq[0][1])
