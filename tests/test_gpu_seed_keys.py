"""Private keys in seed form on the device (include/mldsa_seed.h): mldsa_seed_expand against the ACVP keyGen vectors and against
mldsa_keygen -> mldsa_sk_expand field by field, mldsa_seed_check on damaged keys and seeds, mldsa_sign_seed against mldsa_sign byte for
byte, across passes, refusals and streams, the zeroed scratch behind each of them, and the Python layer on top."""
from gpu_common import *  # noqa: F401,F403
from gpu_common import C, dev, dev_off, filled, hashlib, host, kidx_dev, nonzero_bytes, np, orc, pytest, shake, table, torch

from conftest import PSET
from fips204_amd import _lib, _seed_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PREHASH, MODE_PURE, PH_SHA512, PrivateKeys, _cat_with_offsets, hash_message

pytestmark = pytest.mark.gpu

SETS = (44, 65, 87)
SIZES = (1, 63, 64, 65, 200)  # below, at and past one wave of seeds; 200 = four passes of the 64-key minimum
NULL = C.c_void_p(0)
Q = 8380417


def u8(rows, width):
    return torch.frombuffer(bytearray(b"".join(rows) or bytes(width)), dtype=torch.uint8).cuda().view(-1, width)


def scratch_bytes(m, n, what="expand"):
    lib = _seed_lib.load()
    return {"expand": lib.mldsa_seed_expand_scratch_bytes, "check": lib.mldsa_seed_check_scratch_bytes,
            "sign": lib.mldsa_seed_sign_scratch_bytes}[what](m.pset, n)


# ------------------------------------------------------------------------------------------------- the parent route, once per set
_PARENT = {}


def parent(m, pset):
    """200 SHAKE-derived seeds of a set through mldsa_keygen -> mldsa_sk_expand, computed once; the tests slice it and never write it"""
    if pset not in _PARENT:
        n = max(SIZES)
        xi = [shake(b"seed-key%d" % pset, i) for i in range(n)]
        pk, sk = m.keygen_from_seed(xi)
        sks = m.private_keys_from_bytes(sk)
        _PARENT[pset] = dict(xi=xi, xi_dev=u8(xi, 32), pk=host(pk).copy(), sk=host(sk).copy(), sks=sks,
                             fields={f: host(getattr(sks, f)).copy() for f in ("rho", "cap_k", "tr", "s_1_hat_mont", "s_2_hat_mont", "t_0_hat_mont")})
    return _PARENT[pset]


CANARY_U8, CANARY_I32 = 0xA5, -7


def raw_expand(m, xi_dev, n, scratch, sb=None, want_pk=True, expect=_lib.OK):
    """mldsa_seed_expand into buffers with a canary row on either side; returns the fields as numpy (pk None when not asked for)"""
    k, l = m.params.k, m.params.l
    shapes = dict(rho=(32,), cap_k=(32,), tr=(64,), s_1_hat_mont=(l, 256), s_2_hat_mont=(k, 256), t_0_hat_mont=(k, 256), pk=(m.PK_LEN,))
    bufs = {}
    for f, shp in shapes.items():
        i32 = f.endswith("mont")
        bufs[f] = torch.full((n + 2,) + shp, CANARY_I32 if i32 else CANARY_U8, dtype=torch.int32 if i32 else torch.uint8, device="cuda")
    rc = _seed_lib.load().mldsa_seed_expand(
        m.hp._h, m.pset, _ptr(xi_dev), _ptr(bufs["rho"][1:]), _ptr(bufs["cap_k"][1:]), _ptr(bufs["tr"][1:]), _ptr(bufs["s_1_hat_mont"][1:]),
        _ptr(bufs["s_2_hat_mont"][1:]), _ptr(bufs["t_0_hat_mont"][1:]), _ptr(bufs["pk"][1:]) if want_pk else NULL, n, _ptr(scratch),
        scratch.numel() if sb is None else sb, _stream(m.device))
    assert rc == expect, (rc, _seed_lib.load().mldsa_seed_last_error())
    out = {}
    for f, t in bufs.items():
        h = host(t)
        can = CANARY_I32 if f.endswith("mont") else CANARY_U8
        assert (h[0] == can).all() and (h[-1] == can).all(), f"canary behind {f}"
        if rc != _lib.OK or (f == "pk" and not want_pk):
            assert (h == can).all(), f"{f} was written"
        out[f] = h[1:-1]
    if not want_pk:
        out["pk"] = None
    return out


def assert_same_key(got, par, n):
    for f in ("rho", "cap_k", "tr"):
        assert np.array_equal(got[f], par["fields"][f][:n]), f
    if got["pk"] is not None:
        assert np.array_equal(got["pk"], par["pk"][:n]), "pk"
    for f in ("s_1_hat_mont", "s_2_hat_mont", "t_0_hat_mont"):
        a, b = got[f].astype(np.int64), par["fields"][f][:n].astype(np.int64)
        assert not ((a - b) % Q).any(), f"{f} differs modulo q"
        assert (np.abs(a) < Q).all(), f"{f} leaves (-q, q), the range include/mldsa_seed.h states"


# ------------------------------------------------------------------------------------------------------------------ 1: ACVP
def test_seed_expand_reproduces_the_acvp_keygen_vectors(sets, acvp_keygen):
    seen = set()
    for grp in acvp_keygen["testGroups"]:
        pset = PSET[grp["parameterSet"]]
        m = sets[pset]
        tests = grp["tests"]
        n = len(tests)
        xi = u8([bytes.fromhex(t["seed"]) for t in tests], 32)
        scratch = filled(scratch_bytes(m, n))
        sks, pk = m.expand_seeds_device(xi, want_pk=True, scratch=scratch)
        sk = host(m.private_keys_into_bytes(sks))
        pk = host(pk)
        for i, t in enumerate(tests):
            assert sk[i].tobytes() == bytes.fromhex(t["sk"]), (pset, t["tcId"], "sk")
            assert pk[i].tobytes() == bytes.fromhex(t["pk"]), (pset, t["tcId"], "pk")
        assert nonzero_bytes(m, scratch) == 0
        seen.add(pset)
    assert seen == set(SETS)


# --------------------------------------------------------------------------------------------- 2: parity with the parent route
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", SETS)
def test_seed_expand_equals_keygen_then_sk_expand(sets, pset, n):
    m = sets[pset]
    par = parent(m, pset)
    xi = par["xi_dev"][:n].contiguous()
    one_pass, least = scratch_bytes(m, n), scratch_bytes(m, min(n, 64))
    # a scratch of exactly one pass
    scratch = filled(one_pass)
    assert scratch.numel() == one_pass
    got = raw_expand(m, xi, n, scratch)
    assert_same_key(got, par, n)
    assert nonzero_bytes(m, scratch) == 0, "the scratch is not all zero after mldsa_seed_expand"
    # the 64-key minimum: ceil(n / 64) passes, identical outputs
    scratch = filled(least)
    got_min = raw_expand(m, xi, n, scratch, sb=least)
    for f in got:
        assert np.array_equal(got_min[f], got[f]), f
    assert nonzero_bytes(m, scratch) == 0
    # one byte below the minimum: refused before anything is launched, outputs and scratch untouched
    scratch_nomem = filled(least)
    raw_expand(m, xi, n, scratch_nomem, sb=least - 1, expect=_lib.ERR_NOMEM)
    assert b"scratch" in _seed_lib.load().mldsa_seed_last_error()
    assert bool((scratch_nomem == 0x5A).all())
    # without pk
    scratch = filled(one_pass)
    got_nopk = raw_expand(m, xi, n, scratch, want_pk=False)
    for f in got:
        if f != "pk":
            assert np.array_equal(got_nopk[f], got[f]), f
    assert nonzero_bytes(m, scratch) == 0


# ------------------------------------------------------------------------------------------------------------------ 3: check
def sk_sections(m):
    """(name, first byte, last byte) of the six sections of a wire private key: rho | K | tr | s1 | s2 | t0"""
    p = m.params
    eb = 3 if p.eta == 2 else 4
    bounds = [0, 32, 64, 128, 128 + p.l * 32 * eb, 128 + (p.l + p.k) * 32 * eb, m.SK_LEN]
    assert bounds[-1] - bounds[-2] == p.k * 416
    return [(nm, bounds[i], bounds[i + 1] - 1) for i, nm in enumerate(("rho", "K", "tr", "s1", "s2", "t0"))]


def damages(m):
    """thirteen ways to break a (seed, key) pair: one bit in the first and in the last byte of every section, or one bit of the seed"""
    out = []
    for nm, first, last in sk_sections(m):
        out += [("sk", first, 0x01), ("sk", last, 0x80)]
    return out + [("xi", 17, 0x10)]


def run_check(m, xi, sk, n, scratch, sb=None):
    match = torch.full((n + 2,), CANARY_U8, dtype=torch.uint8, device="cuda")
    xi_d, sk_d = dev(xi), dev(sk)  # (named: the call is asynchronous, its inputs must outlive this line)
    _seed_lib.check(_seed_lib.load().mldsa_seed_check(m.hp._h, m.pset, _ptr(xi_d), _ptr(sk_d), _ptr(match[1:]), n, _ptr(scratch),
                                                      scratch.numel() if sb is None else sb, _stream(m.device)))
    h = host(match)
    assert h[0] == CANARY_U8 and h[-1] == CANARY_U8
    assert nonzero_bytes(m, scratch) == 0, "the scratch is not all zero after mldsa_seed_check"
    return h[1:-1]


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("pset", SETS)
def test_seed_check_tells_damaged_pairs_from_intact_ones(sets, pset, n):
    m = sets[pset]
    par = parent(m, pset)
    dm = damages(m)
    assert len(dm) == 13 and len({d[1] for d in dm if d[0] == "sk"}) == 12
    xi0 = np.frombuffer(b"".join(par["xi"][:n]), dtype=np.uint8).reshape(n, 32)
    one_pass, least = scratch_bytes(m, n, "check"), scratch_bytes(m, min(n, 64), "check")
    # every pair intact
    assert run_check(m, xi0, par["sk"][:n], n, filled(one_pass)).tolist() == [1] * n
    if n == 1:
        # one key: each damage on its own
        for what, at, bit in dm:
            xi, sk = xi0.copy(), par["sk"][:1].copy()
            (xi if what == "xi" else sk)[0, at] ^= bit
            assert run_check(m, xi, sk, 1, filled(one_pass)).tolist() == [0], (what, at)
        return
    # damaged and intact pairs interleaved: the odd keys are damaged, every kind at least twice; a verdict that leaked into a
    # neighbour would turn an even key to 0 or an odd one to 1
    xi, sk = xi0.copy(), par["sk"][:n].copy()
    want = np.ones(n, dtype=np.uint8)
    for i in range(1, n, 2):
        what, at, bit = dm[(i // 2) % 13]
        (xi if what == "xi" else sk)[i, at] ^= bit
        want[i] = 0
    assert (n - 1) // 2 >= 26
    assert run_check(m, xi, sk, n, filled(one_pass)).tolist() == want.tolist()
    # the 64-key minimum (n = 65: two passes), identical verdicts; below it MLDSA_ERR_NOMEM before anything is launched
    assert run_check(m, xi, sk, n, filled(least), sb=least).tolist() == want.tolist()
    match = torch.full((n,), CANARY_U8, dtype=torch.uint8, device="cuda")
    small = filled(least)
    xi_d, sk_d = dev(xi), dev(sk)
    rc = _seed_lib.load().mldsa_seed_check(m.hp._h, pset, _ptr(xi_d), _ptr(sk_d), _ptr(match), n, _ptr(small), least - 1, _stream(m.device))
    assert rc == _lib.ERR_NOMEM and bool((match == CANARY_U8).all()) and bool((small == 0x5A).all())


# ------------------------------------------------------------------------------------------------------------------- 4: sign
def run_sign_seed(m, xi_dev, mode, mb, mo, cb, co, rnd, n_ops, kidx=None, scratch=None, sb=None, expect=_lib.OK, with_status=True):
    sigs = torch.full((n_ops + 2, m.SIG_LEN), CANARY_U8, dtype=torch.uint8, device="cuda")
    status = torch.full((n_ops + 2,), CANARY_I32, dtype=torch.int32, device="cuda")
    if scratch is None:
        scratch = filled(scratch_bytes(m, xi_dev.shape[0], "sign"))
    rc = _seed_lib.load().mldsa_sign_seed(
        m.hp._h, m.pset, mode, _ptr(xi_dev), xi_dev.shape[0], _ptr(kidx) if kidx is not None else NULL, _ptr(mb), _ptr(mo),
        _ptr(cb) if cb is not None else NULL, _ptr(co) if co is not None else NULL, _ptr(rnd), _ptr(sigs[1:]),
        _ptr(status[1:]) if with_status else NULL, n_ops, _ptr(scratch), scratch.numel() if sb is None else sb, _stream(m.device))
    assert rc == expect, (rc, _seed_lib.load().mldsa_seed_last_error())
    if rc == _lib.OK:
        assert nonzero_bytes(m, scratch) == 0, "the scratch is not all zero after mldsa_sign_seed"
    sg, st = host(sigs), host(status)
    assert (sg[0] == CANARY_U8).all() and (sg[-1] == CANARY_U8).all() and st[0] == CANARY_I32 and st[-1] == CANARY_I32
    return [r.tobytes() for r in sg[1:-1]], st[1:-1]


def core_sign(m, sks, mode, mb, mo, cb, co, rnd, n_ops, kidx=None):
    """the parent route's signatures and statuses: mldsa_sign on the sk_expanded mldsa_keygen keys"""
    sigs = torch.full((n_ops, m.SIG_LEN), CANARY_U8, dtype=torch.uint8, device="cuda")
    status = torch.full((n_ops,), CANARY_I32, dtype=torch.int32, device="cuda")
    m.sign_device(sks, mb, mo, rnd, sigs, n_ops, cb, co, kidx, mode, status)
    return [r.tobytes() for r in host(sigs)], host(status)


def first_keys(sks, n):
    return PrivateKeys(sks.pset, *(getattr(sks, f)[:n].contiguous().clone()
                                   for f in ("rho", "cap_k", "tr", "s_1_hat_mont", "s_2_hat_mont", "t_0_hat_mont")))


def sign_inputs(mode, n_ops):
    raw = [hashlib.shake_128(b"seed-msg" + int(i).to_bytes(4, "little")).digest(5 * i % 200) for i in range(n_ops)]
    msgs = [hash_message(x, PH_SHA512) for x in raw] if mode == MODE_PREHASH else raw
    ctxs = [hashlib.shake_128(b"seed-ctx" + int(i).to_bytes(4, "little")).digest((37 * i) % 256) for i in range(n_ops)]
    return msgs, ctxs


@pytest.mark.parametrize("mode", [MODE_PURE, MODE_INTERNAL, MODE_PREHASH])
@pytest.mark.parametrize("pset", SETS)
def test_sign_seed_equals_mldsa_sign_on_the_expanded_keygen_keys(sets, pset, mode):
    m = sets[pset]
    par = parent(m, pset)
    n_ops, n_keys = 65, 3
    xi = par["xi_dev"][:n_keys].contiguous()
    sks = first_keys(par["sks"], n_keys)
    kidx_h = (np.arange(n_ops) * 2 % n_keys).astype(np.uint32)  # 0 2 1 0 2 1 ...: every key many times
    kidx = kidx_dev(kidx_h)
    msgs, ctxs = sign_inputs(mode, n_ops)
    mb, mo = _cat_with_offsets(msgs, m.device)
    cb, co = _cat_with_offsets(ctxs, m.device)
    # the public keys of the seeds, from mldsa_seed_expand, for mldsa_verify_pk and the oracle
    _, pk = m.expand_seeds_device(xi, want_pk=True)
    opk = [orc.pk_try_from_bytes(pset, r.tobytes()) for r in host(pk)]
    for rnd_rows in ([bytes(32)] * n_ops, [shake(b"seed-rnd", i) for i in range(n_ops)]):
        rnd = u8(rnd_rows, 32)
        want, want_st = core_sign(m, sks, mode, mb, mo, cb, co, rnd, n_ops, kidx)
        got, st = run_sign_seed(m, xi, mode, mb, mo, cb, co, rnd, n_ops, kidx)
        assert not st.any() and not want_st.any()
        assert got == want, [i for i in range(n_ops) if got[i] != want[i]][:8]
        sg = dev(np.frombuffer(b"".join(got), dtype=np.uint8))
        ok = torch.zeros(n_ops, dtype=torch.uint8, device="cuda")
        m.verify_pk_device(pk, mb, mo, sg, ok, n_ops, cb, co, kidx, mode)
        assert host(ok).all()
        assert all(orc.verify_internal(pset, opk[kidx_h[i]], msgs[i], got[i], ctx=ctxs[i], mode=mode) for i in range(n_ops))
    # the table plus the smallest expansion pass is enough; one byte less is MLDSA_ERR_NOMEM with nothing written
    least = scratch_bytes(m, n_keys, "sign")  # n_keys < 64: one pass is the minimum
    got2, _ = run_sign_seed(m, xi, mode, mb, mo, cb, co, rnd, n_ops, kidx, scratch=filled(least), sb=least)
    assert got2 == got
    small = filled(least)
    none, st = run_sign_seed(m, xi, mode, mb, mo, cb, co, rnd, n_ops, kidx, scratch=small, sb=least - 1, expect=_lib.ERR_NOMEM)
    assert none == [bytes([CANARY_U8]) * m.SIG_LEN] * n_ops and (st == CANARY_I32).all() and bool((small == 0x5A).all())


@pytest.mark.parametrize("pset", SETS)
def test_sign_seed_with_a_seed_per_op_and_no_key_idx(sets, pset):
    m = sets[pset]
    par = parent(m, pset)
    n = 65
    xi = par["xi_dev"][:n].contiguous()
    sks = first_keys(par["sks"], n)
    msgs, ctxs = sign_inputs(MODE_PURE, n)
    mb, mo = _cat_with_offsets(msgs, m.device)
    cb, co = _cat_with_offsets(ctxs, m.device)
    rnd = u8([shake(b"seed-rnd65", i) for i in range(n)], 32)
    want, _ = core_sign(m, sks, MODE_PURE, mb, mo, cb, co, rnd, n)
    got, st = run_sign_seed(m, xi, MODE_PURE, mb, mo, cb, co, rnd, n)
    assert not st.any() and got == want
    # the table behind a 64-key expansion pass: two passes fill it, the same signatures; status may be NULL
    k, l = m.params.k, m.params.l
    least = n * (1024 * (l + 2 * k) + 128) + scratch_bytes(m, 64)
    assert least < scratch_bytes(m, n, "sign")
    got2, st2 = run_sign_seed(m, xi, MODE_PURE, mb, mo, cb, co, rnd, n, scratch=filled(least), sb=least, with_status=False)
    assert got2 == want and (st2 == CANARY_I32).all()
    run_sign_seed(m, xi, MODE_PURE, mb, mo, cb, co, rnd, n, scratch=filled(least), sb=least - 1, expect=_lib.ERR_NOMEM)
    # fewer seeds than ops without key_idx is an argument error, as in mldsa_sign
    run_sign_seed(m, xi[:64].contiguous(), MODE_PURE, mb, mo, cb, co, rnd, n, expect=_lib.ERR_PARAM)
    pk_all = dev(par["pk"][:n])
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    m.verify_pk_device(pk_all, mb, mo, dev(np.frombuffer(b"".join(got), dtype=np.uint8)), ok, n, cb, co, None, MODE_PURE)
    assert host(ok).all()


@pytest.mark.parametrize("pset", SETS)
def test_sign_seed_refusals_are_mldsa_signs_and_leave_the_neighbours_alone(sets, pset):
    m = sets[pset]
    par = parent(m, pset)
    n_ops, n_keys = 65, 3
    xi = par["xi_dev"][:n_keys].contiguous()
    sks = first_keys(par["sks"], n_keys)
    msgs, ctxs = sign_inputs(MODE_PURE, n_ops)
    ctxs[20] = bytes(256)                                     # MLDSA_ERR_CTX_LEN
    kidx_h = (np.arange(n_ops) % n_keys).astype(np.uint32)
    kidx_h[7], kidx_h[64] = n_keys, 0xFFFFFFFF                # MLDSA_ERR_PARAM
    mbuf, moff = table(msgs)
    moff = moff.copy()
    moff[41] = np.uint64(1) << np.uint64(63)                  # far past the end: the pairs of ops 40 and 41 are malformed, MLDSA_ERR_PARAM
    mb, mo = dev(mbuf), dev_off(moff)
    cb, co = _cat_with_offsets(ctxs, m.device)
    rnd = u8([shake(b"seed-rnd-ref", i) for i in range(n_ops)], 32)
    kidx = kidx_dev(kidx_h)
    want, want_st = core_sign(m, sks, MODE_PURE, mb, mo, cb, co, rnd, n_ops, kidx)
    scratch = filled(scratch_bytes(m, n_keys, "sign"))
    got, st = run_sign_seed(m, xi, MODE_PURE, mb, mo, cb, co, rnd, n_ops, kidx, scratch=scratch)  # (checks the zeroed scratch)
    assert got == want and st.tolist() == want_st.tolist()
    refused = {7: _lib.ERR_PARAM, 64: _lib.ERR_PARAM, 20: _lib.ERR_CTX_LEN, 40: _lib.ERR_PARAM, 41: _lib.ERR_PARAM}
    zero = bytes(m.SIG_LEN)
    # what the neighbours must be: the same batch without damage
    clean_mb, clean_mo = _cat_with_offsets(msgs, m.device)
    clean, _ = core_sign(m, sks, MODE_PURE, clean_mb, clean_mo, cb, co, rnd, n_ops, kidx_dev(np.arange(n_ops) % n_keys))
    for i in range(n_ops):
        if i in refused:
            assert st[i] == refused[i] and got[i] == zero, i
        else:
            assert st[i] == 0 and got[i] == clean[i] and got[i] != zero, i


def test_sign_seed_on_a_non_default_stream(sets):
    pset = 65
    m = sets[pset]
    par = parent(m, pset)
    n_ops, n_keys = 65, 3
    xi = par["xi_dev"][:n_keys].contiguous()
    sks = first_keys(par["sks"], n_keys)
    msgs, _ = sign_inputs(MODE_INTERNAL, n_ops)
    mb, mo = _cat_with_offsets(msgs, m.device)
    rnd = u8([shake(b"seed-rnd-stream", i) for i in range(n_ops)], 32)
    kidx = kidx_dev(np.arange(n_ops) % n_keys)
    want, _ = core_sign(m, sks, MODE_INTERNAL, mb, mo, None, None, rnd, n_ops, kidx)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert _stream(m.device).value == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        got, st = run_sign_seed(m, xi, MODE_INTERNAL, mb, mo, None, None, rnd, n_ops, kidx)
        # expansion and check are asynchronous on that stream too
        scratch = filled(scratch_bytes(m, n_keys))
        fields = raw_expand(m, xi, n_keys, scratch)
        assert nonzero_bytes(m, scratch) == 0
        assert run_check(m, host(xi), par["sk"][:n_keys], n_keys, filled(scratch_bytes(m, n_keys, "check"))).tolist() == [1] * n_keys
    assert got == want and not st.any()
    assert_same_key(fields, par, n_keys)


# ------------------------------------------------------------------------------------------------------------- 6: Python layer
@pytest.mark.parametrize("pset", SETS)
def test_python_layer_expand_check_and_sign_from_seeds(sets, pset):
    m = sets[pset]
    par = parent(m, pset)
    n_keys, n_ops = 5, 12
    seeds = par["xi"][:n_keys]
    msgs = [shake(b"seed-py-msg", i, 40 + i) for i in range(n_ops)]
    ctxs = [bytes([i]) * i for i in range(n_ops)]
    rnd = [shake(b"seed-py-rnd", i) for i in range(n_ops)]
    kidx = np.arange(n_ops, dtype=np.uint32) % n_keys
    # expand_seeds_device feeds the existing signing path; sign_from_seeds_device (behind try_sign_from_seeds) gives the same bytes
    sks, pk = m.expand_seeds_device(seeds, want_pk=True)
    assert isinstance(sks, PrivateKeys) and len(sks) == n_keys and np.array_equal(host(pk), par["pk"][:n_keys])
    via_fields = m.try_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, key_idx=kidx)
    via_seeds = m.try_sign_from_seeds(seeds, msgs, rnd, ctxs=ctxs, key_idx=kidx)
    via_parent = m.try_sign_with_seed(first_keys(par["sks"], n_keys), msgs, rnd, ctxs=ctxs, key_idx=kidx)
    assert torch.equal(via_fields, via_seeds) and torch.equal(via_seeds, via_parent)
    assert m.verify_pk(pk, msgs, via_seeds, ctxs=ctxs, key_idx=kidx).all()
    with pytest.raises(ValueError):
        m.try_sign_from_seeds(seeds, msgs, rnd, ctxs=[bytes(256)] * n_ops, key_idx=kidx)
    with pytest.raises(ValueError):
        m.expand_seeds_device([b"short"])
    # check_seeds_device agrees with the library-level check
    sk = par["sk"][:n_keys].copy()
    sk[1, 0] ^= 1
    sk[3, -1] ^= 0x80
    verdict = m.check_seeds_device(seeds, dev(sk))
    assert verdict.dtype == torch.bool and verdict.tolist() == [True, False, True, False, True]
    xi_h = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(n_keys, 32)
    assert run_check(m, xi_h, sk, n_keys, filled(scratch_bytes(m, n_keys, "check"))).tolist() == [1, 0, 1, 0, 1]
    # the three encodings of one key
    a = m.private_keys_from_forms(seed=seeds[0])
    b = m.private_keys_from_forms(expanded=par["sk"][0].tobytes())
    c = m.private_keys_from_forms(seed=seeds[0], expanded=par["sk"][0].tobytes())
    one = [m.try_sign_with_seed(k, msgs[:1], rnd[:1]) for k in (a, b, c)]
    assert torch.equal(one[0], one[1]) and torch.equal(one[1], one[2])
    with pytest.raises(ValueError):
        m.private_keys_from_forms(seed=seeds[1], expanded=par["sk"][0].tobytes())
