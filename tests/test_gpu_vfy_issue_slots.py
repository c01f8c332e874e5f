"""The large-batch verify pass (include/mldsa_vfy.h) after its k_verify_main was cut down in VALU issue slots: the row loop runs two rows a
trip on two register sets, every lane reads its hint bits from the masks in LDS, w1Encode gathers its dwords with one exchange, and
c_hat is stored negated.  None of that may change a verdict: 1 024 ops over 5 keys per parameter set, whose hints cover every (row,
coefficient) position of w1, clean and with every 7th signature damaged, against mldsa_verify op for op and the oracle for the first
16; and the small sizes that end the grid inside a block.  The layer is called directly, so the routing threshold does not apply."""
from fips204_amd import _lib, _vfy_lib
from fips204_amd.hotpath import _optr, _ptr, _stream
from fips204_amd.ml_dsa import MODE_PURE, PublicKeys, _cat_with_offsets
from gpu_common import *

pytestmark = pytest.mark.gpu

N_OPS, N_KEYS, ORACLE_OPS = 1024, 5, 16
SIZES = (1, 3, 64, 65, 257)
KINDS = ("ctilde_bit", "z_plus_bound", "z_minus_bound", "z_plus_inside", "z_minus_inside", "hint_out_of_order", "hint_count_above_omega",
         "hint_padding_not_zero")


# ------------------------------------------------------------------------------------------------- the signature's sections, on the CPU
def sections(p):
    """(bits per z coefficient, first byte of z, first byte of the hint section) of sigEncode: c~ | z | hints"""
    cb = 18 if p.gamma1 == (1 << 17) else 20
    return cb, p.ctilde_len, p.ctilde_len + p.l * 32 * cb


def hint_positions(p, sig):
    """HintBitUnpack of one signature (numpy uint8): the list of (row, coefficient) with a hint, or None where the section is malformed"""
    _, _, h0 = sections(p)
    y = sig[h0:h0 + p.omega + p.k].astype(int)
    out, first = [], 0
    for i in range(p.k):
        lim = y[p.omega + i]
        if lim < first or lim > p.omega:
            return None
        for j in range(first, lim):
            if j > first and y[j - 1] >= y[j]:
                return None
            out.append((i, int(y[j])))
        first = lim
    if y[first:p.omega].any():
        return None
    return out


def hint_coverage(p, sigs):
    """hints per (row, coefficient) position over the well-formed signatures of `sigs`"""
    cover = np.zeros((p.k, 256), dtype=np.int64)
    for s in sigs:
        pos = hint_positions(p, s)
        assert pos is not None
        for i, c in pos:
            cover[i, c] += 1
    return cover


def set_z(p, sig, poly, idx, z):
    """coefficient idx of z polynomial `poly` := z (BitPack(z, gamma1 - 1, gamma1): the field holds gamma1 - z)"""
    cb, z0, _ = sections(p)
    field = p.gamma1 - z
    assert 0 <= field < (1 << cb)
    bit = 8 * z0 + (poly * 256 + idx) * cb
    v = int.from_bytes(bytes(sig[bit // 8:bit // 8 + 4]), "little")
    sh = bit % 8
    v = (v & ~(((1 << cb) - 1) << sh)) | (field << sh)
    sig[bit // 8:bit // 8 + 4] = np.frombuffer(v.to_bytes(4, "little"), dtype=np.uint8)


def damage(p, good, kind, salt):
    """a copy of the well-formed signature `good` damaged in one way; `salt` moves the site about"""
    _, z0, h0 = sections(p)
    s = good.copy()
    lim = good[h0 + p.omega:h0 + p.omega + p.k].astype(int)
    starts = np.concatenate([[0], lim[:-1]])
    total = int(lim[-1])
    bound = p.gamma1 - p.beta
    if kind == "ctilde_bit":
        s[salt % z0] ^= 1 << (salt % 8)
    elif kind.startswith("z_"):
        z = {"z_plus_bound": bound, "z_minus_bound": -bound, "z_plus_inside": bound - 1, "z_minus_inside": -(bound - 1)}[kind]
        set_z(p, s, salt % p.l, (37 * salt) % 256, z)
    elif kind == "hint_out_of_order":
        i = int(np.argmax(lim - starts))
        assert lim[i] - starts[i] >= 2  # a polynomial with two hints to swap
        a = h0 + int(starts[i]) + salt % int(lim[i] - starts[i] - 1)
        s[a], s[a + 1] = good[a + 1], good[a]
    elif kind == "hint_count_above_omega":
        s[h0 + p.omega + p.k - 1] = p.omega + 1
    else:
        assert kind == "hint_padding_not_zero" and total < p.omega  # (a signature with omega hints has no padding)
        s[h0 + total + salt % (p.omega - total)] = 1 + salt % 255
    assert not np.array_equal(s, good)
    return s


def damaged_batch(p, sig):
    """every 7th signature of the batch damaged, the kinds in turn: (signatures, damaged ops, their kinds)"""
    out = sig.copy()
    ops, kinds = [], []
    for t, op in enumerate(range(0, sig.shape[0], 7)):
        kind = KINDS[t % len(KINDS)]
        _, _, h0 = sections(p)
        if kind == "hint_padding_not_zero" and int(sig[op][h0 + p.omega + p.k - 1]) == p.omega:
            kind = "hint_count_above_omega"
        out[op] = damage(p, sig[op], kind, t)
        ops.append(op)
        kinds.append(kind)
    return out, ops, kinds


# --------------------------------------------------------------------------------------------------------------- the calls
def vfy_verify(lib, m, pks, mb, mo, sigs, n, kidx=None):
    ok = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    scratch = filled(lib.mldsa_vfy_scratch_bytes(m.pset, n))
    _vfy_lib.check(lib.mldsa_vfy_verify(m.hp._h, m.pset, MODE_PURE, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(kidx),
                                        _ptr(mb), _ptr(mo), None, None, _ptr(sigs), _ptr(ok), n, _ptr(scratch), scratch.numel(), _stream(m.device)))
    got = host(ok)
    assert set(got.tolist()) <= {0, 1}
    return got.astype(bool)


def core_verify(m, pks, mb, mo, sigs, n, kidx=None):
    ok = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    _lib.check(m.lib.mldsa_verify(m.hp._h, m.pset, MODE_PURE, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(kidx), _ptr(mb),
                                  _ptr(mo), None, None, _ptr(sigs), _ptr(ok), n, _stream(m.device)))
    got = host(ok)
    assert set(got.tolist()) <= {0, 1}
    return got.astype(bool)


def gathered(pks, kidx):
    g = torch.from_numpy(kidx.astype(np.int64)).cuda()
    return PublicKeys(pks.pset, pks.rho[g].contiguous(), pks.tr[g].contiguous(), pks.t1_d2_hat_mont[g].contiguous())


_batches = {}


def batch(m, n, nk):
    """n ops signed by the library under nk keys, built once per (parameter set, shape)"""
    key = (m.pset, n, nk)
    if key not in _batches:
        xi = [shake(b"slots-key%d" % m.pset, i) for i in range(nk)]
        pk, sk = m.keygen_from_seed(xi)
        pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
        msgs = [shake(b"slots-msg%d" % m.pset, i, 1 + i % 97) for i in range(n)]
        rnd = [shake(b"slots-rnd", i) for i in range(n)]
        kidx = (np.arange(n) * 3 % nk).astype(np.uint32)
        sig = m.try_sign_with_seed(sks, msgs, rnd, key_idx=kidx, mode=MODE_PURE)
        mb, mo = _cat_with_offsets(msgs, m.device)
        okeys = [orc.pk_try_from_bytes(m.pset, host(pk)[i].tobytes()) for i in range(nk)]
        _batches[key] = dict(pks=pks, per_op=gathered(pks, kidx), msgs=msgs, kidx=kidx, sig=host(sig).copy(), mb=mb, mo=mo, okeys=okeys)
    return _batches[key]


def both_mappings(lib, m, b, sig, n):
    """the verdicts of the layer under a key table and under one key per op, and the core's under the key table"""
    sg = dev(sig[:n])
    mo = b["mo"][:n + 1].contiguous()
    with_table = vfy_verify(lib, m, b["pks"], b["mb"], mo, sg, n, kidx_dev(b["kidx"][:n]))
    per_op = vfy_verify(lib, m, b["per_op"], b["mb"], mo, sg, n)
    core = core_verify(m, b["pks"], b["mb"], mo, sg, n, kidx_dev(b["kidx"][:n]))
    return with_table, per_op, core


# --------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verdicts_over_a_batch_whose_hints_cover_every_position(sets, pset):
    m = sets[pset]
    p = m.params
    lib = _vfy_lib.load()
    assert lib.mldsa_vfy_set_part_ops(0) == _vfy_lib.part_ops()  # the part size the library ships with
    b = batch(m, N_OPS, N_KEYS)
    sig = b["sig"]
    # the condition that pins the hint-bit lookup: every lane and mask word of every row decides a hint in some valid signature
    cover = hint_coverage(p, sig)
    assert cover.shape == (p.k, 256) and int(cover.min()) >= 1, np.argwhere(cover == 0)[:8]
    with_table, per_op, core = both_mappings(lib, m, b, sig, N_OPS)
    assert core.all()
    assert with_table.tolist() == core.tolist() and per_op.tolist() == core.tolist()
    for i in range(ORACLE_OPS):
        assert orc.verify_internal(pset, b["okeys"][int(b["kidx"][i])], b["msgs"][i], bytes(sig[i]), mode=MODE_PURE), i
    # ---- every 7th signature damaged, the kinds in turn
    bad, ops, kinds = damaged_batch(p, sig)
    assert set(kinds) == set(KINDS) and len(ops) == (N_OPS + 6) // 7
    with_table, per_op, core = both_mappings(lib, m, b, bad, N_OPS)
    want = np.ones(N_OPS, dtype=bool)
    want[ops] = False
    assert core.tolist() == want.tolist(), [k for o, k in zip(ops, kinds) if core[o]]
    assert with_table.tolist() == core.tolist(), [(o, k) for o, k in zip(ops, kinds) if with_table[o] != core[o]]
    assert per_op.tolist() == core.tolist(), [(o, k) for o, k in zip(ops, kinds) if per_op[o] != core[o]]
    for i in range(ORACLE_OPS):
        assert orc.verify_internal(pset, b["okeys"][int(b["kidx"][i])], b["msgs"][i], bytes(bad[i]), mode=MODE_PURE) == bool(want[i]), i
    # the z sites: exactly the bound is refused by the norm check, one inside it only by the hash -- both are in the batch
    bound = p.gamma1 - p.beta
    cb, z0, _ = sections(p)
    for t, (op, kind) in enumerate(zip(ops, kinds)):
        if kind.startswith("z_"):
            bit = 8 * z0 + ((t % p.l) * 256 + (37 * t) % 256) * cb
            field = (int.from_bytes(bytes(bad[op][bit // 8:bit // 8 + 4]), "little") >> (bit % 8)) & ((1 << cb) - 1)
            assert abs(p.gamma1 - field) == (bound if kind.endswith("bound") else bound - 1), (op, kind)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_small_sizes_under_a_single_key(sets, pset, n):
    """1 and 3 ops leave waves of the only block idle, 65 and 257 end the grid one op into a block; the last op is then damaged in c~"""
    m = sets[pset]
    lib = _vfy_lib.load()
    assert lib.mldsa_vfy_set_part_ops(0) == _vfy_lib.part_ops()
    b = batch(m, max(SIZES), 1)
    assert len(b["pks"]) == 1 and not b["kidx"].any()
    with_table, per_op, core = both_mappings(lib, m, b, b["sig"], n)
    assert core.all() and with_table.tolist() == core.tolist() and per_op.tolist() == core.tolist()
    bad = b["sig"][:n].copy()
    bad[n - 1] = damage(m.params, bad[n - 1], "ctilde_bit", n)
    with_table, per_op, core = both_mappings(lib, m, b, bad, n)
    assert core.tolist() == [True] * (n - 1) + [False]
    assert with_table.tolist() == core.tolist() and per_op.tolist() == core.tolist()
