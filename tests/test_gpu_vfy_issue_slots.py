"""The large-batch verify pass (include/mldsa_vfy.h) after its k_verify_main was cut down in VALU issue slots: the row loop runs two rows a
trip on two register sets, every lane reads its hint bits from the masks in LDS, w1Encode gathers its dwords with one exchange, and
c_hat is stored negated.  None of that may change a verdict: 1 024 ops over 5 keys per parameter set, whose hints cover every (row,
coefficient) position of w1, clean and with every 7th signature damaged, against mldsa_verify op for op and the oracle for the first
16; and the small sizes that end the grid inside a block.  The layer is called directly, so the routing threshold does not apply."""
from fips204_amd import _vfy_lib
from fips204_amd.ml_dsa import MODE_PURE
from gpu_common import *
from sig_cases import KINDS, damage, every_seventh_damaged, get_z, hint_coverage
from vfy_calls import core_verify, fresh, gathered, signed_batch, verdicts, vfy_verify

pytestmark = pytest.mark.gpu

N_OPS, N_KEYS, ORACLE_OPS = 1024, 5, 16
SIZES = (1, 3, 64, 65, 257)

_batches = {}


def batch(m, n, nk):
    """n ops signed by the library under nk keys, built once per (parameter set, shape)"""
    key = (m.pset, n, nk)
    if key not in _batches:
        b = _batches[key] = signed_batch(m, b"slots", n, nk, lambda i: 1 + i % 97)
        b["per_op"] = gathered(b["pks"], b["kidx"])
    return _batches[key]


def both_mappings(lib, m, b, sig, n):
    """the verdicts of the layer under a key table and under one key per op, and the core's under the key table"""
    sg = dev(sig[:n])
    mo, kidx = b["mo"][:n + 1].contiguous(), kidx_dev(b["kidx"][:n])
    with_table = verdicts(vfy_verify(lib, m, b["pks"], b["mb"], mo, sg, fresh(n), n, kidx=kidx), n)
    per_op = verdicts(vfy_verify(lib, m, b["per_op"], b["mb"], mo, sg, fresh(n), n), n)
    core = verdicts(core_verify(m, b["pks"], b["mb"], mo, sg, fresh(n), n, kidx=kidx), n)
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
    bad, ops, kinds = every_seventh_damaged(p, sig)
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
    for t, (op, kind) in enumerate(zip(ops, kinds)):
        if kind.startswith("z_"):
            assert abs(get_z(p, bad[op], t % p.l, (37 * t) % 256)) == (bound if kind.endswith("bound") else bound - 1), (op, kind)


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
