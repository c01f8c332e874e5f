"""The key-deduplication library on the device (include/mldsa_keys.h): the seam mldsa_keys_dedup against a first-occurrence ranking
computed with numpy, forced hash collisions, a table smaller than the number of rows, and mldsa_verify_pk_dedup against
mldsa_verify_pk on the same device arrays (both routes) and against the oracle."""
from gpu_common import *  # noqa: F401,F403

from fips204_amd import _keys_lib
from fips204_amd.hotpath import _ptr, _stream
from fips204_amd.ml_dsa import MODE_INTERNAL, MODE_PREHASH, MODE_PURE, _cat_with_offsets, hash_message

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = -1515870811  # 0xA5A5A5A5 as int32
SEED = bytes(range(16))
NULL = C.c_void_p(0)


# ------------------------------------------------------------------------------------------------------------------ the seam
def keys_with_labels(m, n, d, rng_seed):
    """n keys of random bytes over exactly d distinct values: (pk [n, PK_LEN] on the device, label [n]).  Distinct by construction:
    bytes 4..8 of a value carry its number; values 1, 3, 5, 7, 9 are copies of 0, 2, 4, 6, 8 that differ from them in one byte only
    -- the first, the last, the last byte of lane 0's chunk and the first of lane 1's (bytes 15 and 16: the 16-byte boundary between
    neighbouring lanes), and the first byte of lane 0's second chunk (byte 1024: the boundary between two load steps)."""
    g = torch.Generator(device="cuda").manual_seed(rng_seed)
    base = torch.randint(0, 256, (d, m.PK_LEN), dtype=torch.uint8, device="cuda", generator=g)
    num = torch.arange(d, dtype=torch.int32, device="cuda").view(torch.uint8).view(d, 4)
    base[:, 4:8] = num
    for j, pos in enumerate((0, m.PK_LEN - 1, 15, 16, 1024)):
        if 2 * j + 1 < d:
            base[2 * j + 1] = base[2 * j]
            base[2 * j + 1, pos] ^= 0x40
    rng = np.random.default_rng(rng_seed)
    label = np.concatenate([np.arange(d), rng.integers(0, d, n - d)])
    label = label[rng.permutation(n)]
    pk = base[torch.from_numpy(label).cuda()].contiguous()
    return pk, label


def first_occurrence(label):
    """(row_of [n], index of the key that owns row r [n_rows]) of the ranking the header documents"""
    uniq, first = np.unique(label, return_index=True)
    owners = np.sort(first)
    row_label = np.empty(int(label.max()) + 1, dtype=np.int64)
    row_label[label[owners]] = np.arange(owners.size)
    return row_label[label], owners


def run_dedup(m, pk, seed=SEED, hash_bits=64, table_rows=None):
    """mldsa_keys_dedup on buffers of its own with canaries behind every output: (row_of, table incl. two canary rows, n_rows)"""
    lib = _keys_lib.load()
    n = pk.shape[0]
    rows = n if table_rows is None else table_rows
    row_of = torch.full((n + 64,), CANARY32, dtype=torch.int32, device="cuda")
    table = torch.full((rows + 2, m.PK_LEN), CANARY, dtype=torch.uint8, device="cuda")
    n_rows = torch.full((4,), CANARY32, dtype=torch.int32, device="cuda")
    sb = lib.mldsa_keys_dedup_scratch_bytes(m.pset, n)
    assert sb > 0
    scratch = torch.full((sb + 256,), CANARY, dtype=torch.uint8, device="cuda")
    _keys_lib.check(lib.mldsa_keys_dedup(m.hp._h, m.pset, _ptr(pk), n, seed, hash_bits, _ptr(row_of), _ptr(table) if rows else NULL, rows,
                                         _ptr(n_rows), _ptr(scratch), sb, _stream(m.device)))
    torch.cuda.synchronize()
    assert bool((row_of[n:] == CANARY32).all()) and bool((n_rows[1:] == CANARY32).all()), "written behind row_of / n_rows"
    assert bool((scratch[sb:] == CANARY).all()), "written behind the scratch"
    return row_of[:n], table, int(n_rows[0])


def check_invariants(m, pk, row_of, table, n_rows, table_rows):
    n = pk.shape[0]
    r = row_of.long()
    assert 0 < n_rows <= n and int(r.min()) >= 0 and int(r.max()) < n_rows
    held = min(n_rows, table_rows)
    assert bool((table[held:] == CANARY).all()), "a table row at or beyond min(n_rows, table_rows) was written"
    inside = r < held
    assert torch.equal(table[r[inside]], pk[inside]), "table[row_of[i]] != pk[i]"
    # every row below n_rows has a key
    assert int(torch.unique(r).numel()) == n_rows


# the 65 536-key cases are cases of their own (ids "...-65536"), so that each runs once and can be selected or left out by name
SEAM_SIZES = [pytest.param((1, 2, 63, 64, 65, 1000), id="small"), pytest.param((65536,), id="65536")]


@pytest.mark.parametrize("sizes", SEAM_SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_seam_equals_the_first_occurrence_ranking(sets, pset, sizes):
    m = sets[pset]
    for n in sizes:
        for d in sorted({1, min(2, n), max(1, n // 13), n}):
            pk, label = keys_with_labels(m, n, d, 1000 * pset + n + d)
            want_row_of, owners = first_occurrence(label)
            row_of, table, n_rows = run_dedup(m, pk)
            assert n_rows == d, (n, d, n_rows)
            assert np.array_equal(host(row_of), want_row_of), (n, d)
            assert torch.equal(table[:d], pk[torch.from_numpy(owners).cuda()]), (n, d)
            check_invariants(m, pk, row_of, table, n_rows, n)
            del pk, table
    if 1000 not in sizes:
        return
    # the Python call, with a seed from the system's generator
    pk, label = keys_with_labels(m, 1000, 77, pset)
    row_of, table, n_rows = m.dedup_public_keys_device(pk)
    want_row_of, owners = first_occurrence(label)
    assert int(host(n_rows)[0]) == 77 and np.array_equal(host(row_of), want_row_of)
    assert torch.equal(table[:77], pk[torch.from_numpy(owners).cuda()])


@pytest.mark.parametrize("pset,n", [(44, 1000), (65, 1000), (87, 1000), pytest.param(65, 65536, id="65-65536")])
def test_forced_collisions_keep_every_invariant(sets, pset, n):
    """hash_bits 1, 4, 12: many different keys under one hash value.  A key may then miss its equal and own a surplus row; nothing
    else gives.  One pass, no retry."""
    m = sets[pset]
    for d in sorted({2, max(1, n // 13), n}):
        pk, label = keys_with_labels(m, n, d, 7 * pset + n + d)
        for bits in (1, 4, 12):
            row_of, table, n_rows = run_dedup(m, pk, hash_bits=bits)
            assert d <= n_rows <= n, (bits, d, n_rows)
            check_invariants(m, pk, row_of, table, n_rows, n)
            # keys in one row are equal keys: the rows refine the true classes
            r = host(row_of)
            assert np.unique(np.stack([r, label]), axis=1).shape[1] == n_rows, (bits, d)
            # rows are numbered by first occurrence of their owners
            _, first = np.unique(r, return_index=True)
            assert np.all(np.diff(first) > 0), (bits, d)
        del pk, table


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_a_table_smaller_than_the_rows_is_filled_up_to_its_capacity(sets, pset):
    m = sets[pset]
    pk, label = keys_with_labels(m, 1000, 77, 31 + pset)
    want_row_of, owners = first_occurrence(label)
    for cap in (0, 1, 10, 76, 77, 200):
        row_of, table, n_rows = run_dedup(m, pk, table_rows=cap)
        assert n_rows == 77 and np.array_equal(host(row_of), want_row_of), cap
        held = min(cap, 77)
        assert torch.equal(table[:held], pk[torch.from_numpy(owners[:held]).cuda()]), cap
        assert bool((table[held:] == CANARY).all()), cap


# ------------------------------------------------------------------------------------------------------------------ the op-level call
def build_ops(m, n_ops, nk, mode, tag, damage_at=37):
    """n_ops signed operations over nk keys with the damage the parity tests want; device arrays + host copies for the oracle"""
    pk, sk = m.keygen_from_seed([shake(tag + b"key", i) for i in range(nk)])
    sks = m.private_keys_from_bytes(sk)
    raw = [shake(tag + b"msg", i, 1 + i % 50) for i in range(n_ops)]
    msgs = [hash_message(x, "SHA256") for x in raw] if mode == MODE_PREHASH else raw
    ctxs = [b"ctx-%d" % (i % 7) * (i % 3) for i in range(n_ops)]
    rnd = [shake(tag + b"rnd", i) for i in range(n_ops)]
    kidx = (np.arange(n_ops) % nk).astype(np.uint32)
    sig = m.try_sign_with_seed(sks, msgs, rnd, ctxs=ctxs, key_idx=kidx, mode=mode).clone()
    damaged = np.nonzero(np.arange(n_ops) % 100 == damage_at)[0]          # 1 % damaged signatures
    sig[torch.from_numpy(damaged).cuda(), 17] ^= 0x04
    kidx_v = kidx.copy()
    wrong = np.nonzero(np.arange(n_ops) % 50 == 11)[0]             # ops that point at the wrong key
    if nk > 1:
        kidx_v[wrong] = (kidx_v[wrong] + 1) % nk
    ctxs_v = list(ctxs)
    if n_ops > 5:
        ctxs_v[5] = b"x" * 300                                       # a ctx longer than 255 bytes
    mb, mo = _cat_with_offsets(msgs, m.device)
    cb, co = _cat_with_offsets(ctxs_v, m.device)
    if n_ops > 10:
        mo = mo.clone()
        mo[10] = mo[9] - 1                                           # a malformed message pair (ops 9 and 10 see it)
    return dict(pk=pk, kidx_v=kidx_v, msgs=msgs, ctxs=ctxs_v, sig=sig, mb=mb, mo=mo, cb=cb, co=co, n=n_ops, nk=nk, mode=mode,
                distinct=len(np.unique(kidx_v)))  # redirecting ops to the next key can leave a key without an op


def u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def call_dedup(m, b, pk, kidx, max_cached, scratch=None, hash_bits=64, stream=None, ok=None):
    """mldsa_verify_pk_dedup called directly: (ok, n_rows, route).  scratch: a tensor to use (else one of exactly the documented size,
    with a canary tail).  stream: a hipStream_t to enqueue on without waiting afterwards; `ok` ([n + 64], filled with 9 and complete
    before the call) must then be given, because a buffer made here would be filled on another stream."""
    lib = _keys_lib.load()
    n_keys = pk.shape[0]
    n_dedup = n_keys if kidx is not None else b["n"]
    need = lib.mldsa_keys_verify_scratch_bytes(m.pset, max(n_dedup, b["n"]), max_cached)
    assert need > 0
    own = scratch is None
    if own:
        scratch = torch.full((need + 256,), CANARY, dtype=torch.uint8, device="cuda")
    assert (stream is None) == (ok is None)
    if ok is None:
        ok = torch.full((b["n"] + 64,), 9, dtype=torch.uint8, device="cuda")
    info = _keys_lib.KeysInfo()
    _keys_lib.check(lib.mldsa_verify_pk_dedup(
        m.hp._h, m.pset, b["mode"], _ptr(pk), n_keys, _ptr(kidx) if kidx is not None else NULL, _ptr(b["mb"]), _ptr(b["mo"]), _ptr(b["cb"]),
        _ptr(b["co"]), _ptr(b["sig"]), _ptr(ok), b["n"], SEED, hash_bits, max_cached, _ptr(scratch), need, C.byref(info),
        stream if stream is not None else _stream(m.device)))
    if stream is None:
        torch.cuda.synchronize()
        assert bool((ok[b["n"]:] == 9).all())
        if own:
            assert bool((scratch[need:] == CANARY).all()), "written behind the scratch"
    return ok[:b["n"]], int(info.n_rows), int(info.route)


def call_plain(m, b, pk, kidx):
    ok = torch.full((b["n"],), 9, dtype=torch.uint8, device="cuda")
    m.verify_pk_device(pk, b["mb"], b["mo"], b["sig"], ok, b["n"], b["cb"], b["co"], kidx, b["mode"])
    torch.cuda.synchronize()
    return ok


def oracle_first(m, b, pk_rows, count=64):
    """verdicts of the first ops by the oracle: op i under the key bytes pk_rows[i]; None where the batch's offsets are damaged"""
    out = []
    pkh = host(pk_rows[:count])
    for i in range(min(count, b["n"])):
        if i in (9, 10) and b["n"] > 10:
            out.append(None)
        elif len(b["ctxs"][i]) > 255:
            out.append(False)
        else:
            pk_o = orc.pk_try_from_bytes(m.pset, pkh[i].tobytes())
            out.append(bool(orc.verify_internal(m.pset, pk_o, b["msgs"][i], host(b["sig"][i]).tobytes(), ctx=b["ctxs"][i], mode=b["mode"])))
    return out


def check_against_oracle(ok, want):
    got = host(ok)
    for i, w in enumerate(want):
        if w is not None:
            assert bool(got[i]) == w, i


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_verdicts_are_those_of_verify_pk_on_both_routes(sets, pset):
    m = sets[pset]
    n_ops, nk = 600, 40
    for mode in (MODE_PURE, MODE_INTERNAL, MODE_PREHASH):
        b = build_ops(m, n_ops, nk, mode, b"dedup%d-%d" % (pset, mode))
        # (a) every op carries its own wire key
        pk_ops = b["pk"][torch.from_numpy(b["kidx_v"].astype(np.int64)).cuda()].contiguous()
        base = call_plain(m, b, pk_ops, None)
        good = host(base).astype(bool)
        assert 0.9 * n_ops < good.sum() < n_ops and not good[5] and not good[9] and not good[37]
        check_against_oracle(base, oracle_first(m, b, pk_ops))
        dk = b["distinct"]
        for cap, route in ((dk, _keys_lib.ROUTE_CACHED), (n_ops, _keys_lib.ROUTE_CACHED), (dk - 1, _keys_lib.ROUTE_PLAIN), (0, _keys_lib.ROUTE_PLAIN)):
            ok, n_rows, got_route = call_dedup(m, b, pk_ops, None, cap)
            assert (n_rows, got_route) == (dk, route), (mode, cap, n_rows, got_route)
            assert torch.equal(ok, base), (mode, cap)
        # (b) a key table with repeated rows and key_idx, some entries out of range
        tab = torch.cat([b["pk"], b["pk"][:nk // 2]]).contiguous()
        kv = b["kidx_v"].copy()
        second = (np.arange(n_ops) % 3 == 1) & (kv < nk // 2)
        kv[second] += nk                                          # the same key through its second row
        kv[np.arange(n_ops) % 97 == 3] = tab.shape[0] + 5         # out of range: refused by the core's rule
        kv[np.arange(n_ops) % 97 == 4] = 0xFFFFFFFF
        kd = u32(kv)
        base_t = call_plain(m, b, tab, kd)
        in_range = kv < tab.shape[0]
        assert np.array_equal(host(base_t)[in_range], host(base)[in_range]) and not host(base_t)[~in_range].any()
        for cap, route in ((nk, _keys_lib.ROUTE_CACHED), (nk - 1, _keys_lib.ROUTE_PLAIN)):  # the whole table is deduplicated: nk distinct rows
            ok, n_rows, got_route = call_dedup(m, b, tab, kd, cap)
            assert (n_rows, got_route) == (nk, route), (mode, cap, n_rows, got_route)
            assert torch.equal(ok, base_t), (mode, cap)
        if pset == 65 and mode == MODE_PURE:
            # forced collisions: rows may be surplus, verdicts may not change
            ok, n_rows, got_route = call_dedup(m, b, pk_ops, None, n_ops, hash_bits=4)
            assert dk <= n_rows <= n_ops and got_route == _keys_lib.ROUTE_CACHED and torch.equal(ok, base)
            # the list-level Python call
            sigs = [host(b["sig"][i]).tobytes() for i in range(n_ops)]
            got = m.verify_pk(b["pk"], b["msgs"], sigs, ctxs=[c[:255] for c in b["ctxs"]], key_idx=b["kidx_v"], mode=mode, dedup=True)
            want = m.verify_pk(b["pk"], b["msgs"], sigs, ctxs=[c[:255] for c in b["ctxs"]], key_idx=b["kidx_v"], mode=mode)
            assert np.array_equal(got, want) and 0.9 * n_ops < want.sum() < n_ops
            info = {}
            okd = torch.zeros(n_ops, dtype=torch.uint8, device="cuda")
            m.verify_pk_dedup_device(pk_ops, b["mb"], b["mo"], b["sig"], okd, n_ops, b["cb"], b["co"], None, mode, info=info)
            torch.cuda.synchronize()
            assert info == {"n_rows": dk, "route": "cached"} and torch.equal(okd, base)
            scr = m.dedup_verify_scratch(n_ops)
            for _ in range(2):  # the caller's scratch, reused
                okd.zero_()
                m.verify_pk_dedup_device(pk_ops, b["mb"], b["mo"], b["sig"], okd, n_ops, b["cb"], b["co"], None, mode, scratch=scr)
                torch.cuda.synchronize()
                assert torch.equal(okd, base)


def test_65536_ops_over_1024_keys(sets):
    m = sets[65]
    n_ops, nk = 65536, 1024
    b = build_ops(m, n_ops, nk, MODE_PURE, b"dedup-large")
    pk_ops = b["pk"][torch.from_numpy(b["kidx_v"].astype(np.int64)).cuda()].contiguous()
    base = call_plain(m, b, pk_ops, None)
    good = host(base).astype(bool)
    assert 0.96 * n_ops < good.sum() < 0.98 * n_ops  # 1 % damaged, 2 % under the wrong key, three refused
    check_against_oracle(base, oracle_first(m, b, pk_ops))
    assert b["distinct"] == nk
    ok, n_rows, route = call_dedup(m, b, pk_ops, None, nk)
    assert (n_rows, route) == (nk, _keys_lib.ROUTE_CACHED)
    assert torch.equal(ok, base)
    ok, n_rows, route = call_dedup(m, b, pk_ops, None, nk - 1)
    assert (n_rows, route) == (nk, _keys_lib.ROUTE_PLAIN)
    assert torch.equal(ok, base)


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_small_calls(sets, pset):
    m = sets[pset]
    for n_ops in (1, 2, 8):
        b = build_ops(m, n_ops, min(n_ops, 3), MODE_PURE, b"dedup-small%d-%d" % (pset, n_ops))
        pk_ops = b["pk"][torch.from_numpy(b["kidx_v"].astype(np.int64)).cuda()].contiguous()
        base = call_plain(m, b, pk_ops, None)
        check_against_oracle(base, oracle_first(m, b, pk_ops))
        assert host(base)[0] == 1
        distinct = b["distinct"]
        for cap in (n_ops, 0):
            ok, n_rows, route = call_dedup(m, b, pk_ops, None, cap)
            assert n_rows == distinct and route == (_keys_lib.ROUTE_CACHED if cap else _keys_lib.ROUTE_PLAIN)
            assert torch.equal(ok, base), (n_ops, cap)


def test_two_streams_and_scratch_reused_back_to_back(sets):
    m = sets[65]
    lib = _keys_lib.load()
    ba = build_ops(m, 3000, 50, MODE_PURE, b"dedup-stream-a")
    bb = build_ops(m, 3000, 20, MODE_PURE, b"dedup-stream-b", damage_at=61)
    pa = ba["pk"][torch.from_numpy(ba["kidx_v"].astype(np.int64)).cuda()].contiguous()
    pb = bb["pk"][torch.from_numpy(bb["kidx_v"].astype(np.int64)).cuda()].contiguous()
    want_a, want_b = call_plain(m, ba, pa, None), call_plain(m, bb, pb, None)
    assert not torch.equal(want_a, want_b)
    need = lib.mldsa_keys_verify_scratch_bytes(65, 3000, 64)
    # two streams, a scratch each: the results of serial calls
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    scr_a = torch.full((need,), CANARY, dtype=torch.uint8, device="cuda")
    scr_b = torch.full((need,), CANARY, dtype=torch.uint8, device="cuda")
    oks = [torch.full((3000 + 64,), 9, dtype=torch.uint8, device="cuda") for _ in range(11)]
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        outs.append((call_dedup(m, ba, pa, None, 64, scratch=scr_a, stream=C.c_void_p(sa.cuda_stream), ok=oks[2 * rep]),
                     call_dedup(m, bb, pb, None, 64, scratch=scr_b, stream=C.c_void_p(sb.cuda_stream), ok=oks[2 * rep + 1])))
    torch.cuda.synchronize()
    for (oa, ra, rta), (ob, rb, rtb) in outs:
        assert (ra, rta, rb, rtb) == (ba["distinct"], _keys_lib.ROUTE_CACHED, bb["distinct"], _keys_lib.ROUTE_CACHED)
        assert torch.equal(oa, want_a) and torch.equal(ob, want_b)
    # one stream, one scratch, calls back to back with nothing between them (cached and plain routes mixed)
    s = C.c_void_p(sa.cuda_stream)
    seq = [(ba, pa, want_a, 64), (bb, pb, want_b, 64), (ba, pa, want_a, 10), (bb, pb, want_b, 64), (ba, pa, want_a, 64)]
    got = [call_dedup(m, b_, p_, None, cap, scratch=scr_a, stream=s, ok=oks[6 + j]) for j, (b_, p_, _, cap) in enumerate(seq)]
    torch.cuda.synchronize()
    for (ok, n_rows, route), (b_, _, want, cap) in zip(got, seq):
        assert n_rows == b_["distinct"] and route == (_keys_lib.ROUTE_CACHED if cap >= b_["distinct"] else _keys_lib.ROUTE_PLAIN)
        assert torch.equal(ok, want)
