"""tests/sig_cases.py against the oracle: the section layout, HintBitUnpack, one z coefficient read and written in place, and every way
of damaging a signature, on 8 oracle-made signatures per parameter set.  The GPU verify tests build their inputs with that module, so a
wrong bit offset there would otherwise show only as a puzzling verdict."""
import numpy as np
import pytest

import sig_cases as sc
from oracle import oracle as orc

PSETS = (44, 65, 87)
MALFORMED_HINTS = ("hint_out_of_order", "hint_count_above_omega", "hint_padding_not_zero")
_made = {}


def signed(pset):
    """(parameters, public key, messages, signatures as uint8 arrays), made once per set: messages of 0, 1 and 70 bytes in turn"""
    if pset not in _made:
        pk, sk = orc.keygen_from_seed(pset, bytes([pset]) * 32)
        msgs = [bytes([i]) * (0, 1, 70)[i % 3] for i in range(8)]
        sigs = [np.frombuffer(orc.sign_internal(pset, sk, m, bytes([i]) * 32), dtype=np.uint8).copy() for i, m in enumerate(msgs)]
        assert all(orc.verify_internal(pset, pk, m, bytes(s)) for m, s in zip(msgs, sigs))
        _made[pset] = (orc.params(pset), pk, msgs, sigs)
    return _made[pset]


@pytest.mark.parametrize("pset", PSETS)
def test_sections_and_hint_positions_are_the_decoders(pset):
    p, _, _, sigs = signed(pset)
    cb, z0, h0 = sc.sections(p)
    assert (cb, z0) == (18 if pset == 44 else 20, p.ctilde_len) and h0 + p.omega + p.k == p.sig_len
    assert sc.spans(p) == ((0, z0), (z0, h0), (h0, p.sig_len))
    total = 0
    for s in sigs:
        ok, _, _, h = orc.sig_decode(pset, bytes(s))
        assert ok and sc.hint_positions(p, s) == [(int(i), int(c)) for i, c in np.argwhere(h)]  # (row-major: rows, then positions, ascending)
        assert int(sc.hint_limits(p, s)[-1]) == int(h.sum())
        total += int(h.sum())
    cover = sc.hint_coverage(p, sigs)
    assert cover.shape == (p.k, 256) and int(cover.sum()) == total


@pytest.mark.parametrize("pset", PSETS)
def test_get_z_is_the_decoders_at_every_coefficient(pset):
    p, _, _, sigs = signed(pset)
    z = orc.sig_decode(pset, bytes(sigs[0]))[2]
    assert [[sc.get_z(p, sigs[0], j, i) for i in range(256)] for j in range(p.l)] == z.tolist()


@pytest.mark.parametrize("pset", PSETS)
def test_set_z_changes_one_coefficient_and_its_four_bytes_only(pset):
    """the sites put fields on both sides of a byte boundary, at 18 and at 20 bits per field"""
    p, _, _, sigs = signed(pset)
    good = sigs[1]
    _, ct, z, h = orc.sig_decode(pset, bytes(good))
    bound = p.gamma1 - p.beta
    shifts = set()
    for poly, idx in ((0, 0), (0, 255), (p.l - 1, 3), (p.l - 1, 255)):
        at, sh, _ = sc.z_field(p, poly, idx)
        shifts.add(sh)
        for v in (bound, -bound, bound - 1, 0, p.gamma1, -(p.gamma1 - 1)):
            s = good.copy()
            sc.set_z(p, s, poly, idx, v)
            assert sc.get_z(p, s, poly, idx) == v
            ok, ct2, z2, h2 = orc.sig_decode(pset, bytes(s))
            want = z.copy()
            want[poly, idx] = v
            assert ok and ct2 == ct and np.array_equal(z2, want) and np.array_equal(h2, h), (poly, idx, v)
            assert np.array_equal(s[:at], good[:at]) and np.array_equal(s[at + 4:], good[at + 4:])
    assert len(shifts) >= 2 and 0 in shifts
    with pytest.raises(AssertionError):
        sc.set_z(p, good.copy(), 0, 0, p.gamma1 + 1)  # (the field would be negative)


def _kinds_and_sites(p):
    """every kind damage() takes, with a site where the kind needs one"""
    cb, z0, h0 = sc.sections(p)
    out = [(k, None) for k in sc.KINDS + tuple(sc.ALIASES)] + [("ctilde_bit", (z0 // 2, 3)), ("hint_bit", (h0, 0))]
    return out + [(f"z{j}_bit", (z0 + j * 32 * cb + 11 * (j + 1), j % 8)) for j in range(p.l)]


@pytest.mark.parametrize("pset", PSETS)
def test_every_damage_kind_differs_and_is_refused(pset):
    p, pk, msgs, sigs = signed(pset)
    op = next(i for i, s in enumerate(sigs) if 2 <= int(sc.hint_limits(p, s)[-1]) < p.omega)
    good, msg = sigs[op], msgs[op]
    kinds = _kinds_and_sites(p)
    assert len(kinds) == len(sc.KINDS) + 2 + 2 + p.l
    for kind, site in kinds:
        for salt in (0, 1, 17, 40):
            s = sc.damage(p, good, kind, salt, site)
            assert s is not good and s.shape == good.shape and not np.array_equal(s, good), (kind, salt)
            assert not orc.verify_internal(pset, pk, msg, bytes(s)), (kind, salt)
            if sc.ALIASES.get(kind, kind) in MALFORMED_HINTS:
                assert sc.hint_positions(p, s) is None and not orc.sig_decode(pset, bytes(s))[0], (kind, salt)
            elif not kind.startswith("hint"):
                assert sc.hint_positions(p, s) == sc.hint_positions(p, good)
    assert orc.verify_internal(pset, pk, msg, bytes(good))  # the good signature was left alone
    assert set(MALFORMED_HINTS) < set(sc.KINDS)
    with pytest.raises(AssertionError):
        sc.damage(p, good, "z0_bit", 0, (0, 0))  # a site outside the kind's section
    bad, ops, used = sc.every_seventh_damaged(p, np.stack(sigs))
    assert ops == [0, 7] and used == list(sc.KINDS[:2]) and [i for i in range(8) if not np.array_equal(bad[i], sigs[i])] == ops


@pytest.mark.parametrize("pset", PSETS)
def test_a_signature_with_omega_hints_has_no_padding_to_dirty(pset):
    p, _, _, sigs = signed(pset)
    h0 = sc.sections(p)[2]
    full = sigs[0].copy()
    full[h0:h0 + p.omega] = np.arange(p.omega)  # omega hints in row 0, none in the other rows
    full[h0 + p.omega:] = p.omega
    assert sc.hint_positions(p, full) == [(0, c) for c in range(p.omega)] and orc.sig_decode(pset, bytes(full))[0]
    with pytest.raises(AssertionError):
        sc.damage(p, full, "hint_padding_not_zero", 0)
    used = sc.every_seventh_damaged(p, np.stack([full] * 50))[2]  # the batch takes the kind before it in that signature's place
    assert used == list(sc.KINDS[:7]) + ["hint_count_above_omega"]
