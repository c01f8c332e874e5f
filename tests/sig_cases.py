"""The encoded signature on the CPU: sigEncode's sections c~ | z | hints (encodings.rs:238-276), one z coefficient read and written in
place, HintBitUnpack, and the ways the verify tests damage a well-formed signature.  numpy and the stdlib only; `p` is the parameters
as orc.params(pset) / m.params give them (k, l, gamma1, beta, omega, ctilde_len, sig_len).  test_sig_cases_cpu.py checks this module
against the oracle's decoder."""
import numpy as np

# what damage() knows to do; the *_bit kinds flip one bit of a section (z{j}_bit, one per z polynomial, beside those listed)
KINDS = ("ctilde_bit", "z_plus_bound", "z_minus_bound", "z_plus_inside", "z_minus_inside", "hint_out_of_order", "hint_count_above_omega",
         "hint_padding_not_zero")
ALIASES = {"hint_positions_not_increasing": "hint_out_of_order", "hint_limit_above_omega": "hint_count_above_omega"}


def sections(p):
    """(bits per z coefficient, first byte of z, first byte of the hint section)"""
    cb = 18 if p.gamma1 == (1 << 17) else 20
    return cb, p.ctilde_len, p.ctilde_len + p.l * 32 * cb


def spans(p):
    """the byte ranges (first, end) of c~, z and the hint section"""
    _, z0, h0 = sections(p)
    return (0, z0), (z0, h0), (h0, p.sig_len)


def z_field(p, poly, idx):
    """(first of the 4 bytes that hold coefficient idx of z polynomial `poly`, its shift in them, its mask)"""
    cb, z0, _ = sections(p)
    assert 0 <= poly < p.l and 0 <= idx < 256
    bit = 8 * z0 + (poly * 256 + idx) * cb
    return bit // 8, bit % 8, (1 << cb) - 1


def get_z(p, sig, poly, idx):
    """coefficient idx of z polynomial `poly` (BitUnpack(gamma1 - 1, gamma1): the field holds gamma1 - z)"""
    at, sh, mask = z_field(p, poly, idx)
    return p.gamma1 - ((int.from_bytes(bytes(sig[at:at + 4]), "little") >> sh) & mask)


def set_z(p, sig, poly, idx, z):
    """coefficient idx of z polynomial `poly` := z, in place"""
    at, sh, mask = z_field(p, poly, idx)
    field = p.gamma1 - z
    assert 0 <= field <= mask
    v = (int.from_bytes(bytes(sig[at:at + 4]), "little") & ~(mask << sh)) | (field << sh)
    sig[at:at + 4] = np.frombuffer(v.to_bytes(4, "little"), dtype=np.uint8)


def hint_limits(p, sig):
    """the k running hint counts that end the hint section, as ints: the last is the signature's hint weight"""
    h0 = sections(p)[2]
    return sig[h0 + p.omega:h0 + p.omega + p.k].astype(int)


def hint_positions(p, sig):
    """HintBitUnpack of one signature (numpy uint8): the list of (row, coefficient) with a hint, or None where the section is malformed"""
    h0 = sections(p)[2]
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


def flip(sig, byte, bit):
    """a copy of `sig` with one bit flipped"""
    s = sig.copy()
    s[byte] ^= 1 << bit
    return s


def damage(p, good, kind, salt=0, site=None):
    """A copy of the well-formed signature `good` damaged in one way; `salt` moves the site about.  A *_bit kind flips the bit
    `site` = (byte, bit) of its section where one is given, and ctilde_bit without one byte salt mod the section's length, bit salt mod 8."""
    kind = ALIASES.get(kind, kind)
    _, z0, h0 = sections(p)
    lim = hint_limits(p, good)
    starts = np.concatenate([[0], lim[:-1]])
    total = int(lim[-1])
    bound = p.gamma1 - p.beta
    s = good.copy()
    if kind.endswith("_bit"):
        name = kind[:-4]
        zlen = (h0 - z0) // p.l
        lo, hi = {"ctilde": (0, z0), "hint": (h0, p.sig_len), **{f"z{j}": (z0 + j * zlen, z0 + (j + 1) * zlen) for j in range(p.l)}}[name]
        assert site is not None or name == "ctilde"
        byte, bit = (salt % z0, salt % 8) if site is None else site
        assert lo <= byte < hi and 0 <= bit < 8
        s = flip(good, byte, bit)
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


def every_seventh_damaged(p, sig):
    """every 7th signature of the batch damaged, the kinds in turn: (signatures, damaged ops, their kinds)"""
    out = sig.copy()
    ops, used = [], []
    for t, op in enumerate(range(0, sig.shape[0], 7)):
        kind = KINDS[t % len(KINDS)]
        if kind == "hint_padding_not_zero" and int(hint_limits(p, sig[op])[-1]) == p.omega:
            kind = "hint_count_above_omega"
        out[op] = damage(p, sig[op], kind, t)
        ops.append(op)
        used.append(kind)
    return out, ops, used
