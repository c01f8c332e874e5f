"""The nine pre-hash functions of the NIST hash OID arc beyond the reference's three (include/mldsa_ph.h: SHA-224/384,
SHA-512/224, SHA-512/256, SHA3-224/256/384/512, SHAKE256) without a device: codes, row lengths, sizes, refusals of every
other code, the SHA-2 initial values in the device source, and the host pre-hash.  Everything expected here comes from the
suite's own table (ph_fips_list_cases.py), hashlib and FIPS 180-4 arithmetic, not from the product's tables."""
import ctypes as C
import hashlib
import os
import re
from math import isqrt

import pytest

import ph_fips_list_cases as cases
from fips204_amd import _lib, _ph_lib
from layer_checks import ROOT, built, exported

PH_DIR = os.path.join(ROOT, "fips204_amd", "ph")

# name -> (code, last OID byte, digest bytes, hashlib name, the member of its family among the reference's three: their code)
NEW = {n: cases.ALL[n][:4] + ({64: 0, 128: 1}.get(cases.ALL[n][4], 2),) for n in cases.NEW}
UNKNOWN = tuple(range(3, 16)) + (16, 17, 19, 27, 29, 30, -1, 1 << 20)
# the exported symbols of the library before the nine functions were added: no entry point is new
PARENT_SYMBOLS = {
    "mldsa_ph_abi_version", "mldsa_ph_last_error", "mldsa_ph_row_len", "mldsa_ph_scratch_bytes", "mldsa_prehash",
    "mldsa_hash_verify", "mldsa_hash_verify_pk", "mldsa_hash_sign", "mldsa_ph_state_bytes", "mldsa_ph_init", "mldsa_ph_update",
    "mldsa_ph_final", "mldsa_ph_host_create", "mldsa_ph_host_destroy", "mldsa_hash_verify_host", "mldsa_hash_sign_host",
}


@pytest.fixture(scope="module")
def ph():
    return built(_ph_lib, PH_DIR)


def _macros():
    text = open(_ph_lib.HEADER_PATH).read()
    return {k: int(v) for k, v in re.findall(r"^#define (MLDSA_PH_[A-Z0-9_]+) (-?\d+)\b", text, flags=re.M)}


def test_codes_row_lengths_and_sizes(ph):
    mac = _macros()
    for name, (code, _, dlen, _, member) in NEW.items():
        assert mac["MLDSA_PH_" + name] == code == getattr(_ph_lib, "PH_" + name), name
        assert code == 16 + NEW[name][1]
        assert ph.mldsa_ph_row_len(code) == 11 + dlen, name
        prev_s = prev_t = 0
        for n in (1, 2, 63, 64, 65, 4096, 65536, 1 << 20):
            s, t = ph.mldsa_ph_scratch_bytes(code, n), ph.mldsa_ph_state_bytes(code, n)
            assert s >= n * (11 + dlen) + 8 * (n + 1) and s > prev_s, (name, n, s)
            assert t > prev_t and t == ph.mldsa_ph_state_bytes(member, n), (name, n, t)
            prev_s, prev_t = s, t
        assert ph.mldsa_ph_scratch_bytes(code, 2 ** 63) == 0 and ph.mldsa_ph_state_bytes(code, 2 ** 63) == 0
    assert (mac["MLDSA_PH_SHA256"], mac["MLDSA_PH_SHA512"], mac["MLDSA_PH_SHAKE128"]) == (0, 1, 2)
    assert mac["MLDSA_PH_ABI_VERSION"] == ph.mldsa_ph_abi_version() == 1
    assert mac["MLDSA_PH_COOP_MAX_OPS"] >= 0  # a documented macro of the header
    # the three + the nine, and no other MLDSA_PH_* code
    codes = {v for k, v in mac.items() if k not in ("MLDSA_PH_ABI_VERSION", "MLDSA_PH_COOP_MAX_OPS")}
    assert codes == {0, 1, 2} | {v[0] for v in NEW.values()}


def test_every_other_code_is_still_unknown_through_every_entry_point(ph):
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    null = None
    for code in UNKNOWN:
        assert ph.mldsa_ph_row_len(code) < 0, code
        assert ph.mldsa_ph_scratch_bytes(code, 10) == 0 and ph.mldsa_ph_state_bytes(code, 10) == 0, code
        calls = {
            "mldsa_prehash": lambda: ph.mldsa_prehash(null, code, p, p, p, null, 1, null),
            "mldsa_hash_verify": lambda: ph.mldsa_hash_verify(null, 44, code, p, p, p, 1, null, p, p, null, null, p, p, 1, p, 256, null),
            "mldsa_hash_verify_pk": lambda: ph.mldsa_hash_verify_pk(null, 44, code, p, 1, null, p, p, null, null, p, p, 1, p, 256, null),
            "mldsa_hash_sign": lambda: ph.mldsa_hash_sign(null, 44, code, *([p] * 6), 1, null, p, p, null, null, p, p, p, 1, p, 256, null),
            "mldsa_ph_init": lambda: ph.mldsa_ph_init(null, code, p, 256, 1, null),
            "mldsa_ph_update": lambda: ph.mldsa_ph_update(null, code, p, 256, p, p, 1, null),
            "mldsa_ph_final": lambda: ph.mldsa_ph_final(null, code, p, 256, p, null, null, 1, null),
            "mldsa_hash_verify_host": lambda: ph.mldsa_hash_verify_host(null, 44, code, p, 1, null, p, p, null, null, p, p, 1),
            "mldsa_hash_sign_host": lambda: ph.mldsa_hash_sign_host(null, 44, code, p, 1, null, p, p, null, null, p, p, null, 1),
        }
        for fn, call in calls.items():
            assert call() == _lib.ERR_PARAM, (fn, code)
            assert b"unknown ph" in ph.mldsa_ph_last_error(), (fn, code)
    # a new code gets past that check: the same calls fail on the NULL context instead
    assert ph.mldsa_hash_verify(null, 44, 24, p, p, p, 1, null, p, p, null, null, p, p, 1, p, 256, null) == _lib.ERR_PARAM
    assert b"unknown ph" not in ph.mldsa_ph_last_error()
    assert ph.mldsa_ph_init(null, 28, p, 256, 1, null) == _lib.ERR_PARAM and b"unknown ph" not in ph.mldsa_ph_last_error()
    assert ph.mldsa_prehash(null, 18, null, null, null, null, 0, null) == _lib.OK


def test_exported_symbols_are_the_parents(ph):
    assert {n for n in exported(_ph_lib.LIB_PATH) if n.startswith("mldsa_")} == PARENT_SYMBOLS == set(_ph_lib._SIGNATURES)


# ---- FIPS 180-4 in plain integers: SHA-512's compression function, then the initial values of §5.3.4-5.3.6
def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % q for q in out):
            out.append(k)
        k += 1
    return out


def _frac_root(p, root, bits):
    """the first `bits` bits of the fractional part of the root-th root of p"""
    n = p << (root * bits)
    x = isqrt(n) if root == 2 else int(round(n ** (1 / 3)))
    while x ** root > n:
        x -= 1
    while (x + 1) ** root <= n:
        x += 1
    return x & ((1 << bits) - 1)


_P80 = _primes(80)
_K512 = [_frac_root(p, 3, 64) for p in _P80]
_M64 = (1 << 64) - 1


def _rotr(x, r):
    return ((x >> r) | (x << (64 - r))) & _M64


def _sha512_raw(iv, message):
    padded = message + b"\x80" + bytes((-len(message) - 17) % 128) + (8 * len(message)).to_bytes(16, "big")
    h = list(iv)
    for base in range(0, len(padded), 128):
        w = [int.from_bytes(padded[base + 8 * i:base + 8 * i + 8], "big") for i in range(16)]
        for t in range(16, 80):
            s0 = _rotr(w[t - 15], 1) ^ _rotr(w[t - 15], 8) ^ (w[t - 15] >> 7)
            s1 = _rotr(w[t - 2], 19) ^ _rotr(w[t - 2], 61) ^ (w[t - 2] >> 6)
            w.append((w[t - 16] + s0 + w[t - 7] + s1) & _M64)
        a, b, c, d, e, f, g, hh = h
        for t in range(80):
            t1 = (hh + (_rotr(e, 14) ^ _rotr(e, 18) ^ _rotr(e, 41)) + ((e & f) ^ (~e & g & _M64)) + _K512[t] + w[t]) & _M64
            t2 = ((_rotr(a, 28) ^ _rotr(a, 34) ^ _rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c))) & _M64
            hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & _M64, c, b, a, (t1 + t2) & _M64
        h = [(x + y) & _M64 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]
    return h


def _parse_iv(text, name):
    m = re.search(r"constexpr uint(?:32|64)_t %s\[8\] = \{([^}]*)\};" % name, text)
    assert m, name
    return [int(x.rstrip("ul"), 16) for x in re.findall(r"0x[0-9a-fA-F]+u(?:ll)?", m.group(1))]


def test_sha2_initial_values_in_the_device_source_are_those_of_fips_180_4():
    iv512 = [_frac_root(p, 2, 64) for p in _P80[:8]]
    for msg in (b"", b"abc", bytes(range(256)) * 3):  # the compression function written here is SHA-512's
        assert b"".join(x.to_bytes(8, "big") for x in _sha512_raw(iv512, msg)) == hashlib.sha512(msg).digest()
    iv384 = [_frac_root(p, 2, 64) for p in _P80[8:16]]
    want = {
        "IV256_SHA256": [_frac_root(p, 2, 32) for p in _P80[:8]],
        "IV256_SHA224": [x & 0xFFFFFFFF for x in iv384],
        "IV512_SHA512": iv512,
        "IV512_SHA384": iv384,
        # §5.3.6: SHA-512 from H0 ^ a5a5...a5 over "SHA-512/t"
        "IV512_SHA512_224": _sha512_raw([x ^ 0xA5A5A5A5A5A5A5A5 for x in iv512], b"SHA-512/224"),
        "IV512_SHA512_256": _sha512_raw([x ^ 0xA5A5A5A5A5A5A5A5 for x in iv512], b"SHA-512/256"),
    }
    assert want["IV512_SHA384"][0] == 0xCBBB9D5DC1059ED8 and want["IV256_SHA224"][0] == 0xC1059ED8
    # the derived values reproduce hashlib when run through the same compression function
    for name, hname, dlen in (("IV512_SHA384", "sha384", 48), ("IV512_SHA512_224", "sha512_224", 28), ("IV512_SHA512_256", "sha512_256", 32)):
        got = b"".join(x.to_bytes(8, "big") for x in _sha512_raw(want[name], b"abc"))[:dlen]
        assert got == hashlib.new(hname, b"abc").digest(), name
    text = open(os.path.join(PH_DIR, "sha2_dev.h")).read()
    for name, values in want.items():
        parsed = _parse_iv(text, name)
        assert len(parsed) == 8 and parsed == values, name


def test_hash_message_of_the_nine_names_is_oid_and_hashlib():
    from fips204_amd.ml_dsa import hash_message
    msgs = [b"", b"a", bytes(range(256)), bytes(71), bytes(72), bytes(135), bytes(136), b"\xff" * 1000]
    for name in NEW:
        for m in msgs:
            row = hash_message(m, name)
            assert row == cases.own_row(m, name) and len(row) == 11 + NEW[name][2], (name, len(m))
    for bad in ("SHA1", "sha384", "SHA3-256", "", None, 18):
        with pytest.raises(ValueError):
            hash_message(b"x", bad)
