"""The tests' own table of the twelve HashML-DSA pre-hash functions (FIPS 204 §5.4, the NIST hash OID arc
2.16.840.1.101.3.4.2.*) and the inputs the device tests feed them.  Pure numpy / hashlib: nothing here reads the product's
tables, so a wrong OID byte, digest length or code in the product cannot agree with it by construction."""
import hashlib
import os
import re

import numpy as np

OID_PREFIX = bytes([0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x02])
# name -> (MLDSA_PH_* code, last OID byte, digest bytes, hashlib name, block / rate in bytes)
ALL = {
    "SHA256": (0, 0x01, 32, "sha256", 64),
    "SHA512": (1, 0x03, 64, "sha512", 128),
    "SHAKE128": (2, 0x0B, 32, "shake_128", 168),
    "SHA384": (18, 0x02, 48, "sha384", 128),
    "SHA224": (20, 0x04, 28, "sha224", 64),
    "SHA512_224": (21, 0x05, 28, "sha512_224", 128),
    "SHA512_256": (22, 0x06, 32, "sha512_256", 128),
    "SHA3_224": (23, 0x07, 28, "sha3_224", 144),
    "SHA3_256": (24, 0x08, 32, "sha3_256", 136),
    "SHA3_384": (25, 0x09, 48, "sha3_384", 104),
    "SHA3_512": (26, 0x0A, 64, "sha3_512", 72),
    "SHAKE256": (28, 0x0C, 64, "shake_256", 136),
}
NEW = tuple(n for n in ALL if n not in ("SHA256", "SHA512", "SHAKE128"))
KECCAK = tuple(n for n in ALL if ALL[n][3].startswith(("sha3", "shake")))
# functions whose digests have the same length: only the OID byte separates their rows
SAME_LENGTH = (("SHA256", "SHA3_256", "SHA512_256", "SHAKE128"), ("SHA512", "SHA3_512", "SHAKE256"), ("SHA384", "SHA3_384"),
               ("SHA224", "SHA512_224", "SHA3_224"))
# every padding edge of every family: SHA-2 with 64-byte blocks, with 128-byte blocks, and the five Keccak rates
EDGES = (0, 1, 55, 56, 63, 64, 65, 119, 120, 111, 112, 127, 128, 239, 240) + tuple(
    x for r in (72, 104, 136, 144, 168) for x in (r - 1, r, r + 1, 2 * r - 1, 2 * r))


def row_len(name):
    return 11 + ALL[name][2]


def own_row(message, name):
    """OID || PH(M) from hashlib and this file's table"""
    _, last, dlen, hname, _ = ALL[name]
    h = hashlib.new(hname, message)
    return OID_PREFIX + bytes([last]) + (h.digest(dlen) if hname.startswith("shake") else h.digest())


def coop_max_ops():
    """MLDSA_PH_COOP_MAX_OPS as the public header states it (0: the library has no small-call form)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"^#define MLDSA_PH_COOP_MAX_OPS (\d+)\b", open(os.path.join(root, "include", "mldsa_ph.h")).read(), flags=re.M)
    assert m, "include/mldsa_ph.h does not define MLDSA_PH_COOP_MAX_OPS"
    return int(m.group(1))


def seam_messages():
    """the padding edges, 200 random lengths below 3000, two 4 MiB messages among short ones"""
    rng = np.random.default_rng(7)
    lens = list(EDGES) + list(rng.integers(0, 3000, 200)) + [4 << 20, 5, 4 << 20, 0]
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


def skewed_table(msgs, base, skew=5):
    """(flat bytes, offsets): the messages back to back behind base + skew bytes; the caller passes flat[base:], so that off[0] = skew
    is odd and with base = 1, 2, 3 no message is dword-aligned"""
    flat = np.frombuffer(bytes(base + skew) + b"".join(msgs) + bytes(8), dtype=np.uint8)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[0] = skew
    np.cumsum([len(x) for x in msgs], out=off[1:])
    off[1:] += np.uint64(skew)
    return flat, off


def cut_schedules(msgs, name):
    """label -> cuts[j] = [0 = c_0 <= ... <= c_U = len(msgs[j])]: 1, 3 and 16 pieces at random byte positions, and one cut at
    k block + d for the first two block boundaries of the function's block / rate"""
    B = ALL[name][4]
    out = {}
    for U in (1, 3, 16):
        rng = np.random.default_rng(2000 + U)
        out[f"random_{U}"] = [[0] + sorted(int(x) for x in rng.integers(0, len(m) + 1, U - 1)) + [len(m)] for m in msgs]
    for k in (1, 2):
        for d in (-1, 0, 1):
            p = k * B + d
            out[f"cut_{k}B{d:+d}"] = [[0, min(p, len(m)), len(m)] for m in msgs]
    return out
