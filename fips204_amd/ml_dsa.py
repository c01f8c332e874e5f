"""Batched mirror of the reference's public API for the accelerated path.

`ml_dsa_44`, `ml_dsa_65`, `ml_dsa_87` mirror the modules the `functionality!()` macro stamps
out (src/lib.rs:116-614): KeyGen / Signer / Verifier / SerDes (src/traits.rs), with every
method taking a *batch* of independent operations.  Keys live on the device in the
reference's expanded form (src/types.rs:19-41), field by field.  All compute goes through
the C ABI (include/mldsa_hip.h); there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _crl_lib, _csr_lib, _find_lib, _keycheck_lib, _keys_lib, _lib, _mu_lib, _mus_lib, _path_lib, _ph_lib, _rec_lib, _recsign_lib, _seed_lib, _vfy_lib, _x509_lib, _x509sign_lib
from .hotpath import HotPath, N, _optr, _ptr, _stream

MODE_PURE, MODE_INTERNAL, MODE_PREHASH = 0, 1, 2

# verify_device calls of at least this many ops (per parameter set) that derive A_hat per op run on libmldsa_vfy.so
# (include/mldsa_vfy.h).  Measured on the library as it ships, core and layer alternated four times per set and size over 8 192 ...
# 65 536 ops (profiles/vfy_layer_ab.jsonl kind min_ops): the smallest size from which, at it and at every larger
# size of the sweep, every run of the layer was faster than every run of the core.  Far above the core's single-launch limit
# (MLDSA_OPT_SMALL_FUSED, 256 ops).
VFY_MIN_OPS = {44: 24576, 65: 16384, 87: 65536}

# Ph (src/types.rs:5-12) and hash_message (src/hashing.rs:316-354): the pre-hash of HashML-DSA is message-length-bound
# host work; the device sees OID || PH(M) as the message of a MODE_PREHASH call.
PH_SHA256, PH_SHA512, PH_SHAKE128 = "SHA256", "SHA512", "SHAKE128"
# FIPS 204 §5.4 allows any approved hash or XOF: the nine other functions of the NIST arc 2.16.840.1.101.3.4.2.*
PH_SHA384, PH_SHA224, PH_SHA512_224, PH_SHA512_256 = "SHA384", "SHA224", "SHA512_224", "SHA512_256"
PH_SHA3_224, PH_SHA3_256, PH_SHA3_384, PH_SHA3_512, PH_SHAKE256 = "SHA3_224", "SHA3_256", "SHA3_384", "SHA3_512", "SHAKE256"
_PH_OID = bytes([0x06, 0x09, 0x60, 0x86, 0x48, 0x01, 0x65, 0x03, 0x04, 0x02])
# Ph -> (last OID byte, hashlib name, bytes of output asked of an XOF or None, MLDSA_PH_* of include/mldsa_ph.h); list-level
# calls choose between the hashlib loop and the same pre-hash on the device with prehash="host" | "device"
_PH_TABLE = {
    PH_SHA256: (0x01, "sha256", None, _ph_lib.PH_SHA256),
    PH_SHA384: (0x02, "sha384", None, _ph_lib.PH_SHA384),
    PH_SHA512: (0x03, "sha512", None, _ph_lib.PH_SHA512),
    PH_SHA224: (0x04, "sha224", None, _ph_lib.PH_SHA224),
    PH_SHA512_224: (0x05, "sha512_224", None, _ph_lib.PH_SHA512_224),
    PH_SHA512_256: (0x06, "sha512_256", None, _ph_lib.PH_SHA512_256),
    PH_SHA3_224: (0x07, "sha3_224", None, _ph_lib.PH_SHA3_224),
    PH_SHA3_256: (0x08, "sha3_256", None, _ph_lib.PH_SHA3_256),
    PH_SHA3_384: (0x09, "sha3_384", None, _ph_lib.PH_SHA3_384),
    PH_SHA3_512: (0x0A, "sha3_512", None, _ph_lib.PH_SHA3_512),
    PH_SHAKE128: (0x0B, "shake_128", 32, _ph_lib.PH_SHAKE128),
    PH_SHAKE256: (0x0C, "shake_256", 64, _ph_lib.PH_SHAKE256),
}
_PH_ABI = {name: row[3] for name, row in _PH_TABLE.items()}
_PH_NAMES = "Ph: " + ", ".join(_PH_TABLE)


def _ph_code(ph):
    if ph not in _PH_ABI:
        raise ValueError(_PH_NAMES)
    return _PH_ABI[ph]


def _check_prehash(prehash):
    if prehash not in ("host", "device"):
        raise ValueError('prehash: "host" or "device"')
    return prehash == "device"


class OsRng:
    """rand_core::OsRng as the reference's default generator (src/traits.rs:45, 157, 250): the kernel's CSPRNG"""

    def fill_bytes(self, n):
        import os
        return os.urandom(n)


def hash_message(message, ph):
    """OID || PH(M): DER object identifier of the hash (11 bytes) followed by its digest (28 ... 64 bytes; 32 of SHAKE128, 64 of SHAKE256)."""
    import hashlib
    message = bytes(message)
    if not isinstance(ph, str) or ph not in _PH_TABLE:
        raise ValueError(_PH_NAMES)
    oid_last, name, xof_len, _ = _PH_TABLE[ph]
    h = hashlib.new(name, message)
    return _PH_OID + bytes([oid_last]) + (h.digest(xof_len) if xof_len else h.digest())


def external_mu(tr, message, ctx=b"", mode=MODE_PURE):
    """mu = H(BytesToBits(tr) || M', 64) on the host (FIPS 204 Algorithm 7 line 6): what a client that holds the message and the
    key's 64-byte tr sends to a device that signs or verifies from mu (verify_mu / try_sign_mu_with_seed).  M' as the three modes
    format it: MODE_INTERNAL M; MODE_PURE 0x00 | len(ctx) | ctx | M; MODE_PREHASH 0x01 | len(ctx) | ctx | M with M =
    hash_message(...) = OID || PH(M)."""
    import hashlib
    tr, message, ctx = bytes(tr), bytes(message), bytes(ctx)
    if len(tr) != 64:
        raise ValueError("tr: 64 bytes expected")
    if mode == MODE_INTERNAL:
        m_prime = message
    elif mode in (MODE_PURE, MODE_PREHASH):
        if len(ctx) > 255:
            raise ValueError("ctx too long (at most 255 bytes)")
        m_prime = bytes([1 if mode == MODE_PREHASH else 0, len(ctx)]) + ctx + message
    else:
        raise ValueError("mode: MODE_PURE, MODE_INTERNAL or MODE_PREHASH")
    return hashlib.shake_256(tr + m_prime).digest(64)


FORM_SEED, FORM_EXPANDED, FORM_BOTH = "seed", "expanded", "both"


def private_key_forms(seed=None, expanded=None):
    """Names the encoding a private key arrived in and the route it takes to the device.  The certificate profile for ML-DSA gives a
    private key three encodings: the 32-byte seed xi alone (preferred), the expanded wire key alone, or both -- and asks an importer
    of "both" to check that the expanded key is the one the seed generates.  Returns (form, route):
      (FORM_SEED, "expand_seeds")            MlDsa.expand_seeds_device
      (FORM_EXPANDED, "sk_expand")           MlDsa.private_keys_from_bytes
      (FORM_BOTH, "check_then_expand")       MlDsa.check_seeds_device, then expand_seeds_device for the keys that match
    Pure Python: lengths only (the expanded key's length is the parameter set's, checked where it is used); no ASN.1."""
    if seed is None and expanded is None:
        raise ValueError("a private key needs a seed, an expanded key or both")
    for name, key in (("seed", seed), ("expanded key", expanded)):
        # bytes(32) would be 32 zero bytes: only bytes-like objects are keys
        if key is not None and not isinstance(key, (bytes, bytearray, memoryview)):
            raise TypeError(f"{name}: bytes, bytearray or memoryview expected, not {type(key).__name__}")
    if seed is not None and memoryview(seed).nbytes != _seed_lib.SEED_LEN:
        raise ValueError(f"seed: {_seed_lib.SEED_LEN} bytes expected")
    if expanded is not None and memoryview(expanded).nbytes == 0:
        raise ValueError("expanded key: empty")
    if expanded is None:
        return FORM_SEED, "expand_seeds"
    if seed is None:
        return FORM_EXPANDED, "sk_expand"
    return FORM_BOTH, "check_then_expand"


# parameter set -> (K, L, eta): what the layout of a wire private key depends on (FIPS 204 Table 1)
_SK_SHAPE = {44: (4, 4, 2), 65: (6, 5, 4), 87: (8, 7, 2)}


def private_key_faults(pset, sk_bytes):
    """The range check skDecode (FIPS 204 Algorithm 25, lines 3 and 6) leaves to the importer, on the host: one uint8 per key with
    _keycheck_lib.KEY_S1_RANGE (1) set where a field of the key's s1 section is above 2 eta -- a coefficient outside [-eta, eta] --
    and KEY_S2_RANGE (2) likewise for s2; 0 = both vectors in range.  sk_bytes: one wire key (bytes-like), a list of them, or a uint8
    array of n * SK_LEN bytes.  Pure numpy, no library and no device: what MlDsa.check_private_keys_device(level="range") reports."""
    if pset not in _SK_SHAPE:
        raise ValueError(f"unknown parameter set {pset!r}")
    k, l, eta = _SK_SHAPE[pset]
    bits = 3 if eta == 2 else 4
    sk_len = 128 + 32 * bits * (l + k) + 416 * k
    if isinstance(sk_bytes, (bytes, bytearray, memoryview)):
        sk_bytes = [sk_bytes]
    if isinstance(sk_bytes, np.ndarray):
        a = np.ascontiguousarray(sk_bytes, dtype=np.uint8).reshape(-1)
    else:
        a = np.frombuffer(b"".join(bytes(b) for b in sk_bytes), dtype=np.uint8)
    if a.size % sk_len:
        raise ValueError(f"sk: {a.size} bytes are not a multiple of SK_LEN = {sk_len}")
    a = a.reshape(-1, sk_len)
    region = np.unpackbits(a[:, 128:128 + 32 * bits * (l + k)], axis=1, bitorder="little")
    fields = region.reshape(a.shape[0], (l + k) * 256, bits).astype(np.uint8) @ (1 << np.arange(bits)).astype(np.uint8)
    over = fields > 2 * eta
    return (over[:, :l * 256].any(axis=1) * _keycheck_lib.KEY_S1_RANGE + over[:, l * 256:].any(axis=1) * _keycheck_lib.KEY_S2_RANGE).astype(np.uint8)


def _np_ptr(a):
    """_optr for host memory: a numpy array's address, None -> NULL"""
    return C.c_void_p(0) if a is None else C.c_void_p(a.ctypes.data)


def _cat(items):
    """list of bytes -> (their bytes joined, uint64 offsets[n + 1]); b"\0" stands in for an empty buffer, so that what holds it
    has an address"""
    lens = np.fromiter((len(b) for b in items), dtype=np.uint64, count=len(items))
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return b"".join(bytes(b) for b in items) or b"\0", off


def _cat_with_offsets(items, device):
    """list of bytes -> (uint8 device buffer, uint64 offsets[n + 1] on device)"""
    flat, off = _cat(items)
    buf = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(device)
    return buf, torch.from_numpy(off.view(np.int64)).to(device)


class PublicKeys:
    """n expanded public keys: PublicKey { rho, tr, t1_d2_hat_mont } (src/types.rs:35-41)."""

    def __init__(self, pset, rho, tr, t1_d2_hat_mont):
        self.pset, self.rho, self.tr, self.t1_d2_hat_mont = pset, rho, tr, t1_d2_hat_mont

    def __len__(self):
        return self.rho.shape[0]


class PrivateKeys:
    """n expanded private keys (src/types.rs:19-28).  Like the reference's `Zeroize, ZeroizeOnDrop` struct
    the secret fields are wiped when the object goes away (before their memory returns to the allocator)."""

    def __init__(self, pset, rho, cap_k, tr, s_1_hat_mont, s_2_hat_mont, t_0_hat_mont):
        self.pset, self.rho, self.cap_k, self.tr = pset, rho, cap_k, tr
        self.s_1_hat_mont, self.s_2_hat_mont, self.t_0_hat_mont = s_1_hat_mont, s_2_hat_mont, t_0_hat_mont

    def __len__(self):
        return self.rho.shape[0]

    def zeroize(self):
        for t in (self.cap_k, self.s_1_hat_mont, self.s_2_hat_mont, self.t_0_hat_mont):
            if t is not None:
                t.zero_()

    def __del__(self):
        try:
            self.zeroize()
        except Exception:
            pass


def _sk_ptrs(sks, ptr=_ptr):
    """the fields of a PrivateKeys in the order every call of the C ABI takes them: rho, K, tr, s1, s2, t0.  ptr=_optr where a
    missing field goes to the library as NULL (the slices of sign_group)."""
    return (ptr(sks.rho), ptr(sks.cap_k), ptr(sks.tr), ptr(sks.s_1_hat_mont), ptr(sks.s_2_hat_mont), ptr(sks.t_0_hat_mont))


def _check_key_idx(key_idx, n_keys, n_ops):
    """Host-side courtesy check (the library itself also refuses out-of-range indices per op).
    A uint32 array is passed through without a copy."""
    if key_idx is None:
        if n_keys < n_ops:
            raise ValueError(f"{n_ops} operations but only {n_keys} keys and no key_idx")
        return None
    a = np.asarray(key_idx)
    if a.dtype != np.uint32:
        a64 = a.astype(np.int64)
        if n_ops and a64.size and a64.min() < 0:
            raise IndexError(f"key_idx out of range (n_keys = {n_keys})")
        a = a64.astype(np.uint32) if (not a64.size or a64.max() < 2 ** 32) else np.full(a64.shape, 0xFFFFFFFF, np.uint32)
    if a.shape != (n_ops,):
        raise ValueError("key_idx: one entry per operation expected")
    if n_ops and int(a.max()) >= n_keys:
        raise IndexError(f"key_idx out of range (n_keys = {n_keys})")
    return np.ascontiguousarray(a)


class MlDsa:
    """One parameter set (src/lib.rs:639-656 / 681-698 / 723-740) on one GPU."""

    def __init__(self, pset, device=0, hotpath=None):
        self.pset = pset
        self.hp = hotpath or HotPath(device)
        self.lib = self.hp.lib
        p = _lib.get_params(pset)
        self.params = p
        self.PK_LEN, self.SK_LEN, self.SIG_LEN = p.pk_len, p.sk_len, p.sig_len
        self.device = self.hp.device

    # ---- Verifier (src/traits.rs:330-362; src/lib.rs:364-411) -------------------------
    def verify(self, pks, messages, sigs, ctxs=None, key_idx=None, mode=MODE_PURE):
        """PublicKey::verify for a batch: returns a bool array, one entry per operation.

        `sigs`: uint8 CUDA tensor [n_ops, SIG_LEN] or a list of byte strings (a signature of
        the wrong length verifies as False, like a failed `try_into()` in the reference's
        callers).  `ctxs`: list of byte strings or None (= empty)."""
        return self._verify_batch(pks, messages, sigs, ctxs, key_idx,
                                  lambda *a: self.verify_device(pks, *a, mode=mode))

    def _verify_batch(self, pks, messages, sigs, ctxs, key_idx, run):
        """verify()'s host side around run(msg_buf, msg_off, sigs, ok, n_ops, ctx_buf, ctx_off, key_idx)"""
        n_ops = len(messages)
        sigs, wrong_len = self._sig_rows(sigs)
        msg_buf, msg_off, ctx_buf, ctx_off = self._stage_strings(messages, ctxs)
        kidx = self._stage_key_idx(key_idx, len(pks), n_ops)
        ok = torch.zeros(max(n_ops, 1), dtype=torch.uint8, device=self.device)
        run(msg_buf, msg_off, sigs, ok, n_ops, ctx_buf, ctx_off, kidx)
        return self._verdicts(ok, n_ops, wrong_len)

    # ---- host side of the list-level device calls: each piece written once ----------------
    def _stage_strings(self, messages, ctxs):
        """messages and optional contexts (lists of byte strings) -> (msg_buf, msg_off, ctx_buf, ctx_off) on the device; no
        contexts: ctx_buf = ctx_off = None"""
        msg_buf, msg_off = _cat_with_offsets(messages, self.device)
        ctx_buf = ctx_off = None
        if ctxs is not None:
            ctx_buf, ctx_off = _cat_with_offsets(ctxs, self.device)
        return msg_buf, msg_off, ctx_buf, ctx_off

    def _stage_key_idx(self, key_idx, n_keys, n_ops, wrap=True):
        """key_idx checked (_check_key_idx) and uploaded as the int32 tensor the device calls take, or None.  wrap: without a
        key_idx and with n_keys != n_ops, op i uses key i mod n_keys; wrap=False leaves fewer keys than ops to _check_key_idx,
        which raises."""
        if wrap and key_idx is None and n_keys != n_ops:
            key_idx = np.arange(n_ops, dtype=np.uint32) % n_keys
        key_idx = _check_key_idx(key_idx, n_keys, n_ops)
        return None if key_idx is None else torch.as_tensor(key_idx.view(np.int32)).to(self.device)

    def _sig_rows(self, sigs):
        """signatures as verify takes them -> (uint8 device tensor, wrong_len).  A list is uploaded with zeros in place of every
        signature of the wrong length and wrong_len marks those (bool array); a tensor passes through with wrong_len = None."""
        if isinstance(sigs, torch.Tensor):
            return sigs, None
        wrong_len = np.array([len(s) != self.SIG_LEN for s in sigs], dtype=bool)
        flat = b"".join(bytes(s) if len(s) == self.SIG_LEN else bytes(self.SIG_LEN) for s in sigs)
        return torch.frombuffer(bytearray(flat or b"\0"), dtype=torch.uint8).to(self.device), wrong_len

    def _verdicts(self, ok, n_ops, wrong_len=None):
        """waits for the device and reads ok[:n_ops] back as a bool array, False where _sig_rows found a wrong length"""
        torch.cuda.synchronize(self.device)
        res = ok[:n_ops].cpu().numpy().astype(bool)
        if wrong_len is not None:
            res &= ~wrong_len
        return res

    def hash_verify(self, pks, messages, sigs, ctxs=None, ph=PH_SHA512, key_idx=None, prehash="host"):
        """PublicKey::hash_verify (src/traits.rs:361, src/lib.rs:391-411) for a batch: HashML-DSA.Verify with the
        pre-hash `ph` computed on the host (prehash="host") or on the device (prehash="device", mldsa_hash_verify)."""
        if _check_prehash(prehash):
            code = _ph_code(ph)
            return self._verify_batch(pks, messages, sigs, ctxs, key_idx,
                                      lambda *a: self.hash_verify_device(pks, *a[:5], code, *a[5:]))
        return self.verify(pks, [hash_message(m, ph) for m in messages], sigs, ctxs=ctxs, key_idx=key_idx, mode=MODE_PREHASH)

    def expand_a_for_keys(self, keys):
        """A_hat = ExpandA(rho) of every key of a PublicKeys / PrivateKeys batch: the `cap_a_hat`
        pre-compute the reference lists as an open optimisation (benches/README.md:4-8).  Pass the result
        as `a_hat=` to verify_device / sign_device to skip the per-operation ExpandA."""
        return self.hp.expand_a(self.pset, keys.rho.contiguous())

    def verify_route(self, n_ops, a_hat=None):
        """the library a verify_device call of this shape runs on: "vfy" (libmldsa_vfy.so, the large-batch pass) from VFY_MIN_OPS[set]
        ops on when A_hat is derived per op, else "core" """
        return "vfy" if a_hat is None and VFY_MIN_OPS[self.pset] <= n_ops <= _vfy_lib.MAX_OPS else "core"

    def _vfy_scratch(self, lib, n_ops):
        """(pointer, bytes) of this object's scratch for the large-batch pass: one tensor, grown on demand, used in stream order"""
        nb = lib.mldsa_vfy_scratch_bytes(self.pset, n_ops)
        buf = getattr(self, "_vfy_buf", None)
        if buf is None or buf.numel() < nb:
            self._vfy_buf = buf = None  # (the old tensor goes back to the caching allocator before the larger one is asked for)
            self._vfy_buf = buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
        return _ptr(buf), buf.numel()

    def verify_device(self, pks, msg_buf, msg_off, sigs, ok, n_ops, ctx_buf=None, ctx_off=None, key_idx=None,
                      mode=MODE_PURE, a_hat=None):
        """Same, everything already resident in HBM (what bench.py times)."""
        if self.verify_route(n_ops, a_hat) == "vfy":
            lib = _vfy_lib.load()
            self.hp._vfy_profile_sync(lib)
            self.hp._vfy_calls = getattr(self.hp, "_vfy_calls", 0) + 1  # (HotPath.stats counts them as direct calls)
            _vfy_lib.check(lib.mldsa_vfy_verify(
                self.hp._h, self.pset, mode, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(key_idx),
                _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf), _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops,
                *self._vfy_scratch(lib, n_ops), _stream(self.device)))
            return ok
        fn, first = (self.lib.mldsa_verify, pks.rho) if a_hat is None else (self.lib.mldsa_verify_cached_a, a_hat)
        _lib.check(fn(
            self.hp._h, self.pset, mode, _ptr(first), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(key_idx),
            _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf), _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops, _stream(self.device)))
        return ok

    def verify_pk_device(self, pk_bytes, msg_buf, msg_off, sigs, ok, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE):
        """mldsa_verify_pk: PublicKey::try_from_bytes + verify in one call -- pk_bytes = uint8 CUDA tensor [n_keys, PK_LEN] in wire format
        (key_idx None: op i uses key i).  Same verdicts as public_keys_from_bytes + verify_device."""
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        _lib.check(self.lib.mldsa_verify_pk(
            self.hp._h, self.pset, mode, _ptr(pk), pk.shape[0], _optr(key_idx), _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf),
            _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops, _stream(self.device)))
        return ok

    def verify_pk(self, pk_bytes, messages, sigs, ctxs=None, key_idx=None, mode=MODE_PURE, dedup=False):
        """PublicKey::try_from_bytes(pk)?.verify(message, sig, ctx) for a batch of wire-format keys (src/lib.rs:471-475, 364-380).
        dedup=True: through verify_pk_dedup_device (equal keys are found on the device and expanded once); same verdicts."""
        n_ops = len(messages)
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        msg_buf, msg_off, ctx_buf, ctx_off = self._stage_strings(messages, ctxs)
        # stricter than verify: fewer keys than ops without a key_idx raises, and so does a signature of the wrong length
        kidx = self._stage_key_idx(key_idx, pk.shape[0], n_ops, wrap=False)
        sg = self._key_bytes(sigs, self.SIG_LEN, "sigs") if n_ops else torch.zeros((1, self.SIG_LEN), dtype=torch.uint8, device=self.device)
        ok = torch.zeros(max(n_ops, 1), dtype=torch.uint8, device=self.device)
        if dedup:
            self.verify_pk_dedup_device(pk, msg_buf, msg_off, sg, ok, n_ops, ctx_buf, ctx_off, kidx, mode)
        else:
            self.verify_pk_device(pk, msg_buf, msg_off, sg, ok, n_ops, ctx_buf, ctx_off, kidx, mode)
        return self._verdicts(ok, n_ops)

    # ---- equal wire-format keys found on the device (include/mldsa_keys.h) ------------
    @staticmethod
    def _dedup_seed(seed):
        seed = OsRng().fill_bytes(16) if seed is None else bytes(seed)
        if len(seed) != 16:
            raise ValueError("seed: 16 bytes expected")
        return seed

    def dedup_public_keys_device(self, pk_bytes, seed=None, hash_bits=64, table_rows=None):
        """mldsa_keys_dedup: (row_of [n] int32, table [table_rows, PK_LEN] uint8, n_rows [1] int32), all on the device and
        asynchronous on the current stream.  table[row_of[i]] == pk[i]; rows are numbered in order of first occurrence and n_rows
        of them exist; the table holds the rows below table_rows (default: n, so every row).  seed: 16 bytes (None: from OsRng)."""
        lib = _keys_lib.load()
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        n = pk.shape[0]
        rows = n if table_rows is None else int(table_rows)
        row_of = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        table = torch.empty((max(rows, 1), self.PK_LEN), dtype=torch.uint8, device=self.device)
        n_rows = torch.empty(1, dtype=torch.int32, device=self.device)
        scratch = torch.empty(max(lib.mldsa_keys_dedup_scratch_bytes(self.pset, n), 16), dtype=torch.uint8, device=self.device)
        _keys_lib.check(lib.mldsa_keys_dedup(self.hp._h, self.pset, _ptr(pk), n, self._dedup_seed(seed), hash_bits, _ptr(row_of),
                                             _ptr(table) if rows else C.c_void_p(0), rows, _ptr(n_rows), _ptr(scratch), scratch.numel(),
                                             _stream(self.device)))
        return row_of[:n], table[:rows], n_rows

    # Rows the cached route of verify_pk_dedup_device may build when the caller does not say: the largest number of distinct keys
    # at which the route measured faster than mldsa_verify_pk at 65 536 ops (0.42 ... 0.52 of its time on the three sets; at 65 536
    # distinct keys it loses 11 ... 14 %; profiles/keys_dedup_bench.jsonl).
    DEDUP_MAX_CACHED_KEYS = 8192

    def dedup_verify_scratch(self, n, max_cached_keys=None):
        """device scratch for verify_pk_dedup_device calls of up to n ops and n keys, to be reused call after call on one stream"""
        cap = min(self.DEDUP_MAX_CACHED_KEYS if max_cached_keys is None else int(max_cached_keys), n)
        nb = _keys_lib.load().mldsa_keys_verify_scratch_bytes(self.pset, n, cap)
        return torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)

    def verify_pk_dedup_device(self, pk_bytes, msg_buf, msg_off, sigs, ok, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE,
                               seed=None, hash_bits=64, max_cached_keys=None, info=None, scratch=None):
        """mldsa_verify_pk_dedup: verify_pk_device's arguments and verdicts; equal keys are found on the device and the batch runs
        on the table of distinct keys when there are at most max_cached_keys of them (None: DEDUP_MAX_CACHED_KEYS).  Waits once for
        the current stream (the number of distinct keys decides the route).  info: a dict that receives n_rows and route.
        scratch: the caller's own device scratch, a uint8 tensor from dedup_verify_scratch() (None: one is allocated for the call)."""
        lib = _keys_lib.load()
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        n_keys = pk.shape[0]
        n_dedup = n_keys if key_idx is not None else n_ops
        cap = min(self.DEDUP_MAX_CACHED_KEYS if max_cached_keys is None else int(max_cached_keys), max(n_dedup, 0))
        nb = lib.mldsa_keys_verify_scratch_bytes(self.pset, max(n_dedup, n_ops), cap)
        if scratch is None:
            scratch = torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)
        elif scratch.numel() < nb:
            raise ValueError(f"scratch: {scratch.numel()} bytes, the call needs {nb}")
        out = _keys_lib.KeysInfo()
        _keys_lib.check(lib.mldsa_verify_pk_dedup(
            self.hp._h, self.pset, mode, _ptr(pk), n_keys, _optr(key_idx), _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf),
            _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops, self._dedup_seed(seed), hash_bits, cap, _ptr(scratch), scratch.numel(),
            C.byref(out), _stream(self.device)))
        if info is not None:
            info["n_rows"], info["route"] = int(out.n_rows), ("cached" if out.route == _keys_lib.ROUTE_CACHED else "plain")
        return ok

    # ---- SerDes (src/traits.rs:372-424; src/lib.rs:421-424, 471-475) ------------------
    def _key_bytes(self, keys, length, what):
        if isinstance(keys, torch.Tensor):
            if keys.dtype != torch.uint8 or keys.numel() % length:
                raise ValueError(f"{what}: expected uint8 tensor of n * {length} bytes")
            return keys.to(self.device).contiguous().view(-1, length)
        for b in keys:
            if len(b) != length:  # the reference's ByteArray is a fixed-size array type
                raise ValueError(f"{what}: wrong length {len(b)} (expected {length})")
        return torch.frombuffer(bytearray(b"".join(bytes(b) for b in keys)), dtype=torch.uint8).to(self.device).view(-1, length)

    def empty_public_keys(self, n):
        k = self.params.k
        return PublicKeys(self.pset, torch.empty((n, 32), dtype=torch.uint8, device=self.device),
                          torch.empty((n, 64), dtype=torch.uint8, device=self.device),
                          torch.empty((n, k, N), dtype=torch.int32, device=self.device))

    def empty_private_keys(self, n):
        k, l, dev = self.params.k, self.params.l, self.device
        return PrivateKeys(self.pset, torch.empty((n, 32), dtype=torch.uint8, device=dev), torch.empty((n, 32), dtype=torch.uint8, device=dev),
                           torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty((n, l, N), dtype=torch.int32, device=dev),
                           torch.empty((n, k, N), dtype=torch.int32, device=dev), torch.empty((n, k, N), dtype=torch.int32, device=dev))

    def public_keys_from_bytes(self, pk_bytes, out=None):
        """PublicKey::try_from_bytes for a batch -> PublicKeys (expand_public, src/ml_dsa.rs:477).
        out: a PublicKeys from empty_public_keys() to fill (same buffers every call: a repeated call shape)."""
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        n = pk.shape[0]
        o = out or self.empty_public_keys(n)
        _lib.check(self.lib.mldsa_pk_expand(self.hp._h, self.pset, _ptr(pk), _ptr(o.rho), _ptr(o.tr), _ptr(o.t1_d2_hat_mont), n, _stream(self.device)))
        return o

    def private_keys_from_bytes(self, sk_bytes, out=None):
        """PrivateKey::try_from_bytes for a batch -> PrivateKeys (expand_private, src/ml_dsa.rs:445)"""
        sk = self._key_bytes(sk_bytes, self.SK_LEN, "sk")
        n = sk.shape[0]
        o = out or self.empty_private_keys(n)
        _lib.check(self.lib.mldsa_sk_expand(self.hp._h, self.pset, _ptr(sk), *_sk_ptrs(o), n, _stream(self.device)))
        return o

    def public_keys_into_bytes(self, pks):
        """PublicKey::into_bytes for a batch (src/lib.rs:478-493): uint8 tensor [n, PK_LEN]"""
        n = len(pks)
        pk = torch.empty((n, self.PK_LEN), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mldsa_pk_into_bytes(self.hp._h, self.pset, _ptr(pks.rho), _ptr(pks.t1_d2_hat_mont), _ptr(pk), n, _stream(self.device)))
        return pk

    def private_keys_into_bytes(self, sks):
        """PrivateKey::into_bytes for a batch (src/lib.rs:427-465): uint8 tensor [n, SK_LEN]"""
        n = len(sks)
        sk = torch.empty((n, self.SK_LEN), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mldsa_sk_into_bytes(self.hp._h, self.pset, *_sk_ptrs(sks), _ptr(sk), n, _stream(self.device)))
        return sk

    def get_public_key(self, sks):
        """PrivateKey::get_public_key for a batch (src/lib.rs:345-349 -> private_to_public_key, ml_dsa.rs:502-559)"""
        n, k = len(sks), self.params.k
        rho = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        tr = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        t1 = torch.empty((n, k, N), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mldsa_get_public_key(self.hp._h, self.pset, _ptr(sks.rho), _ptr(sks.tr), _ptr(sks.s_1_hat_mont),
                                                 _ptr(sks.s_2_hat_mont), _ptr(rho), _ptr(tr), _ptr(t1), n, _stream(self.device)))
        return PublicKeys(self.pset, rho, tr, t1)

    # ---- host-memory entry points (numpy arrays in, numpy arrays out; staging inside the library) --------
    def _host_fn(self, op):
        return getattr(self.lib, f"mldsa_{op}_host")

    def _host_handle(self):
        return self.hp._h

    @staticmethod
    def _np_u8(a, row, what):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if row and a.size % row:
            raise ValueError(f"{what}: length is not a multiple of {row}")
        return a

    @staticmethod
    def _cat_host(items):
        flat, off = _cat(items)
        return np.frombuffer(flat, dtype=np.uint8), off

    @staticmethod
    def _host_strings(items, n_ops, what):
        """list of byte strings or (flat uint8, uint64 offsets[n_ops + 1]) -> validated contiguous (flat, offsets).
        The library walks offsets[0 .. n_ops] and reads flat[offsets[0] .. offsets[n_ops]): both are checked here, so a
        short list or a truncated buffer is a ValueError and never an out-of-bounds read on the C side."""
        if isinstance(items, tuple):
            flat, off = items
            flat = np.ascontiguousarray(flat, dtype=np.uint8)
            off = np.ascontiguousarray(off)
            if off.dtype != np.uint64:
                if off.size and (not np.issubdtype(off.dtype, np.integer) or int(off.min()) < 0):
                    raise ValueError(f"{what}: offsets must be non-negative integers")
                off = off.astype(np.uint64)
        else:
            if len(items) != n_ops:
                raise ValueError(f"{what}: {len(items)} entries for {n_ops} operations")
            flat, off = MlDsa._cat_host(items)
        if off.ndim != 1 or off.size != n_ops + 1:
            raise ValueError(f"{what}: offsets must have n_ops + 1 = {n_ops + 1} entries, got {off.size}")
        if n_ops and bool(np.any(off[1:] < off[:-1])):
            raise ValueError(f"{what}: offsets must be non-decreasing")
        if int(off[-1]) > flat.size:
            raise ValueError(f"{what}: offsets run past the end of the byte buffer ({int(off[-1])} > {flat.size})")
        return flat, off

    @staticmethod
    def _host_out(a, dtype, n_items, what):
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable or a.size < n_items:
            raise ValueError(f"{what}: a writable C-contiguous {np.dtype(dtype).name} array of at least {n_items} elements is required")
        return a

    def _verify_host_call(self, run, name, pk_bytes, messages, sigs, ctxs, key_idx, out):
        """verify_host's body around run(pk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, sigs, ok, n_ops): the library's call
        with its handle, set and mode or ph in front of these, and its check.  name: the calling method, for messages."""
        pk = self._np_u8(pk_bytes, self.PK_LEN, "pk")
        sg = self._np_u8(sigs, self.SIG_LEN, "sigs")
        n_keys, n_ops = pk.size // self.PK_LEN, sg.size // self.SIG_LEN
        mflat, moff = self._host_strings(messages, n_ops, "messages")
        cflat = coff = None
        if ctxs is not None:
            cflat, coff = self._host_strings(ctxs, n_ops, "ctxs")
        kidx = _check_key_idx(key_idx, n_keys, n_ops)
        # out: caller's (page-locked) uint8[n_ops]
        ok = self._host_out(out, np.uint8, n_ops, f"{name}: out") if out is not None else np.zeros(max(n_ops, 1), dtype=np.uint8)
        run(_np_ptr(pk), n_keys, _np_ptr(kidx), _np_ptr(mflat), _np_ptr(moff), _np_ptr(cflat), _np_ptr(coff), _np_ptr(sg), _np_ptr(ok),
            n_ops)
        return ok[:n_ops].astype(bool)

    def _sign_host_call(self, run, name, alg, sk_bytes, messages, rnd, ctxs, key_idx, out):
        """sign_host's body around run(sk, n_keys, key_idx, msgs, msg_off, ctxs, ctx_off, rnd, sigs, status, n_ops), as
        _verify_host_call.  alg: "ML-DSA" or "HashML-DSA", for the message of a refused ctx."""
        sk = self._np_u8(sk_bytes, self.SK_LEN, "sk")
        rn = self._np_u8(rnd, 32, "rnd")
        n_keys, n_ops = sk.size // self.SK_LEN, rn.size // 32
        mflat, moff = self._host_strings(messages, n_ops, "messages")
        cflat = coff = None
        if ctxs is not None:
            cflat, coff = self._host_strings(ctxs, n_ops, "ctxs")
        kidx = _check_key_idx(key_idx, n_keys, n_ops)
        if out is not None:
            if not isinstance(out, tuple) or len(out) != 2:
                raise ValueError(f"{name}: out = (sig uint8[n_ops, SIG_LEN], status int32[n_ops])")
            sig = self._host_out(out[0], np.uint8, n_ops * self.SIG_LEN, f"{name}: out[0] (signatures)")
            status = self._host_out(out[1], np.int32, n_ops, f"{name}: out[1] (status)")
            if sig.ndim == 2 and sig.shape[1] != self.SIG_LEN:
                raise ValueError(f"{name}: out[0] rows must be SIG_LEN = {self.SIG_LEN} bytes")
            sig = sig.reshape(-1)[:n_ops * self.SIG_LEN].reshape(n_ops, self.SIG_LEN) if n_ops else sig
        else:
            sig, status = np.zeros((max(n_ops, 1), self.SIG_LEN), dtype=np.uint8), np.zeros(max(n_ops, 1), dtype=np.int32)
        run(_np_ptr(sk), n_keys, _np_ptr(kidx), _np_ptr(mflat), _np_ptr(moff), _np_ptr(cflat), _np_ptr(coff), _np_ptr(rn), _np_ptr(sig),
            _np_ptr(status), n_ops)
        if n_ops and int(status[:n_ops].min()) < 0:
            raise ValueError(f"{alg}.Sign: ctx too long")
        return sig[:n_ops]

    def verify_host(self, pk_bytes, messages, sigs, ctxs=None, key_idx=None, mode=MODE_PURE, out=None):
        """mldsa_verify_host: wire-format public keys [n_keys, PK_LEN], signatures [n_ops, SIG_LEN] and messages
        in HOST memory (numpy); returns a bool array.  `messages` / `ctxs`: list of byte strings, or a
        (flat uint8 array, uint64 offsets[n + 1]) pair."""
        return self._verify_host_call(lambda *a: _lib.check(self._host_fn("verify")(self._host_handle(), self.pset, mode, *a)),
                                      "verify_host", pk_bytes, messages, sigs, ctxs, key_idx, out)

    def sign_host(self, sk_bytes, messages, rnd, ctxs=None, key_idx=None, mode=MODE_PURE, out=None):
        """mldsa_sign_host: wire-format private keys, messages and rnd in HOST memory; returns uint8 [n_ops, SIG_LEN].
        out: (sig uint8[n_ops, SIG_LEN], status int32[n_ops]) buffers of the caller (page-locked ones are filled by DMA)."""
        return self._sign_host_call(lambda *a: _lib.check(self._host_fn("sign")(self._host_handle(), self.pset, mode, *a)),
                                    "sign_host", "ML-DSA", sk_bytes, messages, rnd, ctxs, key_idx, out)

    def keygen_host(self, xi, out=None):
        """mldsa_keygen_host: seeds [n, 32] in host memory -> (pk [n, PK_LEN], sk [n, SK_LEN]) numpy arrays.
        out: (pk, sk) uint8 arrays to fill (page-locked ones are written by the DMA directly)."""
        x = self._np_u8(xi, 32, "xi")
        n = x.size // 32
        if out is not None:
            pk, sk = out
            if pk.dtype != np.uint8 or sk.dtype != np.uint8 or pk.size < n * self.PK_LEN or sk.size < n * self.SK_LEN \
                    or not pk.flags.c_contiguous or not sk.flags.c_contiguous:
                raise ValueError("keygen_host: out = (pk, sk) contiguous uint8 arrays of at least n keys")
        else:
            pk = np.zeros((max(n, 1), self.PK_LEN), dtype=np.uint8)
            sk = np.zeros((max(n, 1), self.SK_LEN), dtype=np.uint8)
        _lib.check(self._host_fn("keygen")(self._host_handle(), self.pset, _np_ptr(x), _np_ptr(pk), _np_ptr(sk), n))
        return pk[:n], sk[:n]

    # ---- KeyGen (src/traits.rs:8-114; src/lib.rs:247-250) ------------------------------
    def keygen_from_seed(self, xi, out=None):
        """KG::keygen_from_seed for a batch of 32-byte seeds -> (pk bytes, sk bytes) tensors
        [n, PK_LEN] / [n, SK_LEN] in FIPS 204 wire format (= the reference's into_bytes()).
        out: (pk, sk) tensors to fill."""
        xi = self._key_bytes(xi, 32, "xi")
        n = xi.shape[0]
        pk, sk = out or (torch.empty((n, self.PK_LEN), dtype=torch.uint8, device=self.device),
                         torch.empty((n, self.SK_LEN), dtype=torch.uint8, device=self.device))
        _lib.check(self.lib.mldsa_keygen(self.hp._h, self.pset, _ptr(xi), _ptr(pk), _ptr(sk), n, _stream(self.device)))
        return pk, sk

    def try_keygen_with_rng(self, rng, n=1):
        """KG::try_keygen_with_rng: xi drawn from the caller's rng (rng.fill_bytes(32) per key)"""
        xi = [rng.fill_bytes(32) for _ in range(n)]
        return self.keygen_from_seed(xi)

    def try_keygen(self, n=1):
        """KG::try_keygen (src/traits.rs:44-46): xi from the operating system's generator (OsRng)"""
        return self.try_keygen_with_rng(OsRng(), n)

    # ---- Signer (src/traits.rs:118-308; src/lib.rs:268-342, 586-600) -------------------
    def try_sign_with_rng(self, rng, sks, messages, ctxs=None, key_idx=None):
        """PrivateKey::try_sign_with_rng (src/lib.rs:268-296): one rnd = rng.fill_bytes(32) per op, drawn only after
        every ctx passed the length check (lib.rs:274 comes before lib.rs:282)"""
        if ctxs is not None and any(len(c) > 255 for c in ctxs):
            raise ValueError("ML-DSA.Sign: ctx too long")
        return self.try_sign_with_seed(sks, messages, [rng.fill_bytes(32) for _ in messages], ctxs=ctxs, key_idx=key_idx)

    def try_sign(self, sks, messages, ctxs=None, key_idx=None):
        """PrivateKey::try_sign (src/traits.rs:156-158): hedged signing with rnd from OsRng"""
        return self.try_sign_with_rng(OsRng(), sks, messages, ctxs=ctxs, key_idx=key_idx)

    def try_hash_sign_with_rng(self, rng, sks, messages, ctxs=None, ph=PH_SHA512, key_idx=None, prehash="host"):
        """PrivateKey::try_hash_sign_with_rng (src/lib.rs:310-342)"""
        if ctxs is not None and any(len(c) > 255 for c in ctxs):
            raise ValueError("HashML-DSA.Sign: ctx too long")
        return self.try_hash_sign_with_seed(sks, messages, [rng.fill_bytes(32) for _ in messages], ctxs=ctxs, ph=ph, key_idx=key_idx,
                                            prehash=prehash)

    def try_hash_sign(self, sks, messages, ctxs=None, ph=PH_SHA512, key_idx=None, prehash="host"):
        """PrivateKey::try_hash_sign (src/traits.rs:247-251)"""
        return self.try_hash_sign_with_rng(OsRng(), sks, messages, ctxs=ctxs, ph=ph, key_idx=key_idx, prehash=prehash)

    def try_sign_with_seed(self, sks, messages, rnd, ctxs=None, key_idx=None, mode=MODE_PURE):
        """PrivateKey::try_sign_with_seed for a batch: rnd = one 32-byte seed per op (zeros =
        deterministic signing).  Raises ValueError if any ctx is longer than 255 bytes
        (src/lib.rs:274).  Returns a uint8 tensor [n_ops, SIG_LEN]."""
        return self._sign_batch(sks, messages, rnd, ctxs, key_idx,
                                lambda mb, mo, rn, sg, n, cb, co, ki, st: self.sign_device(sks, mb, mo, rn, sg, n, cb, co, ki, mode, st))

    def _sign_batch(self, sks, messages, rnd, ctxs, key_idx, run):
        """try_sign_with_seed()'s host side around run(msg_buf, msg_off, rnd, sigs, n_ops, ctx_buf, ctx_off, key_idx, status)"""
        n_ops = len(messages)
        msg_buf, msg_off, ctx_buf, ctx_off = self._stage_strings(messages, ctxs)
        kidx = self._stage_key_idx(key_idx, len(sks), n_ops)
        rnd = self._key_bytes(rnd, 32, "rnd") if n_ops else torch.zeros((1, 32), dtype=torch.uint8, device=self.device)
        sigs = torch.empty((max(n_ops, 1), self.SIG_LEN), dtype=torch.uint8, device=self.device)
        status = torch.zeros(max(n_ops, 1), dtype=torch.int32, device=self.device)
        run(msg_buf, msg_off, rnd, sigs, n_ops, ctx_buf, ctx_off, kidx, status)
        torch.cuda.synchronize(self.device)
        if n_ops and int(status[:n_ops].min()) < 0:
            st = status[:n_ops].cpu().numpy()
            bad = int(np.flatnonzero(st < 0)[0])
            code = int(st[bad])
            what = {_lib.ERR_CTX_LEN: "ML-DSA.Sign: ctx too long",
                    _lib.ERR_PARAM: "ML-DSA.Sign: operation refused (malformed offsets or key index out of range)",
                    _lib.ERR_AGAIN: "ML-DSA.Sign: operation left unfinished by an asynchronous call"}.get(code, f"ML-DSA.Sign: status {code}")
            raise ValueError(f"{what} (op {bad})")
        return sigs[:n_ops]

    def try_hash_sign_with_seed(self, sks, messages, rnd, ctxs=None, ph=PH_SHA512, key_idx=None, prehash="host"):
        """PrivateKey::try_hash_sign_with_seed (src/traits.rs:280-284, src/lib.rs:310-342) for a batch: HashML-DSA.Sign
        with the pre-hash `ph` computed on the host (prehash="host") or on the device (prehash="device", mldsa_hash_sign)."""
        if _check_prehash(prehash):
            code = _ph_code(ph)
            return self._sign_batch(sks, messages, rnd, ctxs, key_idx,
                                    lambda mb, mo, rn, sg, n, cb, co, ki, st: self.hash_sign_device(sks, mb, mo, rn, sg, n, code, cb, co,
                                                                                                    ki, st))
        return self.try_sign_with_seed(sks, [hash_message(m, ph) for m in messages], rnd, ctxs=ctxs, key_idx=key_idx,
                                       mode=MODE_PREHASH)

    def sign_device(self, sks, msg_buf, msg_off, rnd, sigs, n_ops, ctx_buf=None, ctx_off=None, key_idx=None,
                    mode=MODE_PURE, status=None, a_hat=None, wait=True):
        """Everything already resident in HBM (what bench.py times).  wait=False -> mldsa_sign_async: the call
        only enqueues; an op the enqueued rounds leave unfinished (p < 1e-9 per call) has status
        MLDSA_ERR_AGAIN and must be signed again."""
        if a_hat is not None:
            fn, first = self.lib.mldsa_sign_cached_a, a_hat
        else:
            fn, first = (self.lib.mldsa_sign if wait else self.lib.mldsa_sign_async), sks.rho
        _lib.check(fn(
            self.hp._h, self.pset, mode, _ptr(first), *_sk_ptrs(sks)[1:], len(sks), _optr(key_idx), _ptr(msg_buf), _ptr(msg_off),
            _optr(ctx_buf), _optr(ctx_off), _ptr(rnd), _ptr(sigs), _optr(status), n_ops, _stream(self.device)))
        return sigs

    # ---- HashML-DSA with the pre-hash on the device (include/mldsa_ph.h) ------------------
    def _ph_scratch(self, code, n_ops):
        """device scratch of one call, from the caching allocator on the current stream (the call uses it in that stream's order)"""
        nb = _ph_lib.load().mldsa_ph_scratch_bytes(code, n_ops)
        return torch.empty(max(nb, 8), dtype=torch.uint8, device=self.device)

    @staticmethod
    def _ph_arg(ph):
        return ph if isinstance(ph, int) else _ph_code(ph)

    def prehash_device(self, msg_buf, msg_off, n_ops, ph):
        """mldsa_prehash: rows[n_ops, row_len] = OID || PH(M_i) (= hash_message(M_i, ph)), bad[n_ops] = 1 where the
        message pair is malformed (row all zero).  Returns (rows, bad); asynchronous on the current stream."""
        lib, code = _ph_lib.load(), self._ph_arg(ph)
        rl = lib.mldsa_ph_row_len(code)
        if rl < 0:
            raise ValueError(f"unknown ph {ph!r}")
        rows = torch.empty((max(n_ops, 1), rl), dtype=torch.uint8, device=self.device)
        bad = torch.empty(max(n_ops, 1), dtype=torch.uint8, device=self.device)
        _ph_lib.check(lib.mldsa_prehash(self.hp._h, code, _optr(msg_buf), _ptr(msg_off), _ptr(rows), _ptr(bad), n_ops,
                                        _stream(self.device)))
        return rows[:n_ops], bad[:n_ops]

    def hash_verify_device(self, pks, msg_buf, msg_off, sigs, ok, n_ops, ph, ctx_buf=None, ctx_off=None, key_idx=None):
        """mldsa_hash_verify: verify_device's arguments on RAW messages, the pre-hash `ph` computed on the device."""
        code = self._ph_arg(ph)
        scratch = self._ph_scratch(code, n_ops)
        _ph_lib.check(_ph_lib.load().mldsa_hash_verify(
            self.hp._h, self.pset, code, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(key_idx),
            _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf), _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops, _ptr(scratch), scratch.numel(),
            _stream(self.device)))
        return ok

    def hash_verify_pk_device(self, pk_bytes, msg_buf, msg_off, sigs, ok, n_ops, ph, ctx_buf=None, ctx_off=None, key_idx=None):
        """mldsa_hash_verify_pk: verify_pk_device's arguments (wire-format keys) on RAW messages, the pre-hash on the device."""
        code = self._ph_arg(ph)
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk")
        scratch = self._ph_scratch(code, n_ops)
        _ph_lib.check(_ph_lib.load().mldsa_hash_verify_pk(
            self.hp._h, self.pset, code, _ptr(pk), pk.shape[0], _optr(key_idx), _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf),
            _optr(ctx_off), _ptr(sigs), _ptr(ok), n_ops, _ptr(scratch), scratch.numel(), _stream(self.device)))
        return ok

    def hash_sign_device(self, sks, msg_buf, msg_off, rnd, sigs, n_ops, ph, ctx_buf=None, ctx_off=None, key_idx=None, status=None):
        """mldsa_hash_sign: sign_device's arguments on RAW messages, the pre-hash `ph` computed on the device.  Synchronous like
        mldsa_sign: signatures and statuses are final on return."""
        code = self._ph_arg(ph)
        scratch = self._ph_scratch(code, n_ops)
        _ph_lib.check(_ph_lib.load().mldsa_hash_sign(
            self.hp._h, self.pset, code, *_sk_ptrs(sks), len(sks), _optr(key_idx), _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf),
            _optr(ctx_off), _ptr(rnd), _ptr(sigs), _optr(status), n_ops, _ptr(scratch), scratch.numel(), _stream(self.device)))
        return sigs


    # ---- externally computed mu (include/mldsa_mu.h) ---------------------------------------
    def mu_device(self, tr, msg_buf, msg_off, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE):
        """mldsa_mu_compute: (mu [n_ops, 64] uint8, mu_flag [n_ops] int32) on the device, asynchronous on the current stream.
        tr: uint8 CUDA tensor [n_keys, 64] (the .tr of PublicKeys / PrivateKeys).  mu_flag: 0 hashed, 1 ctx longer than 255 bytes,
        2 malformed offsets or key index out of range; a flagged op's mu row is zero."""
        tr = tr.contiguous().view(-1, 64)
        mu = torch.empty((max(n_ops, 1), _mu_lib.MU_LEN), dtype=torch.uint8, device=self.device)
        flag = torch.empty(max(n_ops, 1), dtype=torch.int32, device=self.device)
        _mu_lib.check(_mu_lib.load().mldsa_mu_compute(
            self.hp._h, mode, _ptr(tr), tr.shape[0], _optr(key_idx), _optr(msg_buf), _ptr(msg_off), _optr(ctx_buf), _optr(ctx_off),
            _ptr(mu), _ptr(flag), n_ops, _stream(self.device)))
        return mu[:n_ops], flag[:n_ops]

    def mu_scratch(self, n_ops, sign=False):
        """device scratch of one full pass of verify_mu_device (sign=True: sign_mu_device) over n_ops operations; a smaller one,
        down to a pass of min(n_ops, 64) operations, makes the call run in several passes"""
        lib = _mu_lib.load()
        nb = (lib.mldsa_mu_sign_scratch_bytes if sign else lib.mldsa_mu_verify_scratch_bytes)(self.pset, n_ops)
        return torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)

    def verify_mu_device(self, pks, mu, sigs, ok, n_ops, key_idx=None, mu_flag=None, scratch=None):
        """mldsa_verify_mu: ML-DSA.Verify_internal from mu [n_ops, 64]; ok[op] = 1 iff accepted.  Asynchronous on the current
        stream.  scratch: a uint8 CUDA tensor from mu_scratch() (None: one is allocated for the call)."""
        if scratch is None:
            scratch = self.mu_scratch(n_ops)
        _mu_lib.check(_mu_lib.load().mldsa_verify_mu(
            self.hp._h, self.pset, _ptr(pks.rho), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(key_idx), _ptr(mu), _optr(mu_flag),
            _ptr(sigs), _ptr(ok), n_ops, _ptr(scratch), scratch.numel(), _stream(self.device)))
        return ok

    def sign_mu_device(self, sks, mu, rnd, sigs, n_ops, key_idx=None, mu_flag=None, status=None, scratch=None):
        """mldsa_sign_mu: ML-DSA.Sign_internal from mu [n_ops, 64] and rnd [n_ops, 32]; blocks like sign_device, and the scratch is
        all zero when it returns."""
        if scratch is None:
            scratch = self.mu_scratch(n_ops, sign=True)
        _mu_lib.check(_mu_lib.load().mldsa_sign_mu(
            self.hp._h, self.pset, _ptr(sks.rho), _ptr(sks.cap_k), _ptr(sks.s_1_hat_mont), _ptr(sks.s_2_hat_mont), _ptr(sks.t_0_hat_mont),
            len(sks), _optr(key_idx), _ptr(mu), _optr(mu_flag), _ptr(rnd), _ptr(sigs), _optr(status), n_ops, _ptr(scratch),
            scratch.numel(), _stream(self.device)))
        return sigs

    def _mu_rows(self, mus, n_ops):
        return self._key_bytes(mus, _mu_lib.MU_LEN, "mu") if n_ops else torch.zeros((1, _mu_lib.MU_LEN), dtype=torch.uint8, device=self.device)

    def verify_mu(self, pks, mus, sigs, key_idx=None):
        """ML-DSA.Verify with an externally computed mu (external_mu) per operation: returns a bool array.  mus: list of 64-byte
        strings or a uint8 tensor [n_ops, 64]; sigs as for verify (a signature of the wrong length verifies as False)."""
        n_ops = len(mus)
        sigs, wrong_len = self._sig_rows(sigs)
        ok = torch.zeros(max(n_ops, 1), dtype=torch.uint8, device=self.device)
        self.verify_mu_device(pks, self._mu_rows(mus, n_ops), sigs, ok, n_ops, self._stage_key_idx(key_idx, len(pks), n_ops))
        return self._verdicts(ok, n_ops, wrong_len)

    def try_sign_mu_with_seed(self, sks, mus, rnd, key_idx=None):
        """ML-DSA.Sign with an externally computed mu (external_mu) per operation and one 32-byte rnd each (zeros = deterministic):
        the signature try_sign_with_seed gives on the message behind mu.  Returns a uint8 tensor [n_ops, SIG_LEN]."""
        n_ops = len(mus)
        rnd = self._key_bytes(rnd, 32, "rnd") if n_ops else torch.zeros((1, 32), dtype=torch.uint8, device=self.device)
        sigs = torch.empty((max(n_ops, 1), self.SIG_LEN), dtype=torch.uint8, device=self.device)
        status = torch.zeros(max(n_ops, 1), dtype=torch.int32, device=self.device)
        self.sign_mu_device(sks, self._mu_rows(mus, n_ops), rnd, sigs, n_ops, self._stage_key_idx(key_idx, len(sks), n_ops), status=status)
        if n_ops and int(status[:n_ops].min()) < 0:
            bad = int(np.flatnonzero(status[:n_ops].cpu().numpy() < 0)[0])
            raise ValueError(f"ML-DSA.Sign from mu: operation refused (op {bad})")
        return sigs[:n_ops]


    # ---- private keys in seed form (include/mldsa_seed.h) -----------------------------------
    def seed_scratch(self, n_keys, what="expand"):
        """device scratch of one full pass of expand_seeds_device ("expand"), check_seeds_device ("check") or
        sign_from_seeds_device ("sign") over n_keys seeds; a smaller one, down to a pass of min(n_keys, 64) keys, makes the call run
        in several passes"""
        lib = _seed_lib.load()
        fn = {"expand": lib.mldsa_seed_expand_scratch_bytes, "check": lib.mldsa_seed_check_scratch_bytes,
              "sign": lib.mldsa_seed_sign_scratch_bytes}[what]
        return torch.empty(max(fn(self.pset, n_keys), 256), dtype=torch.uint8, device=self.device)

    def expand_seeds_device(self, xi, out=None, want_pk=False, scratch=None):
        """mldsa_seed_expand: ML-DSA.KeyGen_internal(xi) for a batch of 32-byte seeds, delivered as the PrivateKeys that the signing
        calls take -- no wire-format private key is written.  want_pk: also return the wire public keys, uint8 [n, PK_LEN].
        Asynchronous on the current stream; the scratch is all zero behind the call.  Returns PrivateKeys, or (PrivateKeys, pk)."""
        xi = self._key_bytes(xi, _seed_lib.SEED_LEN, "xi")
        n = xi.shape[0]
        o = out if out is not None else self.empty_private_keys(n)
        pk = torch.empty((n, self.PK_LEN), dtype=torch.uint8, device=self.device) if want_pk else None
        if scratch is None:
            scratch = self.seed_scratch(n)
        _seed_lib.check(_seed_lib.load().mldsa_seed_expand(
            self.hp._h, self.pset, _ptr(xi), *_sk_ptrs(o), _optr(pk), n, _ptr(scratch), scratch.numel(), _stream(self.device)))
        return (o, pk) if want_pk else o

    def check_seeds_device(self, xi, sk_bytes, scratch=None):
        """mldsa_seed_check: the consistency check of private keys that arrive as seed AND expanded key.  Returns a bool tensor:
        True where sk_bytes[i] is byte for byte the private key ML-DSA.KeyGen_internal(xi[i]) generates."""
        xi = self._key_bytes(xi, _seed_lib.SEED_LEN, "xi")
        sk = self._key_bytes(sk_bytes, self.SK_LEN, "sk")
        n = xi.shape[0]
        if sk.shape[0] != n:
            raise ValueError(f"{n} seeds but {sk.shape[0]} expanded keys")
        match = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        if scratch is None:
            scratch = self.seed_scratch(n, "check")
        _seed_lib.check(_seed_lib.load().mldsa_seed_check(self.hp._h, self.pset, _ptr(xi), _ptr(sk), _ptr(match), n, _ptr(scratch),
                                                          scratch.numel(), _stream(self.device)))
        return match[:n].bool()

    def sign_from_seeds_device(self, xi, msg_buf, msg_off, rnd, sigs, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE,
                               status=None, scratch=None):
        """mldsa_sign_seed: sign_device with the key table given as seeds xi (uint8 CUDA tensor [n_keys, 32]): the seeds are expanded
        once per call into the scratch, which is all zero when the call returns.  Blocks like sign_device."""
        n_keys = xi.shape[0]
        if scratch is None:
            scratch = self.seed_scratch(n_keys, "sign")
        _seed_lib.check(_seed_lib.load().mldsa_sign_seed(
            self.hp._h, self.pset, mode, _ptr(xi), n_keys, _optr(key_idx), _ptr(msg_buf), _ptr(msg_off), _optr(ctx_buf), _optr(ctx_off),
            _ptr(rnd), _ptr(sigs), _optr(status), n_ops, _ptr(scratch), scratch.numel(), _stream(self.device)))
        return sigs

    def try_sign_from_seeds(self, xi, messages, rnd, ctxs=None, key_idx=None, mode=MODE_PURE):
        """try_sign_with_seed with the private keys given as 32-byte seeds (list of bytes or uint8 tensor [n_keys, 32]): 32 bytes
        uploaded per key instead of SK_LEN, and no expanded key outlives the call.  Returns a uint8 tensor [n_ops, SIG_LEN]."""
        xi = self._key_bytes(xi, _seed_lib.SEED_LEN, "xi")
        return self._sign_batch(xi, messages, rnd, ctxs, key_idx,
                                lambda mb, mo, rn, sg, n, cb, co, ki, st: self.sign_from_seeds_device(xi, mb, mo, rn, sg, n, cb, co, ki, mode, st))

    def private_keys_from_forms(self, seed=None, expanded=None):
        """One private key in any of its three encodings (private_key_forms) -> PrivateKeys of length 1.  For "both" the expanded
        key is checked against the seed first: ValueError when they disagree."""
        form, _ = private_key_forms(seed, expanded)
        if form == FORM_EXPANDED:
            return self.private_keys_from_bytes([expanded])
        if form == FORM_BOTH and not bool(self.check_seeds_device([seed], [expanded])[0]):
            raise ValueError("private key: the expanded key is not the one the seed generates")
        return self.expand_seeds_device([seed])

    # ---- strict import of wire private keys (include/mldsa_keycheck.h) ------------------------
    def keycheck_scratch(self, n_keys):
        """device scratch of one full pass of the pair check over n_keys keys; a smaller one, down to a pass of min(n_keys, 64) keys,
        makes the call run in several passes"""
        nb = _keycheck_lib.load().mldsa_keycheck_scratch_bytes(self.pset, n_keys)
        return torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)

    @staticmethod
    def _keycheck_level(level):
        if level not in _keycheck_lib.LEVELS:
            raise ValueError('level: "range" or "pair"')
        return _keycheck_lib.LEVELS[level]

    def _sk_and_pk(self, sk_bytes, pk_bytes):
        sk = self._key_bytes(sk_bytes, self.SK_LEN, "sk")
        pk = self._key_bytes(pk_bytes, self.PK_LEN, "pk") if pk_bytes is not None else None
        if pk is not None and pk.shape[0] != sk.shape[0]:
            raise ValueError(f"{sk.shape[0]} private keys but {pk.shape[0]} public keys")
        return sk, pk

    def check_private_keys_device(self, sk_bytes, pk_bytes=None, level="pair", scratch=None):
        """mldsa_keypair_check (level="pair") or mldsa_sk_range_check (level="range") on wire private keys [n, SK_LEN]: a uint8 tensor
        with one verdict per key, 0 = good, else the KEY_* bits of _keycheck_lib -- S1_RANGE 1, S2_RANGE 2 (a coefficient outside
        [-eta, eta]), T0 4, TR 8 (the field does not belong to the key's rho, s1, s2), PK 16 (pk_bytes, wire public keys [n, PK_LEN],
        given and not the key's).  A key with a range bit reports no other.  Asynchronous on the current stream; the scratch of the
        pair check (keycheck_scratch(); None: allocated for the call) is all zero behind it."""
        lvl = self._keycheck_level(level)
        sk, pk = self._sk_and_pk(sk_bytes, pk_bytes)
        n = sk.shape[0]
        flag = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        lib = _keycheck_lib.load()
        if lvl == _keycheck_lib.LEVEL_RANGE:
            _keycheck_lib.check(lib.mldsa_sk_range_check(self.hp._h, self.pset, _ptr(sk), _ptr(flag), n, _stream(self.device)))
        else:
            if scratch is None:
                scratch = self.keycheck_scratch(n)
            _keycheck_lib.check(lib.mldsa_keypair_check(self.hp._h, self.pset, _ptr(sk), _optr(pk), _ptr(flag), n, _ptr(scratch),
                                                        scratch.numel(), _stream(self.device)))
        return flag[:n]

    def private_keys_try_from_bytes(self, sk_bytes, pk_bytes=None, level="pair", out=None, scratch=None):
        """The strict counterpart of private_keys_from_bytes (mldsa_sk_import): the keys are expanded and checked at `level` as
        check_private_keys_device checks them.  Raises ValueError naming the first flagged key and its bits (the fields of every
        flagged key are zero by then); otherwise returns the PrivateKeys, byte for byte those of private_keys_from_bytes."""
        lvl = self._keycheck_level(level)
        sk, pk = self._sk_and_pk(sk_bytes, pk_bytes)
        n = sk.shape[0]
        o = out or self.empty_private_keys(n)
        flag = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        if lvl == _keycheck_lib.LEVEL_PAIR and scratch is None:
            scratch = self.keycheck_scratch(n)
        _keycheck_lib.check(_keycheck_lib.load().mldsa_sk_import(
            self.hp._h, self.pset, lvl, _ptr(sk), _optr(pk), *_sk_ptrs(o), _ptr(flag), n, _optr(scratch),
            scratch.numel() if scratch is not None else 0, _stream(self.device)))
        torch.cuda.synchronize(self.device)
        verdict = flag[:n].cpu().numpy()
        if verdict.any():
            bad = int(np.flatnonzero(verdict)[0])
            raise ValueError(f"private key {bad}: {_keycheck_lib.bit_names(int(verdict[bad]))} (flag {int(verdict[bad])}); "
                             f"{int(np.count_nonzero(verdict))} of {n} keys refused")
        return o

    # ---- incremental pre-hash and HashML-DSA from host memory (include/mldsa_ph.h) -------------
    def prehash_stream(self, n_ops, ph):
        """mldsa_ph_init: fresh hash states for n_ops messages that arrive in pieces.  Returns a PrehashStream:
        update(piece_buf, piece_off) any number of times, then final() -> (rows, bad) as prehash_device gives them."""
        return PrehashStream(self, n_ops, ph)

    def _host_feed(self, loader, layer, staging_bytes):
        """the mldsa_<layer>_host of this staging size on this context (created on first use, kept)"""
        hosts = self.__dict__.setdefault("_host_feeds", {})
        h = hosts.get((layer, staging_bytes))
        if h is None:
            h = hosts[(layer, staging_bytes)] = _HostFeed(self.hp, staging_bytes, loader, f"mldsa_{layer}_host_create", f"mldsa_{layer}_host_destroy")
        return h.handle

    def _ph_host(self, staging_bytes):
        return self._host_feed(_ph_lib, "ph", staging_bytes)

    def hash_verify_host(self, pk_bytes, messages, sigs, ctxs=None, ph=PH_SHA512, key_idx=None, out=None, staging_bytes=0):
        """mldsa_hash_verify_host: verify_host's arguments on RAW messages in host memory; the pre-hash `ph` is computed on the
        device while the message bytes stream through two staging chunks of `staging_bytes` (0 = the library's default)."""
        code = self._ph_arg(ph)
        return self._verify_host_call(
            lambda *a: _ph_lib.check(_ph_lib.load().mldsa_hash_verify_host(self._ph_host(staging_bytes), self.pset, code, *a)),
            "hash_verify_host", pk_bytes, messages, sigs, ctxs, key_idx, out)

    def hash_sign_host(self, sk_bytes, messages, rnd, ctxs=None, ph=PH_SHA512, key_idx=None, out=None, staging_bytes=0):
        """mldsa_hash_sign_host: sign_host's arguments on RAW messages in host memory, the pre-hash `ph` on the device;
        returns uint8 [n_ops, SIG_LEN].  out: (sig uint8[n_ops, SIG_LEN], status int32[n_ops]) buffers of the caller."""
        code = self._ph_arg(ph)
        return self._sign_host_call(
            lambda *a: _ph_lib.check(_ph_lib.load().mldsa_hash_sign_host(self._ph_host(staging_bytes), self.pset, code, *a)),
            "hash_sign_host", "HashML-DSA", sk_bytes, messages, rnd, ctxs, key_idx, out)


    # ---- mu of messages in pieces or in host memory (include/mldsa_mus.h) ------------------------
    def mu_stream(self, tr, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE):
        """mldsa_mus_init: sponge states of n_ops messages that arrive in pieces, with tr and the ctx prefix of `mode` absorbed.
        tr, ctx_buf / ctx_off, key_idx: device tensors as for mu_device.  Returns a MuStream: update(piece_buf, piece_off) any
        number of times, then final() -> (mu, mu_flag) as mu_device gives them."""
        return MuStream(self, tr, n_ops, ctx_buf, ctx_off, key_idx, mode)

    def _mus_host(self, staging_bytes):
        return self._host_feed(_mus_lib, "mus", staging_bytes)

    def _upload(self, a):
        """a host array on the device; the bytes go through a ctypes view, so a read-only array needs no writable copy"""
        t = torch.empty(a.shape, dtype=torch.uint8, device=self.device)
        if a.size:
            _lib.check(self.lib.mldsa_memcpy_h2d(_ptr(t), _np_ptr(np.ascontiguousarray(a)), a.size, _stream(self.device)))
            torch.cuda.synchronize(self.device)
        return t

    def mu_host(self, tr, messages, ctxs=None, key_idx=None, mode=MODE_PURE, staging_bytes=0):
        """mldsa_mus_host_compute: (mu [n_ops, 64] uint8, mu_flag [n_ops] int32) on the device from RAW messages in HOST memory of
        any total size; the bytes stream through two staging chunks of `staging_bytes` (0 = the library's default), so device
        memory does not grow with the messages.  tr: uint8 CUDA tensor [n_keys, 64]; messages / ctxs: list of byte strings or a
        (flat uint8 array, uint64 offsets[n + 1]) pair in host memory; key_idx: None, an array, or an int32 CUDA tensor.
        Blocks: mu is complete on return."""
        tr = tr.contiguous().view(-1, 64)
        n_ops = len(messages) if not isinstance(messages, tuple) else len(messages[1]) - 1
        mflat, moff = self._host_strings(messages, n_ops, "messages")
        cflat = coff = None
        if ctxs is not None:
            cflat, coff = self._host_strings(ctxs, n_ops, "ctxs")
        if not isinstance(key_idx, torch.Tensor):
            key_idx = self._stage_key_idx(key_idx, tr.shape[0], n_ops)
        mu = torch.zeros((max(n_ops, 1), _mus_lib.MU_LEN), dtype=torch.uint8, device=self.device)
        flag = torch.zeros(max(n_ops, 1), dtype=torch.int32, device=self.device)
        # the call runs on the object's own streams: tr and key_idx must be complete, mu and mu_flag free of pending work
        torch.cuda.synchronize(self.device)
        _mus_lib.check(_mus_lib.load().mldsa_mus_host_compute(
            self._mus_host(staging_bytes), mode, _ptr(tr), tr.shape[0], _optr(key_idx), _np_ptr(mflat), _np_ptr(moff), _np_ptr(cflat),
            _np_ptr(coff), _ptr(mu), _ptr(flag), n_ops))
        return mu[:n_ops], flag[:n_ops]

    def verify_host_streamed(self, pk_bytes, messages, sigs, ctxs=None, key_idx=None, out=None, staging_bytes=0):
        """verify_host(mode=MODE_PURE) with the messages streamed: the keys are uploaded and expanded, mu_host hashes the raw
        messages in bounded device memory, verify_mu_device verifies from mu, the verdicts come back.  Returns a bool array."""
        pk = self._np_u8(pk_bytes, self.PK_LEN, "pk")
        sg = self._np_u8(sigs, self.SIG_LEN, "sigs")
        n_keys, n_ops = pk.size // self.PK_LEN, sg.size // self.SIG_LEN
        kidx = _check_key_idx(key_idx, n_keys, n_ops)
        ok_h = self._host_out(out, np.uint8, n_ops, "verify_host_streamed: out") if out is not None else np.zeros(max(n_ops, 1), dtype=np.uint8)
        if n_ops == 0:
            return ok_h[:0].astype(bool)
        pks = self.public_keys_from_bytes(self._upload(pk.reshape(n_keys, self.PK_LEN)))
        kidx_d = None if kidx is None else torch.as_tensor(kidx.view(np.int32)).to(self.device)
        mu, flag = self.mu_host(pks.tr, messages, ctxs, kidx_d, MODE_PURE, staging_bytes)
        ok = torch.zeros(n_ops, dtype=torch.uint8, device=self.device)
        self.verify_mu_device(pks, mu, self._upload(sg.reshape(n_ops, self.SIG_LEN)), ok, n_ops, kidx_d, mu_flag=flag)
        torch.cuda.synchronize(self.device)
        ok_h[:n_ops] = ok.cpu().numpy()
        return ok_h[:n_ops].astype(bool)

    def sign_host_streamed(self, sk_bytes, messages, rnd, ctxs=None, key_idx=None, out=None, staging_bytes=0):
        """sign_host(mode=MODE_PURE) with the messages streamed, as verify_host_streamed: mu_host, then sign_mu_device.  Returns
        uint8 [n_ops, SIG_LEN]; out: (sig uint8[n_ops, SIG_LEN], status int32[n_ops]) buffers of the caller.  The expanded private
        fields are zeroised before the call returns."""
        sk = self._np_u8(sk_bytes, self.SK_LEN, "sk")
        rn = self._np_u8(rnd, 32, "rnd")
        n_keys, n_ops = sk.size // self.SK_LEN, rn.size // 32
        kidx = _check_key_idx(key_idx, n_keys, n_ops)
        if out is not None:
            if not isinstance(out, tuple) or len(out) != 2:
                raise ValueError("sign_host_streamed: out = (sig uint8[n_ops, SIG_LEN], status int32[n_ops])")
            sig_h = self._host_out(out[0], np.uint8, n_ops * self.SIG_LEN, "sign_host_streamed: out[0] (signatures)")
            status_h = self._host_out(out[1], np.int32, n_ops, "sign_host_streamed: out[1] (status)")
            sig_h = sig_h.reshape(-1)[:n_ops * self.SIG_LEN].reshape(n_ops, self.SIG_LEN) if n_ops else sig_h
        else:
            sig_h, status_h = np.zeros((max(n_ops, 1), self.SIG_LEN), dtype=np.uint8), np.zeros(max(n_ops, 1), dtype=np.int32)
        if n_ops == 0:
            return sig_h[:0]
        sk_d = self._upload(sk.reshape(n_keys, self.SK_LEN))
        sks = self.private_keys_from_bytes(sk_d)
        try:
            kidx_d = None if kidx is None else torch.as_tensor(kidx.view(np.int32)).to(self.device)
            mu, flag = self.mu_host(sks.tr, messages, ctxs, kidx_d, MODE_PURE, staging_bytes)
            sigs = torch.zeros((n_ops, self.SIG_LEN), dtype=torch.uint8, device=self.device)
            status = torch.zeros(n_ops, dtype=torch.int32, device=self.device)
            self.sign_mu_device(sks, mu, self._upload(rn.reshape(n_ops, 32)), sigs, n_ops, kidx_d, mu_flag=flag,
                                status=status)
            torch.cuda.synchronize(self.device)
        finally:
            sks.zeroize()
            sk_d.zero_()
        sig_h[:n_ops] = sigs.cpu().numpy()
        status_h[:n_ops] = status.cpu().numpy()
        if int(status_h[:n_ops].min()) < 0:
            raise ValueError("ML-DSA.Sign: ctx too long")
        return sig_h[:n_ops]


class _HostFeed:
    """One mldsa_ph_host or mldsa_mus_host (staging chunks, streams, per-batch buffers) on a HotPath's context: `loader` is the
    layer's _*_lib module, `create` / `destroy` its entry points' names.  It keeps the HotPath alive; destroying it does not need
    the context, so it may follow HotPath.close()."""

    def __init__(self, hp, staging_bytes, loader, create, destroy):
        self.hp, self.loader, self.destroy = hp, loader, destroy
        out = C.c_void_p(0)
        loader.check(getattr(loader.load(), create)(hp._h, int(staging_bytes), C.byref(out)))
        self.handle = out

    def __del__(self):
        try:
            if self.handle:
                getattr(self.loader.load(), self.destroy)(self.handle)
            self.handle = None
        except Exception:
            pass


class MuStream:
    """Sponge states of n_ops messages in device memory (mldsa_mus_init / _update / _final).  Every call is asynchronous on the
    current stream; the states are used in stream order.  final() leaves the states as they are: more updates and another
    final() give the mu of the longer messages."""

    def __init__(self, m, tr, n_ops, ctx_buf=None, ctx_off=None, key_idx=None, mode=MODE_PURE):
        self.m, self.n_ops = m, int(n_ops)
        self.lib = _mus_lib.load()
        tr = tr.contiguous().view(-1, 64)
        self.state_bytes = self.lib.mldsa_mus_state_bytes(self.n_ops)
        self.state = torch.empty(max(self.state_bytes, 8), dtype=torch.uint8, device=m.device)
        _mus_lib.check(self.lib.mldsa_mus_init(m.hp._h, mode, _ptr(tr), tr.shape[0], _optr(key_idx), _optr(ctx_buf), _optr(ctx_off),
                                               _ptr(self.state), self.state_bytes, self.n_ops, _stream(m.device)))

    def update(self, piece_buf, piece_off):
        """op i absorbs piece_buf[piece_off[i] : piece_off[i + 1]] (device tensors; piece_off: n_ops + 1 uint64 offsets)"""
        _mus_lib.check(self.lib.mldsa_mus_update(self.m.hp._h, _ptr(self.state), self.state_bytes, _optr(piece_buf), _ptr(piece_off),
                                                 self.n_ops, _stream(self.m.device)))
        return self

    def final(self):
        """(mu [n_ops, 64] uint8, mu_flag [n_ops] int32): the shapes of mu_device"""
        mu = torch.empty((max(self.n_ops, 1), _mus_lib.MU_LEN), dtype=torch.uint8, device=self.m.device)
        flag = torch.empty(max(self.n_ops, 1), dtype=torch.int32, device=self.m.device)
        _mus_lib.check(self.lib.mldsa_mus_final(self.m.hp._h, _ptr(self.state), self.state_bytes, _ptr(mu), _ptr(flag), self.n_ops,
                                                _stream(self.m.device)))
        return mu[:self.n_ops], flag[:self.n_ops]


class PrehashStream:
    """Hash states of n_ops messages in device memory (mldsa_ph_init / _update / _final).  Every call is asynchronous on the
    current stream; the states are used in stream order."""

    def __init__(self, m, n_ops, ph):
        self.m, self.n_ops = m, int(n_ops)
        self.lib, self.code = _ph_lib.load(), m._ph_arg(ph)
        self.row_len = self.lib.mldsa_ph_row_len(self.code)
        if self.row_len < 0:
            raise ValueError(f"unknown ph {ph!r}")
        self.state_bytes = self.lib.mldsa_ph_state_bytes(self.code, self.n_ops)
        self.state = torch.empty(max(self.state_bytes, 8), dtype=torch.uint8, device=m.device)
        _ph_lib.check(self.lib.mldsa_ph_init(m.hp._h, self.code, _ptr(self.state), self.state_bytes, self.n_ops, _stream(m.device)))

    def update(self, piece_buf, piece_off):
        """op i absorbs piece_buf[piece_off[i] : piece_off[i + 1]] (device tensors; piece_off: n_ops + 1 uint64 offsets)"""
        _ph_lib.check(self.lib.mldsa_ph_update(self.m.hp._h, self.code, _ptr(self.state), self.state_bytes, _optr(piece_buf),
                                               _ptr(piece_off), self.n_ops, _stream(self.m.device)))
        return self

    def final(self):
        """(rows [n_ops, row_len] = OID || PH(M_i), bad [n_ops]): the shapes of prehash_device"""
        rows = torch.empty((max(self.n_ops, 1), self.row_len), dtype=torch.uint8, device=self.m.device)
        bad = torch.empty(max(self.n_ops, 1), dtype=torch.uint8, device=self.m.device)
        _ph_lib.check(self.lib.mldsa_ph_final(self.m.hp._h, self.code, _ptr(self.state), self.state_bytes, _ptr(rows), C.c_void_p(0),
                                              _ptr(bad), self.n_ops, _stream(self.m.device)))
        return rows[:self.n_ops], bad[:self.n_ops]


class MlDsaGroup(MlDsa):
    """The host-memory entry points over SEVERAL GPUs of one node: mldsa_group_create(device_ids) + mldsa_*_host_group
    (include/mldsa_hip.h "several GPUs of one node").  verify_host / sign_host / keygen_host take exactly the arguments of
    MlDsa's and return byte-identical results: the library cuts the batch into contiguous slices of ceil(B / N) ops, one
    worker thread and context per entry of `device_ids` (a device may be listed twice: two contexts on one GPU), results
    land directly in the caller's arrays.  Needs no torch: every pointer is host memory."""

    def __init__(self, pset, device_ids):
        self.pset = pset
        self.lib = _lib.load()
        p = _lib.get_params(pset)
        self.params = p
        self.PK_LEN, self.SK_LEN, self.SIG_LEN = p.pk_len, p.sk_len, p.sig_len
        self.device_ids = [int(d) for d in device_ids]
        ids = (C.c_int * len(self.device_ids))(*self.device_ids)
        g = C.c_void_p()
        _lib.check(self.lib.mldsa_group_create(ids, len(self.device_ids), C.byref(g)))
        self._g = g
        self.hp = None

    def __len__(self):
        return len(self.device_ids)

    def close(self):
        if getattr(self, "_g", None):
            self.lib.mldsa_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _host_fn(self, op):
        return getattr(self.lib, f"mldsa_{op}_host_group")

    def _host_handle(self):
        return self._g

    def ctx(self, i):
        """the i-th context of the group as a raw handle (mldsa_set_option / mldsa_reserve)"""
        return C.c_void_p(self.lib.mldsa_group_ctx(self._g, i))

    def set_option(self, option, value):
        for i in range(len(self)):
            _lib.check(self.lib.mldsa_set_option(self.ctx(i), option, value))

    # ---- device-resident slices: one process, one thread, N devices (mldsa_*_group) --------------------------
    def on_device(self, i):
        """an MlDsa bound to the i-th context of the group (its device, its workspace): expand keys and stage a slice's
        inputs there, then hand the slices to verify_group / sign_group / keygen_group"""
        h = HotPath.from_handle(self.ctx(i), self.device_ids[i])
        return MlDsa(self.pset, hotpath=h)

    @staticmethod
    def _slice_stream(t, stream):
        if stream is not None:
            return C.c_void_p(stream)
        with torch.cuda.device(t.device):
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def verify_group(self, slices, mode=MODE_PURE, wait=True):
        """mldsa_verify_group.  slices[i]: dict(pks=PublicKeys on device i, msg_buf, msg_off, sigs, ok, n_ops and optionally
        ctx_buf, ctx_off, key_idx, stream) -- the arguments of MlDsa.verify_device for slice i, tensors on device i."""
        arr = (_lib.VerifySlice * len(self))()
        for i, sl in enumerate(slices):
            pks = sl["pks"]
            arr[i] = _lib.VerifySlice(_optr(pks.rho), _optr(pks.tr), _optr(pks.t1_d2_hat_mont), len(pks), _optr(sl.get("key_idx")),
                                      _optr(sl["msg_buf"]), _optr(sl["msg_off"]), _optr(sl.get("ctx_buf")), _optr(sl.get("ctx_off")),
                                      _optr(sl["sigs"]), _optr(sl["ok"]), sl["n_ops"], self._slice_stream(sl["ok"], sl.get("stream")))
        _lib.check(self.lib.mldsa_verify_group(self._g, self.pset, mode, arr, 1 if wait else 0))

    def sign_group(self, slices, mode=MODE_PURE, wait=True):
        """mldsa_sign_group.  slices[i]: dict(sks=PrivateKeys on device i, msg_buf, msg_off, rnd, sigs, status, n_ops and
        optionally ctx_buf, ctx_off, key_idx, stream); wait=False signs with mldsa_sign_async semantics."""
        arr = (_lib.SignSlice * len(self))()
        for i, sl in enumerate(slices):
            sks = sl["sks"]
            arr[i] = _lib.SignSlice(*_sk_ptrs(sks, _optr), len(sks), _optr(sl.get("key_idx")), _optr(sl["msg_buf"]), _optr(sl["msg_off"]),
                                    _optr(sl.get("ctx_buf")), _optr(sl.get("ctx_off")), _optr(sl["rnd"]), _optr(sl["sigs"]),
                                    _optr(sl.get("status")), sl["n_ops"], self._slice_stream(sl["sigs"], sl.get("stream")))
        _lib.check(self.lib.mldsa_sign_group(self._g, self.pset, mode, arr, 1 if wait else 0))

    def keygen_group(self, slices, wait=True):
        """mldsa_keygen_group.  slices[i]: dict(xi, pk, sk, n_keys[, stream]), tensors on device i."""
        arr = (_lib.KeygenSlice * len(self))()
        for i, sl in enumerate(slices):
            arr[i] = _lib.KeygenSlice(_optr(sl["xi"]), _optr(sl["pk"]), _optr(sl["sk"]), sl["n_keys"], self._slice_stream(sl["pk"], sl.get("stream")))
        _lib.check(self.lib.mldsa_keygen_group(self._g, self.pset, arr, 1 if wait else 0))

    def sync(self):
        """mldsa_group_sync: waits for the streams of the last device-resident group call"""
        _lib.check(self.lib.mldsa_group_sync(self._g))

    def allgather(self, bufs, n_ops, use_rccl=-1):
        """mldsa_group_allgather over one uint8 tensor per device (N * ceil(n_ops / N) bytes each, slice i of bufs[i] filled)"""
        arr = (C.c_void_p * len(self))(*[b.data_ptr() for b in bufs])
        _lib.check(self.lib.mldsa_group_allgather(self._g, arr, n_ops, use_rccl))

    def shard(self, n_ops, part):
        """(first, count) of the slice part `part` owns: mldsa_group_shard (= multi_gpu.shard)"""
        a, c = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.mldsa_group_shard(n_ops, len(self), part, C.byref(a), C.byref(c)))
        return a.value, c.value


class MlDsaBatcher:
    """mldsa_batcher_*: the reference's ONE-operation-per-call surface (src/traits.rs:118-308, 330-362) for many host threads at once.
    verify / sign / keygen block the calling thread (ctypes releases the GIL for the duration), the library coalesces whatever
    the threads submit into batched calls on one context.  Byte strings in, byte strings / bool out."""

    def __init__(self, pset, device=0, max_batch=4096, max_wait_us=0, cache_keys=0, hotpath=None, device_ids=None):
        """device_ids: mldsa_batcher_create_on -- one lane (context + dispatcher thread + key table) per entry, owned by the batcher;
        otherwise one lane on `hotpath`'s context (or a new one on `device`)."""
        self.pset = pset
        p = _lib.get_params(pset)
        self.PK_LEN, self.SK_LEN, self.SIG_LEN = p.pk_len, p.sk_len, p.sig_len
        h = C.c_void_p()
        if device_ids is not None:
            self.hp = None
            self.lib = _lib.load()
            ids = (C.c_int * len(device_ids))(*device_ids)
            _lib.check(self.lib.mldsa_batcher_create_on(ids, len(device_ids), pset, max_batch, max_wait_us, cache_keys, C.byref(h)))
        else:
            self.hp = hotpath or HotPath(device)
            self.lib = self.hp.lib
            _lib.check(self.lib.mldsa_batcher_create(self.hp._h, pset, max_batch, max_wait_us, cache_keys, C.byref(h)))
        self._b = h

    def close(self):
        if getattr(self, "_b", None):
            self.lib.mldsa_batcher_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _fixed(b, n, what):
        b = bytes(b)
        if len(b) != n:
            raise ValueError(f"{what}: {len(b)} bytes, expected {n}")
        return b

    def verify(self, pk, message, sig, ctx=b"", mode=MODE_PURE):
        """PublicKey::try_from_bytes(pk)?.verify(message, sig, ctx) (src/lib.rs:364-380)"""
        pk, sig = self._fixed(pk, self.PK_LEN, "pk"), self._fixed(sig, self.SIG_LEN, "sig")
        message, ctx = bytes(message), bytes(ctx)
        ok = C.c_uint8(0)
        _lib.check(self.lib.mldsa_batcher_verify(self._b, mode, pk, message, len(message), ctx, len(ctx), sig, C.byref(ok)))
        return bool(ok.value)

    def sign(self, sk, message, rnd, ctx=b"", mode=MODE_PURE):
        """PrivateKey::try_from_bytes(sk)?.try_sign_with_seed(rnd, message, ctx) (src/lib.rs:268-296); raises MldsaError for |ctx| > 255"""
        sk, rnd = self._fixed(sk, self.SK_LEN, "sk"), self._fixed(rnd, 32, "rnd")
        message, ctx = bytes(message), bytes(ctx)
        sig = (C.c_uint8 * self.SIG_LEN)()
        _lib.check(self.lib.mldsa_batcher_sign(self._b, mode, sk, message, len(message), ctx, len(ctx), rnd, sig))
        return bytes(sig)

    def keygen_from_seed(self, xi):
        """KG::keygen_from_seed(xi) (src/lib.rs:247-250) -> (pk bytes, sk bytes)"""
        xi = self._fixed(xi, 32, "xi")
        pk, sk = (C.c_uint8 * self.PK_LEN)(), (C.c_uint8 * self.SK_LEN)()
        _lib.check(self.lib.mldsa_batcher_keygen(self._b, xi, pk, sk))
        return bytes(pk), bytes(sk)

    def forget_key(self, key):
        """take one key (pk or sk wire bytes) out of the device-resident tables: the host copy is cleared, a private key's device fields zeroed"""
        key = bytes(key)
        _lib.check(self.lib.mldsa_batcher_forget_key(self._b, key, len(key)))

    def flush_keys(self):
        _lib.check(self.lib.mldsa_batcher_flush_keys(self._b))

    def set_private_key_cache(self, on):
        """False: no private key stays in the table beyond the batch that used it (the caller's zeroize then ends the key's life)"""
        _lib.check(self.lib.mldsa_batcher_set_private_key_cache(self._b, 1 if on else 0))

    def stats(self):
        st = _lib.BatcherStats()
        _lib.check(self.lib.mldsa_batcher_get_stats(self._b, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}


# ---- verification from wire records (include/mldsa_rec.h) --------------------------------------------------------------------------
def records_blob(records, pad=0, front=0, fill=0xC3):
    """Lays records (pset, pk, message, sig, ctx) out in one buffer, field after field -- key, signature, message, context --, and
    describes them: (blob, ops) = (uint8 numpy array, numpy array of _rec_lib.OP_DTYPE, one mldsa_rec_op per record).
    pad: the gap in front of every field, one int or a sequence that is cycled through, so that a caller chooses every field's
    alignment; front: bytes in front of the first gap; the gaps hold `fill`."""
    pads = [int(pad)] if np.isscalar(pad) else [int(x) for x in pad]
    ops = np.zeros(len(records), dtype=_rec_lib.OP_DTYPE)
    parts, at, k = [bytes([fill]) * front], front, 0
    for i, (pset, pk, message, sig, ctx) in enumerate(records):
        if len(ctx) > 0xFFFF or len(message) > 0xFFFFFFFF:
            raise ValueError("records_blob: a context or message too long for its descriptor field")
        ops[i]["set"], ops[i]["msg_len"], ops[i]["ctx_len"] = pset, len(message), len(ctx)
        for name, field in (("pk_off", pk), ("sig_off", sig), ("msg_off", message), ("ctx_off", ctx)):
            gap = pads[k % len(pads)]
            k += 1
            parts += [bytes([fill]) * gap, bytes(field)]
            ops[i][name] = at + gap
            at += gap + len(field)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), ops


class MlDsaRecords:
    """Batched verification straight from serialized records on one GPU, any mix of parameter sets in one call: libmldsa_rec.so
    (include/mldsa_rec.h).  blob = uint8 CUDA tensor (any alignment: a slice will do), ops = uint8 CUDA tensor holding n_ops
    mldsa_rec_op descriptors (ops_tensor() uploads a numpy array of _rec_lib.OP_DTYPE)."""

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.rec = _rec_lib.load()
        self._sets = {}

    def set(self, pset):
        """the MlDsa of one parameter set on this object's context"""
        if pset not in self._sets:
            self._sets[pset] = MlDsa(pset, hotpath=self.hp)
        return self._sets[pset]

    def ops_tensor(self, ops):
        a = np.ascontiguousarray(ops, dtype=_rec_lib.OP_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(40, np.uint8)).to(self.device)

    @staticmethod
    def _n_ops(ops, n_ops):
        if ops.dtype != torch.uint8 or ops.numel() % 40:
            raise ValueError("ops: a uint8 tensor of n_ops * 40 bytes expected")
        return ops.numel() // 40 if n_ops is None else int(n_ops)

    def plan_device(self, blob, ops, n_ops=None):
        """mldsa_rec_plan, asynchronous on the current stream: (class_slot int32 [n_ops] -- (class << 30) | slot, to be read as
        uint32 --, totals int64 [10] -- ops per class 44 / 65 / 87 / refused, message bytes per class, context bytes per class --,
        plan uint8: the working memory pack_device takes)."""
        n = self._n_ops(ops, n_ops)
        class_slot = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        totals = torch.zeros(10, dtype=torch.int64, device=self.device)
        plan = torch.empty(max(self.rec.mldsa_rec_plan_bytes(n), 256), dtype=torch.uint8, device=self.device)
        _rec_lib.check(self.rec.mldsa_rec_plan(self.hp._h, _ptr(blob), blob.numel(), _ptr(ops), n, _ptr(class_slot), _ptr(totals), _ptr(plan),
                                               plan.numel(), _stream(self.device)))
        return class_slot[:n], totals, plan

    def pack_device(self, blob, ops, class_slot, totals, plan, n_ops=None, arena=None):
        """mldsa_rec_pack behind plan_device: waits for the current stream to read the totals (unless `totals` is already a
        _rec_lib.RecTotals), then packs asynchronously.  Returns {pset: dict(n, pk [n, PK_LEN], sigs [n, SIG_LEN], msgs, msg_off
        [n + 1], ctxs, ctx_off [n + 1], ok [n])}, every tensor a view of one arena -- what verify_pk_device, verify_pk_dedup_device
        or hash_verify_pk_device of MlDsa(pset) take."""
        n = self._n_ops(ops, n_ops)
        if not isinstance(totals, _rec_lib.RecTotals):
            torch.cuda.current_stream(self.device).synchronize()
            h = [int(x) for x in totals.cpu().tolist()]
            totals = _rec_lib.RecTotals()
            totals.n[:], totals.msg_bytes[:], totals.ctx_bytes[:] = h[0:4], h[4:7], h[7:10]
        need = self.rec.mldsa_rec_scratch_bytes(totals.n[0], totals.n[1], totals.n[2], sum(totals.msg_bytes), sum(totals.ctx_bytes))
        if arena is None:
            arena = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        out = _rec_lib.RecPacked()
        _rec_lib.check(self.rec.mldsa_rec_pack(self.hp._h, _ptr(blob), blob.numel(), _ptr(ops), n, _ptr(class_slot), _ptr(plan), plan.numel(),
                                               C.byref(totals), _ptr(arena), arena.numel(), C.byref(out), _stream(self.device)))
        base, packed = arena.data_ptr(), {}
        for c, pset in enumerate(_rec_lib.CLASS_SETS):
            k, m = out.c[c], self.set(pset)
            cut = lambda p, nbytes: arena[(p or base) - base:(p or base) - base + nbytes]  # noqa: E731
            packed[pset] = dict(
                n=int(k.n), pk=cut(k.pk, k.n * m.PK_LEN).view(int(k.n), m.PK_LEN), sigs=cut(k.sigs, k.n * m.SIG_LEN).view(int(k.n), m.SIG_LEN),
                msgs=cut(k.msgs, max(int(totals.msg_bytes[c]), 1)), msg_off=cut(k.msg_off, 8 * (k.n + 1)).view(torch.int64),
                ctxs=cut(k.ctxs, max(int(totals.ctx_bytes[c]), 1)), ctx_off=cut(k.ctx_off, 8 * (k.n + 1)).view(torch.int64), ok=cut(k.ok, k.n))
        return packed

    def verify_scratch(self, n_ops, msg_bytes, ctx_bytes):
        """device scratch that no verify_device call of up to n_ops ops with these byte totals can outgrow, whatever its mix"""
        nb = self.rec.mldsa_rec_front_bytes(n_ops) + self.rec.mldsa_rec_scratch_bytes_max(n_ops, msg_bytes, ctx_bytes)
        return torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)

    def verify_device(self, blob, ops, ok, n_ops=None, mode=MODE_PURE, scratch=None, info=None):
        """mldsa_rec_verify: ok[i] = mldsa_verify_pk's verdict on record i under its own parameter set, 0 for a refused record.
        Waits once for the current stream (the mix decides the layout).  scratch: a uint8 tensor, e.g. from verify_scratch(); None:
        one that holds any mix whose messages and contexts fit the blob four times over (a call that needs more raises MldsaError
        with MLDSA_ERR_NOMEM, and info names the need).  info: a dict that receives n44, n65, n87, refused, msg_bytes, ctx_bytes and
        scratch_needed."""
        n = self._n_ops(ops, n_ops)
        if scratch is None:
            scratch = self.verify_scratch(n, 4 * blob.numel(), 4 * blob.numel())
        out = _rec_lib.RecInfo()
        rc = self.rec.mldsa_rec_verify(self.hp._h, mode, _ptr(blob), blob.numel(), _ptr(ops), n, _ptr(ok), _ptr(scratch), scratch.numel(),
                                       C.byref(out), _stream(self.device))
        if info is not None and rc in (_lib.OK, _lib.ERR_NOMEM) and n:
            info.update(n44=int(out.n[0]), n65=int(out.n[1]), n87=int(out.n[2]), refused=int(out.n[3]), msg_bytes=int(out.msg_bytes),
                        ctx_bytes=int(out.ctx_bytes), scratch_needed=int(out.scratch_needed))
        _rec_lib.check(rc)
        return ok

    def verify(self, records, mode=MODE_PURE, dedup=False, pad=0):
        """A host list of (pset, pk, message, sig, ctx) -> a bool array, one verdict per record: the records are laid out in one
        blob (records_blob) and verified from it.  dedup=True: the blob is planned and packed, and each parameter set's arrays run
        through MlDsa(pset).verify_pk_dedup_device (equal keys are expanded once); same verdicts."""
        n = len(records)
        if n == 0:
            return np.zeros(0, dtype=bool)
        blob_h, ops_h = records_blob(records, pad=pad)
        blob = torch.from_numpy(blob_h.copy() if blob_h.size else np.zeros(1, np.uint8)).to(self.device)[:blob_h.size]
        ops = self.ops_tensor(ops_h)
        ok = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if not dedup:
            self.verify_device(blob, ops, ok, n, mode)
        else:
            class_slot, totals, plan = self.plan_device(blob, ops, n)
            packed = self.pack_device(blob, ops, class_slot, totals, plan, n)
            cs = class_slot.cpu().numpy().view(np.uint32)
            for c, pset in enumerate(_rec_lib.CLASS_SETS):
                k = packed[pset]
                if k["n"] == 0:
                    continue
                self.set(pset).verify_pk_dedup_device(k["pk"], k["msgs"], k["msg_off"], k["sigs"], k["ok"], k["n"], k["ctxs"], k["ctx_off"],
                                                      None, mode)
                mine = np.nonzero(cs >> 30 == c)[0]
                ok[torch.from_numpy(mine).to(self.device)] = k["ok"][torch.from_numpy((cs[mine] & 0x3FFFFFFF).astype(np.int64)).to(self.device)]
        torch.cuda.synchronize(self.device)
        return ok.cpu().numpy().astype(bool)


# ---- signing of request records (include/mldsa_recsign.h) ---------------------------------------------------------------------------
def sign_requests_blob(requests, pad=0, front=0, fill=0xC3, in_place=False):
    """Lays signing requests (pset, key, message, ctx, rnd or None) out in one buffer, field after field -- message, context, the 32
    bytes of rnd where there are any, and with in_place the hole the signature goes to --, and describes them: (blob, ops, out_len) =
    (uint8 numpy array, numpy array of _recsign_lib.OP_DTYPE, one mldsa_recsign_op per request, the length of the output buffer).
    key: the row of the parameter set's key table.  rnd None: the deterministic variant (no MLDSA_RECSIGN_RND flag).
    pad: the gap in front of every field and every hole, one int or a sequence that is cycled through, so that a caller chooses every
    field's alignment; front: bytes in front of the first gap; gaps and holes hold `fill`.  Without in_place the holes lie in a
    separate output buffer, laid out with the same gaps; with it they lie in the blob itself (out_len = the blob's length)."""
    pads = [int(pad)] if np.isscalar(pad) else [int(x) for x in pad]
    ops = np.zeros(len(requests), dtype=_recsign_lib.OP_DTYPE)
    parts, at, k, out_at = [bytes([fill]) * front], front, 0, front
    for i, (pset, key, message, ctx, rnd) in enumerate(requests):
        if pset not in _recsign_lib.CLASS_SETS:
            raise ValueError("sign_requests_blob: unknown parameter set")
        if len(ctx) > 0xFFFF or len(message) > 0xFFFFFFFF or (rnd is not None and len(rnd) != 32):
            raise ValueError("sign_requests_blob: a context or message too long for its descriptor field, or rnd not 32 bytes")
        sig_len = _lib.get_params(pset).sig_len
        ops[i]["set"], ops[i]["key"], ops[i]["msg_len"], ops[i]["ctx_len"] = pset, key, len(message), len(ctx)
        ops[i]["flags"] = 0 if rnd is None else _recsign_lib.FLAG_RND
        fields = [("msg_off", message), ("ctx_off", ctx)] + ([("rnd_off", rnd)] if rnd is not None else [])
        if in_place:
            fields.append(("sig_off", bytes([fill]) * sig_len))
        for name, field in fields:
            gap = pads[k % len(pads)]
            k += 1
            parts += [bytes([fill]) * gap, bytes(field)]
            ops[i][name] = at + gap
            at += gap + len(field)
        if not in_place:
            gap = pads[k % len(pads)]
            k += 1
            ops[i]["sig_off"] = out_at + gap
            out_at += gap + sig_len
    return np.frombuffer(b"".join(parts), dtype=np.uint8), ops, (at if in_place else out_at)


class MlDsaRecordSigner:
    """Batched signing straight from serialized requests on one GPU, any mix of parameter sets in one call, every signature written to
    its byte offset: libmldsa_recsign.so (include/mldsa_recsign.h).  blob, out = uint8 CUDA tensors (any alignment: a slice will do;
    out may be the blob), ops = uint8 CUDA tensor holding n_ops mldsa_recsign_op descriptors (ops_tensor() uploads a numpy array of
    _recsign_lib.OP_DTYPE), status = int32 CUDA tensor [n_ops].  The key tables are set_keys()'s PrivateKeys, used where they lie."""

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _recsign_lib.load()
        self._keys = {}

    def set_keys(self, pset, sks):
        """the key table of one parameter set: a PrivateKeys (kept by reference, never copied); None: the set is no longer served"""
        if pset not in _recsign_lib.CLASS_SETS or (sks is not None and sks.pset != pset):
            raise ValueError("set_keys: the keys of ML-DSA-%s expected" % pset)
        if sks is None:
            self._keys.pop(pset, None)
        else:
            self._keys[pset] = sks

    def _n_keys(self):
        return (C.c_size_t * 3)(*[len(self._keys[p]) if p in self._keys else 0 for p in _recsign_lib.CLASS_SETS])

    def _key_tables(self):
        t = (_recsign_lib.RecsignKeys * 3)()
        for c, pset in enumerate(_recsign_lib.CLASS_SETS):
            if pset in self._keys:
                sks = self._keys[pset]
                ptrs = [p.value if isinstance(p, C.c_void_p) else p for p in _sk_ptrs(sks)]
                t[c].n_keys = len(sks)
                t[c].rho, t[c].cap_k, t[c].tr, t[c].s_1_hat_mont, t[c].s_2_hat_mont, t[c].t_0_hat_mont = ptrs
        return t

    def ops_tensor(self, ops):
        a = np.ascontiguousarray(ops, dtype=_recsign_lib.OP_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(48, np.uint8)).to(self.device)

    @staticmethod
    def _n_ops(ops, n_ops):
        if ops.dtype != torch.uint8 or ops.numel() % 48:
            raise ValueError("ops: a uint8 tensor of n_ops * 48 bytes expected")
        return ops.numel() // 48 if n_ops is None else int(n_ops)

    def plan_device(self, ops, blob_len, out_len, n_ops=None):
        """mldsa_recsign_plan, asynchronous on the current stream: (class_slot int32 [n_ops] -- (class << 30) | slot, to be read as
        uint32 --, totals int64 [10] -- ops per class 44 / 65 / 87 / refused, message bytes per class, context bytes per class --,
        plan uint8: the working memory pack_device takes)."""
        n = self._n_ops(ops, n_ops)
        class_slot = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        totals = torch.zeros(10, dtype=torch.int64, device=self.device)
        plan = torch.empty(max(self.lib.mldsa_recsign_plan_bytes(n), 256), dtype=torch.uint8, device=self.device)
        _recsign_lib.check(self.lib.mldsa_recsign_plan(self.hp._h, int(blob_len), int(out_len), _ptr(ops), n, self._n_keys(), _ptr(class_slot),
                                                       _ptr(totals), _ptr(plan), plan.numel(), _stream(self.device)))
        return class_slot[:n], totals, plan

    def pack_device(self, blob, ops, out_len, class_slot, totals, plan, n_ops=None, arena=None):
        """mldsa_recsign_pack behind plan_device: waits for the current stream to read the totals (unless `totals` is already a
        _recsign_lib.RecsignTotals), then packs asynchronously.  Returns {pset: dict(n, key_idx [n], msgs, msg_off [n + 1], ctxs,
        ctx_off [n + 1], rnd [n, 32], sigs [n, SIG_LEN], status [n])}, every tensor a view of one arena -- what sign_device of
        MlDsa(pset) takes --, and under "raw" the mldsa_recsign_packed scatter_device takes, under "arena" the arena and under
        "rnd_region" the view of all rnd rows, which the caller zeroes after signing."""
        n = self._n_ops(ops, n_ops)
        if not isinstance(totals, _recsign_lib.RecsignTotals):
            torch.cuda.current_stream(self.device).synchronize()
            h = [int(x) for x in totals.cpu().tolist()]
            totals = _recsign_lib.RecsignTotals()
            totals.n[:], totals.msg_bytes[:], totals.ctx_bytes[:] = h[0:4], h[4:7], h[7:10]
        need = self.lib.mldsa_recsign_arena_bytes(totals.n[0], totals.n[1], totals.n[2], sum(totals.msg_bytes), sum(totals.ctx_bytes))
        if arena is None:
            arena = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        out = _recsign_lib.RecsignPacked()
        _recsign_lib.check(self.lib.mldsa_recsign_pack(self.hp._h, _ptr(blob), blob.numel(), int(out_len), _ptr(ops), n, self._n_keys(),
                                                       _ptr(class_slot), _ptr(plan), plan.numel(), C.byref(totals), _ptr(arena), arena.numel(),
                                                       C.byref(out), _stream(self.device)))
        base = arena.data_ptr()
        cut = lambda p, nbytes: arena[(p or base) - base:(p or base) - base + nbytes]  # noqa: E731
        packed = dict(raw=out, arena=arena, rnd_region=cut(out.rnd_region, out.rnd_region_bytes))
        for c, pset in enumerate(_recsign_lib.CLASS_SETS):
            k, sig_len = out.c[c], _lib.get_params(pset).sig_len
            packed[pset] = dict(
                n=int(k.n), key_idx=cut(k.key_idx, 4 * k.n).view(torch.int32), msgs=cut(k.msgs, max(int(totals.msg_bytes[c]), 1)),
                msg_off=cut(k.msg_off, 8 * (k.n + 1)).view(torch.int64), ctxs=cut(k.ctxs, max(int(totals.ctx_bytes[c]), 1)),
                ctx_off=cut(k.ctx_off, 8 * (k.n + 1)).view(torch.int64), rnd=cut(k.rnd, 32 * k.n).view(int(k.n), 32),
                sigs=cut(k.sigs, k.n * sig_len).view(int(k.n), sig_len), status=cut(k.status, 4 * k.n).view(torch.int32))
        return packed

    def scatter_device(self, ops, blob_len, out, class_slot, packed, status, n_ops=None):
        """mldsa_recsign_scatter behind the signing calls on the current stream: every accepted op's row of its class's sigs to its
        offset in `out`, status[i] = the class's status[slot] or the refusal's code.  packed: what pack_device returned."""
        n = self._n_ops(ops, n_ops)
        _recsign_lib.check(self.lib.mldsa_recsign_scatter(self.hp._h, _ptr(ops), n, int(blob_len), _ptr(out), out.numel(), self._n_keys(),
                                                          _ptr(class_slot), C.byref(packed["raw"]), _ptr(status), _stream(self.device)))
        return out

    def sign_scratch(self, n_ops, msg_bytes, ctx_bytes):
        """device scratch that no sign_device call of up to n_ops ops with these byte totals can outgrow, whatever its mix"""
        nb = self.lib.mldsa_recsign_front_bytes(n_ops) + self.lib.mldsa_recsign_arena_bytes_max(n_ops, msg_bytes, ctx_bytes)
        return torch.empty(max(nb, 256), dtype=torch.uint8, device=self.device)

    def sign_device(self, blob, ops, out, status, n_ops=None, mode=MODE_PURE, scratch=None, info=None):
        """mldsa_recsign_sign: request i signed under its own parameter set with key `key` of that set's table, the signature written
        to out[sig_off:], status[i] = mldsa_sign's status or the refusal's code.  Complete when it returns.  scratch: a uint8 tensor,
        e.g. from sign_scratch(); None: one that holds any mix whose messages and contexts fit the blob four times over (a call that
        needs more raises MldsaError with MLDSA_ERR_NOMEM, and info names the need).  info: a dict that receives n44, n65, n87,
        refused, msg_bytes, ctx_bytes and scratch_needed."""
        n = self._n_ops(ops, n_ops)
        if scratch is None:
            scratch = self.sign_scratch(n, 4 * blob.numel(), 4 * blob.numel())
        got = _recsign_lib.RecsignInfo()
        rc = self.lib.mldsa_recsign_sign(self.hp._h, mode, self._key_tables(), _ptr(blob), blob.numel(), _ptr(ops), n, _ptr(out), out.numel(),
                                         _ptr(status), _ptr(scratch), scratch.numel(), C.byref(got), _stream(self.device))
        if info is not None and rc in (_lib.OK, _lib.ERR_NOMEM) and n:
            info.update(n44=int(got.n[0]), n65=int(got.n[1]), n87=int(got.n[2]), refused=int(got.n[3]), msg_bytes=int(got.msg_bytes),
                        ctx_bytes=int(got.ctx_bytes), scratch_needed=int(got.scratch_needed))
        _recsign_lib.check(rc)
        return out

    def sign(self, requests, mode=MODE_PURE, in_place=False):
        """A host list of (pset, key, message, ctx, rnd or None) -> (signatures, status): the requests are laid out in one blob
        (sign_requests_blob; with in_place the signatures are written into the blob itself) and signed from it.  signatures: a list of
        bytes, one per request (its hole as it was laid out for a request whose status is not 0); status: an int32 array."""
        n = len(requests)
        if n == 0:
            return [], np.zeros(0, dtype=np.int32)
        blob_h, ops_h, out_len = sign_requests_blob(requests, in_place=in_place)
        blob = torch.from_numpy(blob_h.copy() if blob_h.size else np.zeros(1, np.uint8)).to(self.device)[:blob_h.size]
        out = blob if in_place else torch.zeros(max(out_len, 1), dtype=torch.uint8, device=self.device)[:out_len]
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.sign_device(blob, self.ops_tensor(ops_h), out, status, n, mode)
        torch.cuda.synchronize(self.device)
        out_h = out.cpu().numpy()
        sigs = [out_h[int(o["sig_off"]):int(o["sig_off"]) + _lib.get_params(int(o["set"])).sig_len].tobytes() for o in ops_h]
        return sigs, status.cpu().numpy()


# ---- certificate signatures from DER (include/mldsa_x509.h) --------------------------------------------------------------------------
def certificates_blob(ders, issuers, pad=0, front=0, fill=0xC3):
    """Lays DER certificates out in one buffer and describes them: (blob, certs) = (uint8 numpy array, numpy array of
    _x509_lib.CERT_DTYPE, one mldsa_x509_cert per certificate).  issuers[i]: the index of the certificate whose subject key signs
    certificate i (a self-signed root names itself), or None / _x509_lib.NO_ISSUER for a certificate that is parsed only.
    pad: the gap in front of every certificate, one int or a sequence that is cycled through, as in records_blob; front: bytes in
    front of the first gap; the gaps hold `fill`."""
    if len(ders) != len(issuers):
        raise ValueError("certificates_blob: one issuer per certificate expected")
    pads = [int(pad)] if np.isscalar(pad) else [int(x) for x in pad]
    certs = np.zeros(len(ders), dtype=_x509_lib.CERT_DTYPE)
    parts, at = [bytes([fill]) * front], front
    for i, (der, issuer) in enumerate(zip(ders, issuers)):
        if len(der) > 0xFFFFFFFF:
            raise ValueError("certificates_blob: a certificate too long for its descriptor field")
        gap = pads[i % len(pads)]
        parts += [bytes([fill]) * gap, bytes(der)]
        certs[i]["off"], certs[i]["len"] = at + gap, len(der)
        certs[i]["issuer"] = _x509_lib.NO_ISSUER if issuer is None else int(issuer)
        at += gap + len(der)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), certs


class MlDsaCertificates:
    """The signature leg of X.509 path validation on one GPU, any mix of parameter sets in one call: libmldsa_x509.so
    (include/mldsa_x509.h) in front of libmldsa_rec.so.  blob = uint8 CUDA tensor (any alignment: a slice will do), certs = uint8 CUDA
    tensor holding n mldsa_x509_cert entries (certs_tensor() uploads a numpy array of _x509_lib.CERT_DTYPE).  Validity dates, extensions
    and revocation are not looked at."""

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _x509_lib.load()
        self.records = MlDsaRecords(hotpath=self.hp)

    def certs_tensor(self, certs):
        a = np.ascontiguousarray(certs, dtype=_x509_lib.CERT_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).to(self.device)

    @staticmethod
    def _n(certs, n):
        if certs.dtype != torch.uint8 or certs.numel() % 16:
            raise ValueError("certs: a uint8 tensor of n * 16 bytes expected")
        return certs.numel() // 16 if n is None else int(n)

    def ops_device(self, blob, certs, n=None, check_names=True, status=None):
        """mldsa_x509_ops, asynchronous on the current stream: (ops uint8 [n * 40] -- one mldsa_rec_op per certificate, all zero
        where status is not 0, as MlDsaRecords takes them --, status uint8 [n], fields uint8 [n * 56] -- to be read as
        _x509_lib.FIELDS_DTYPE).  status: a uint8 tensor to write to instead of a new one."""
        n = self._n(certs, n)
        ops = torch.empty(max(n, 1) * 40, dtype=torch.uint8, device=self.device)
        fields = torch.empty(max(n, 1) * 56, dtype=torch.uint8, device=self.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        _x509_lib.check(self.lib.mldsa_x509_ops(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), n, _x509_lib.CHECK_NAMES if check_names else 0,
                                                _ptr(fields), _ptr(ops), _ptr(status), _stream(self.device)))
        return ops[:n * 40], status[:n], fields[:n * 56]

    def verify_device(self, blob, certs, ok, status=None, check_names=True, scratch=None):
        """ok[i] = 1 where certificate i's signature verifies under its issuer's subject key (pure ML-DSA, empty context) and its
        status is 0; 0 everywhere else.  ops_device, then MlDsaRecords.verify_device on the ops and the same stream (which waits for
        the stream once).  Returns the status tensor."""
        n = self._n(certs, None)
        ops, status, _ = self.ops_device(blob, certs, n, check_names, status=status)
        if n:
            self.records.verify_device(blob, ops, ok, n, MODE_PURE, scratch=scratch)
        return status

    def verify(self, ders, issuers, check_names=True, pad=0):
        """Host lists of DER certificates and their issuers' indices -> (bool array, status array): the certificates are laid out
        in one blob (certificates_blob) and verified from it."""
        n = len(ders)
        if n == 0:
            return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint8)
        blob_h, certs_h = certificates_blob(ders, issuers, pad=pad)
        blob = torch.from_numpy(blob_h.copy() if blob_h.size else np.zeros(1, np.uint8)).to(self.device)[:blob_h.size]
        ok = torch.zeros(n, dtype=torch.uint8, device=self.device)
        status = self.verify_device(blob, self.certs_tensor(certs_h), ok, check_names=check_names)
        torch.cuda.synchronize(self.device)
        return ok.cpu().numpy().astype(bool), status.cpu().numpy()


# ---- certificates issued from TBSCertificates (include/mldsa_x509sign.h) -----------------------------------------------------------------
def tbs_blob(requests, pad=0, front=0, fill=0xC3):
    """Lays issuing requests (pset, key_row, tbs_der, rnd or None, issuer) out in one buffer -- each TBSCertificate and, where there is
    one, its 32 bytes of rnd behind it -- and describes them: (blob, reqs) = (uint8 numpy array, numpy array of
    _x509sign_lib.REQ_DTYPE, one mldsa_x509sign_req per request).  key_row: the row of the parameter set's key table; rnd None: the
    deterministic variant (no MLDSA_X509SIGN_RND flag); issuer: copied through to the finished certificate's entry (None:
    _x509_lib.NO_ISSUER).  pad: the gap in front of every TBS and every rnd, one int or a sequence that is cycled through, as in
    certificates_blob; front: bytes in front of the first gap; the gaps hold `fill`."""
    pads = [int(pad)] if np.isscalar(pad) else [int(x) for x in pad]
    reqs = np.zeros(len(requests), dtype=_x509sign_lib.REQ_DTYPE)
    parts, at, k = [bytes([fill]) * front], front, 0
    for i, (pset, key, tbs, rnd, issuer) in enumerate(requests):
        if len(tbs) > 0xFFFFFFFF or (rnd is not None and len(rnd) != 32) or not 0 <= int(pset) <= 255:
            raise ValueError("tbs_blob: a TBSCertificate too long for its entry, rnd not 32 bytes, or a set that is no byte")
        reqs[i]["set"], reqs[i]["key"], reqs[i]["len"] = pset, key, len(tbs)
        reqs[i]["issuer"] = _x509_lib.NO_ISSUER if issuer is None else int(issuer)
        reqs[i]["flags"] = 0 if rnd is None else _x509sign_lib.FLAG_RND
        for name, field in [("off", tbs)] + ([("rnd_off", rnd)] if rnd is not None else []):
            gap = pads[k % len(pads)]
            k += 1
            parts += [bytes([fill]) * gap, bytes(field)]
            reqs[i][name] = at + gap
            at += gap + len(field)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), reqs


class MlDsaCertificateIssuer:
    """X.509 certificates issued on one GPU from DER TBSCertificates, any mix of parameter sets in one call: libmldsa_x509sign.so
    (include/mldsa_x509sign.h) in front of libmldsa_recsign.so.  blob, out = uint8 CUDA tensors (any alignment: a slice will do; they
    must not overlap), reqs = uint8 CUDA tensor holding n mldsa_x509sign_req entries (requests_tensor() uploads a numpy array of
    _x509sign_lib.REQ_DTYPE).  The key tables are set_keys()'s PrivateKeys, used where they lie.  Validity dates, extensions and name
    chaining are not looked at."""

    tbs_blob = staticmethod(tbs_blob)

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _x509sign_lib.load()
        self.signer = MlDsaRecordSigner(hotpath=self.hp)

    def set_keys(self, pset, sks):
        """the issuers' key table of one parameter set: a PrivateKeys (kept by reference, never copied); None: the set is not served"""
        self.signer.set_keys(pset, sks)

    def requests_tensor(self, reqs):
        a = np.ascontiguousarray(reqs, dtype=_x509sign_lib.REQ_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(32, np.uint8)).to(self.device)

    @staticmethod
    def _n(reqs, n):
        if reqs.dtype != torch.uint8 or reqs.numel() % 32:
            raise ValueError("reqs: a uint8 tensor of n * 32 bytes expected")
        return reqs.numel() // 32 if n is None else int(n)

    def plan_memory(self, n):
        return torch.empty(max(self.lib.mldsa_x509sign_plan_bytes(n), 256), dtype=torch.uint8, device=self.device)

    def issue_ops_device(self, blob, reqs, out, n=None, plan=None):
        """mldsa_x509sign_issue_ops, asynchronous on the current stream: every accepted certificate's frame -- all but its signature
        -- is written to `out`.  Returns (out_certs uint8 [n * 16] -- one mldsa_x509_cert per request, as MlDsaCertificates takes them
        with `out` as the blob --, ops uint8 [n * 48] -- one mldsa_recsign_op per request, all zero where status is not 0, as
        MlDsaRecordSigner takes them --, status uint8 [n], totals int64 [3] -- accepted, refused, out_bytes).  plan: the working memory,
        a uint8 tensor from plan_memory()."""
        n = self._n(reqs, n)
        out_certs = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=self.device)
        ops = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device=self.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        totals = torch.zeros(3, dtype=torch.int64, device=self.device)
        if plan is None:
            plan = self.plan_memory(n)
        _x509sign_lib.check(self.lib.mldsa_x509sign_issue_ops(self.hp._h, _ptr(blob), blob.numel(), _ptr(reqs), n, self.signer._n_keys(),
                                                              _ptr(out), out.numel(), _ptr(out_certs), _ptr(ops), _ptr(status), _ptr(totals),
                                                              _ptr(plan), plan.numel(), _stream(self.device)))
        return out_certs[:n * 16], ops[:n * 48], status[:n], totals

    def issue_device(self, blob, reqs, out, sig_status, n=None, plan=None, scratch=None):
        """The two calls: issue_ops_device, then MlDsaRecordSigner.sign_device (pure ML-DSA, empty context) on the ops and the same
        stream, which writes every accepted certificate's signature into its hole and sig_status[i] (int32 [n]).  Certificate i is
        issued where status[i] == 0 and sig_status[i] == 0.  Complete when it returns.  Returns (out_certs, status, totals)."""
        n = self._n(reqs, n)
        out_certs, ops, status, totals = self.issue_ops_device(blob, reqs, out, n, plan=plan)
        if n:
            self.signer.sign_device(blob, ops, out, sig_status, n, MODE_PURE, scratch=scratch)
        return out_certs, status, totals

    def issue(self, requests, pad=0):
        """A host list of (pset, key_row, tbs_der, rnd or None, issuer) -> (certificates, status, sig_status): the requests are laid
        out in one blob (tbs_blob) and issued from it.  certificates: a list of DER bytes, None for a request that was refused or
        whose signing gave up; status: a uint8 array; sig_status: an int32 array."""
        n = len(requests)
        if n == 0:
            return [], np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32)
        blob_h, reqs_h = tbs_blob(requests, pad=pad)
        out_len = self.lib.mldsa_x509sign_out_bytes_max(n, int(sum(len(r[2]) for r in requests)))
        blob = torch.from_numpy(blob_h.copy() if blob_h.size else np.zeros(1, np.uint8)).to(self.device)[:blob_h.size]
        out = torch.zeros(max(out_len, 1), dtype=torch.uint8, device=self.device)
        sig_status = torch.zeros(n, dtype=torch.int32, device=self.device)
        out_certs, status, _ = self.issue_device(blob, self.requests_tensor(reqs_h), out, sig_status, n)
        torch.cuda.synchronize(self.device)
        out_h, st, sst = out.cpu().numpy(), status.cpu().numpy(), sig_status.cpu().numpy()
        rows = out_certs.cpu().numpy().view(_x509_lib.CERT_DTYPE)
        certs = [out_h[int(c["off"]):int(c["off"]) + int(c["len"])].tobytes() if st[i] == 0 and sst[i] == 0 else None for i, c in enumerate(rows)]
        return certs, st, sst


# ---- certification requests: proof of possession and TBSCertificates (include/mldsa_csr.h) ------------------------------------------------
def csr_blob(ders, templates=None, pad=0, front=0, fill=0xC3):
    """Lays DER certification requests out in one buffer and describes them: (blob, items) = (uint8 numpy array, numpy array of
    _csr_lib.ITEM_DTYPE, one mldsa_csr_item per request).  With templates -- one (pset, key_row, serial, issuer_name, validity,
    extensions or b"", rnd or None, issuer) per request: the set and the row of the CA key that will sign, the serial number's content
    bytes, the DER issuer Name, Validity and [3] extensions, and the index copied through to the finished certificate's entry (None:
    _x509_lib.NO_ISSUER) -- the template pieces are laid out behind the requests, equal pieces once, and (blob, items, entries) is
    returned with entries a numpy array of _csr_lib.ISSUE_DTYPE.  rnd is not laid out here: it belongs to the buffer the
    TBSCertificates go to, so entries[i]["rnd_off"] is left 0 and only the flag is set.
    pad: the gap in front of every request and every piece, one int or a sequence that is cycled through, as in certificates_blob;
    front: bytes in front of the first gap; the gaps hold `fill`."""
    pads = [int(pad)] if np.isscalar(pad) else [int(x) for x in pad]
    items = np.zeros(len(ders), dtype=_csr_lib.ITEM_DTYPE)
    parts, at, k = [bytes([fill]) * front], front, 0

    def lay(field):
        nonlocal at, k
        gap = pads[k % len(pads)]
        k += 1
        parts.extend([bytes([fill]) * gap, bytes(field)])
        at += gap + len(field)
        return at - len(field)

    for i, der in enumerate(ders):
        if len(der) > 0xFFFFFFFF:
            raise ValueError("csr_blob: a request too long for its descriptor field")
        items[i]["off"], items[i]["len"] = lay(der), len(der)
    if templates is None:
        return np.frombuffer(b"".join(parts), dtype=np.uint8), items
    if len(templates) != len(ders):
        raise ValueError("csr_blob: one template per request expected")
    entries = np.zeros(len(ders), dtype=_csr_lib.ISSUE_DTYPE)
    placed = {}
    for i, (pset, key, serial, issuer_name, validity, ext, rnd, issuer) in enumerate(templates):
        if not 0 <= int(pset) <= 255 or len(serial) > 255 or (rnd is not None and len(rnd) != 32):
            raise ValueError("csr_blob: a set or a serial length that is no byte, or rnd not 32 bytes")
        e = entries[i]
        e["set"], e["key"], e["serial_len"], e["flags"] = pset, key, len(serial), 0 if rnd is None else _csr_lib.FLAG_RND
        e["issuer"] = _x509_lib.NO_ISSUER if issuer is None else int(issuer)
        for name, piece in (("serial", serial), ("issuer", issuer_name), ("validity", validity), ("ext", ext)):
            piece = bytes(piece)
            if piece and piece not in placed:
                placed[piece] = lay(piece)
            e[name + "_off"] = placed.get(piece, 0)
            if name != "serial":
                e[name + "_len"] = len(piece)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), items, entries


class MlDsaCertificateRequests:
    """PKCS#10 certification requests on one GPU, any mix of parameter sets in one call: libmldsa_csr.so (include/mldsa_csr.h) in front
    of libmldsa_rec.so (the proof of possession) and of libmldsa_x509sign.so and libmldsa_recsign.so (the certificate).  blob, tbs, out =
    uint8 CUDA tensors (any alignment: a slice will do; no two may overlap), items / entries = uint8 CUDA tensors holding n
    mldsa_csr_item / mldsa_csr_issue rows (items_tensor() and issue_tensor() upload numpy arrays of _csr_lib.ITEM_DTYPE and
    _csr_lib.ISSUE_DTYPE).  The CA's key tables are set_keys()'s PrivateKeys.  Attributes, name policy and validity dates are not
    looked at."""

    csr_blob = staticmethod(csr_blob)

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _csr_lib.load()
        self.records = MlDsaRecords(hotpath=self.hp)
        self.issuer = MlDsaCertificateIssuer(hotpath=self.hp)

    def set_keys(self, pset, sks):
        """the CA's key table of one parameter set: a PrivateKeys (kept by reference, never copied); None: the set is not served"""
        self.issuer.set_keys(pset, sks)

    def _rows(self, rows, dtype):
        a = np.ascontiguousarray(rows, dtype=dtype)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(dtype.itemsize, np.uint8)).to(self.device)

    def items_tensor(self, items):
        return self._rows(items, _csr_lib.ITEM_DTYPE)

    def issue_tensor(self, entries):
        return self._rows(entries, _csr_lib.ISSUE_DTYPE)

    @staticmethod
    def _n(rows, n, size, what):
        if rows.dtype != torch.uint8 or rows.numel() % size:
            raise ValueError("%s: a uint8 tensor of n * %d bytes expected" % (what, size))
        return rows.numel() // size if n is None else int(n)

    def plan_memory(self, n):
        return torch.empty(max(self.lib.mldsa_csr_plan_bytes(n), 256), dtype=torch.uint8, device=self.device)

    def parse_device(self, blob, items, n=None, status=None):
        """mldsa_csr_parse, asynchronous on the current stream: (fields uint8 [n * 56] -- to be read as _csr_lib.FIELDS_DTYPE --, ops
        uint8 [n * 40] -- one mldsa_rec_op per request, all zero where status is not 0, as MlDsaRecords takes them --, status uint8
        [n]).  status: a uint8 tensor to write to instead of a new one."""
        n = self._n(items, n, 16, "items")
        fields = torch.empty(max(n, 1) * 56, dtype=torch.uint8, device=self.device)
        ops = torch.empty(max(n, 1) * 40, dtype=torch.uint8, device=self.device)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        _csr_lib.check(self.lib.mldsa_csr_parse(self.hp._h, _ptr(blob), blob.numel(), _ptr(items), n, _ptr(fields), _ptr(ops), _ptr(status),
                                                _stream(self.device)))
        return fields[:n * 56], ops[:n * 40], status[:n]

    def verify_device(self, blob, items, ok, n=None, scratch=None):
        """ok[i] = 1 where request i is well formed and signed by the key it carries (pure ML-DSA, empty context); 0 everywhere else.
        parse_device, then MlDsaRecords.verify_device on the ops and the same stream (which waits for the stream once).  Returns
        (fields, status)."""
        n = self._n(items, n, 16, "items")
        fields, ops, status = self.parse_device(blob, items, n)
        if n:
            self.records.verify_device(blob, ops, ok, n, MODE_PURE, scratch=scratch)
        return fields, status

    def tbs_device(self, blob, fields, entries, ok, out, n=None, plan=None):
        """mldsa_csr_tbs, asynchronous on the current stream: the TBSCertificate of every request that is accepted and possessed is
        written to `out`.  Returns (reqs uint8 [n * 32] -- one mldsa_x509sign_req per request, all zero where status is not 0, as
        MlDsaCertificateIssuer takes them with `out` as the blob --, status uint8 [n], totals int64 [3] -- accepted, refused,
        out_bytes).  plan: the working memory, a uint8 tensor from plan_memory()."""
        n = self._n(entries, n, 64, "entries")
        reqs = torch.empty(max(n, 1) * 32, dtype=torch.uint8, device=self.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        totals = torch.zeros(3, dtype=torch.int64, device=self.device)
        if plan is None:
            plan = self.plan_memory(n)
        _csr_lib.check(self.lib.mldsa_csr_tbs(self.hp._h, _ptr(blob), blob.numel(), _ptr(fields), _ptr(entries), _ptr(ok), n, _ptr(out),
                                              out.numel(), _ptr(reqs), _ptr(status), _ptr(totals), _ptr(plan), plan.numel(),
                                              _stream(self.device)))
        return reqs[:n * 32], status[:n], totals

    def issue_device(self, blob, items, entries, tbs, out, sig_status, n=None, tbs_len=None, scratch=None):
        """The five calls: parse_device, MlDsaRecords.verify_device, tbs_device into tbs[:tbs_len], then
        MlDsaCertificateIssuer.issue_device with the whole of `tbs` as its blob -- a caller that signs hedged keeps the randomness in
        tbs[tbs_len:] and points the entries' rnd_off there.  Request i is a certificate where status[i] == 0, issue_status[i] == 0 and
        sig_status[i] == 0 (int32 [n]).  Complete when it returns.  Returns (out_certs -- one mldsa_x509_cert per request, as
        MlDsaCertificates takes them with `out` as the blob --, status, issue_status, totals -- mldsa_csr_tbs's)."""
        n = self._n(items, n, 16, "items")
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        fields, _ = self.verify_device(blob, items, ok, n, scratch=scratch)
        reqs, status, totals = self.tbs_device(blob, fields, entries, ok, tbs if tbs_len is None else tbs[:tbs_len], n)
        out_certs, issue_status, _ = self.issuer.issue_device(tbs, reqs, out, sig_status, n)
        return out_certs, status, issue_status, totals

    def verify(self, ders, pad=0):
        """A host list of DER certification requests -> (bool array, status array): the requests are laid out in one blob (csr_blob)
        and their proofs of possession verified from it."""
        n = len(ders)
        if n == 0:
            return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint8)
        blob_h, items_h = csr_blob(ders, pad=pad)
        blob = torch.from_numpy(blob_h.copy()).to(self.device)
        ok = torch.zeros(n, dtype=torch.uint8, device=self.device)
        _, status = self.verify_device(blob, self.items_tensor(items_h), ok, n)
        torch.cuda.synchronize(self.device)
        return ok.cpu().numpy().astype(bool), status.cpu().numpy()

    def issue(self, ders, templates, pad=0):
        """Host lists of DER certification requests and their templates (csr_blob) -> (certificates, status, sig_status).
        certificates: a list of DER bytes, None for a request that was refused at any stage or whose signing gave up; status: a uint8
        array, the first nonzero of mldsa_csr_tbs's and mldsa_x509sign_issue_ops's; sig_status: an int32 array."""
        n = len(ders)
        if n == 0:
            return [], np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32)
        blob_h, items_h, entries_h = csr_blob(ders, templates, pad=pad)
        tbs_len = int(sum(len(d) + 64 + len(t[3]) + len(t[4]) + len(t[5]) for d, t in zip(ders, templates)))
        rnd = np.zeros((n, 32), dtype=np.uint8)
        for i, t in enumerate(templates):
            if t[6] is not None:
                rnd[i] = np.frombuffer(bytes(t[6]), dtype=np.uint8)
                entries_h[i]["rnd_off"] = tbs_len + 32 * i
        blob = torch.from_numpy(blob_h.copy()).to(self.device)
        tbs = torch.zeros(tbs_len + 32 * n, dtype=torch.uint8, device=self.device)
        tbs[tbs_len:] = torch.from_numpy(rnd.reshape(-1)).to(self.device)
        out = torch.zeros(self.issuer.lib.mldsa_x509sign_out_bytes_max(n, tbs_len), dtype=torch.uint8, device=self.device)
        sig_status = torch.zeros(n, dtype=torch.int32, device=self.device)
        out_certs, status, issue_status, _ = self.issue_device(blob, self.items_tensor(items_h), self.issue_tensor(entries_h), tbs, out,
                                                               sig_status, n, tbs_len=tbs_len)
        torch.cuda.synchronize(self.device)
        tbs[tbs_len:].zero_()  # the randomness of the hedged variant
        out_h, st, ist, sst = out.cpu().numpy(), status.cpu().numpy(), issue_status.cpu().numpy(), sig_status.cpu().numpy()
        st = np.where(st != 0, st, ist).astype(np.uint8)
        rows = out_certs.cpu().numpy().view(_x509_lib.CERT_DTYPE)
        certs = [out_h[int(c["off"]):int(c["off"]) + int(c["len"])].tobytes() if st[i] == 0 and sst[i] == 0 else None for i, c in enumerate(rows)]
        return certs, st, sst


# ---- certificate revocation lists (include/mldsa_crl.h) ------------------------------------------------------------------------------
def _crl_items(rows):
    """mldsa_x509_cert rows (offset, length, issuer) as mldsa_crl_item rows: the same three fields"""
    items = np.zeros(len(rows), dtype=_crl_lib.ITEM_DTYPE)
    for f in ("off", "len", "issuer"):
        items[f] = rows[f]
    return items


def crl_blob(crls, issuers, pad=0, front=0, fill=0xC3):
    """Lays DER CertificateLists out in one buffer and describes them: (blob, items) = (uint8 numpy array, numpy array of
    _crl_lib.ITEM_DTYPE, one mldsa_crl_item per CRL).  issuers[i]: the row, among the certificates' mldsa_x509_fields, of the CA
    certificate whose subject key signs CRL i.  pad, front, fill: as in certificates_blob.  The certificates that a lookup reads lie
    in the same buffer: a caller who needs both lays the CRLs out behind them (front = the bytes in front)."""
    if len(crls) != len(issuers):
        raise ValueError("crl_blob: one issuer per CRL expected")
    blob, rows = certificates_blob(crls, issuers, pad=pad, front=front, fill=fill)
    return blob, _crl_items(rows)


class MlDsaRevocationLists:
    """The revocation leg of X.509 path validation on one GPU, any mix of parameter sets in one call: libmldsa_crl.so
    (include/mldsa_crl.h) in front of and behind libmldsa_rec.so, beside libmldsa_x509.so.  blob = uint8 CUDA tensor that holds the
    CRLs and the certificates (any alignment: a slice will do), items = uint8 CUDA tensor holding n mldsa_crl_item rows
    (items_tensor() uploads a numpy array of _crl_lib.ITEM_DTYPE).  Update times, delta and indirect CRLs, distribution points and
    critical extensions are not looked at."""

    crl_blob = staticmethod(crl_blob)

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _crl_lib.load()
        self.certificates = MlDsaCertificates(hotpath=self.hp)
        self.records = self.certificates.records

    def items_tensor(self, items):
        a = np.ascontiguousarray(items, dtype=_crl_lib.ITEM_DTYPE)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).to(self.device)

    @staticmethod
    def _n(rows, n, size, what):
        if rows.dtype != torch.uint8 or rows.numel() % size:
            raise ValueError("%s: a uint8 tensor of n * %d bytes expected" % (what, size))
        return rows.numel() // size if n is None else int(n)

    def ops_device(self, blob, items, cert_fields, n=None, max_entries=None, check_names=True):
        """mldsa_crl_ops, asynchronous on the current stream: (ops uint8 [n * 40] -- one mldsa_rec_op per CRL, all zero where status
        is not 0, as MlDsaRecords takes them --, status uint8 [n], crl_fields uint8 [n * 88] -- to be read as _crl_lib.FIELDS_DTYPE
        --, entries uint8 [max_entries * 32] -- _crl_lib.ENTRY_DTYPE --, totals int64 [5] -- _crl_lib.TOTALS_DTYPE).  cert_fields:
        the rows MlDsaCertificates.ops_device returned.  max_entries None: blob.numel() // 20 slots, which CRLs that do not overlap
        cannot outgrow."""
        n = self._n(items, n, 16, "items")
        n_certs = self._n(cert_fields, None, 56, "cert_fields")
        if max_entries is None:
            max_entries = blob.numel() // 20
        entries = torch.empty(max(max_entries, 1) * 32, dtype=torch.uint8, device=self.device)
        ops = torch.empty(max(n, 1) * 40, dtype=torch.uint8, device=self.device)
        fields = torch.empty(max(n, 1) * 88, dtype=torch.uint8, device=self.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        totals = torch.zeros(5, dtype=torch.int64, device=self.device)
        scratch = torch.empty(max(self.lib.mldsa_crl_scratch_bytes(n), 256), dtype=torch.uint8, device=self.device)
        _crl_lib.check(self.lib.mldsa_crl_ops(self.hp._h, _ptr(blob), blob.numel(), _ptr(items), n, _ptr(cert_fields), n_certs,
                                              _crl_lib.CHECK_NAMES if check_names else 0, _ptr(fields), _ptr(entries), max_entries, _ptr(ops),
                                              _ptr(status), _ptr(totals), _ptr(scratch), scratch.numel(), _stream(self.device)))
        return ops[:n * 40], status[:n], fields[:n * 88], entries[:max_entries * 32], totals

    def table_device(self, entries, totals=None):
        """mldsa_crl_table, asynchronous on the current stream: (table int32 [mldsa_crl_table_slots], totals) -- the lookup table over
        the entry rows, built once per CRL refresh and taken by every check_device.  totals: mldsa_crl_ops' row, whose overflow field
        the call writes; None: a new one."""
        max_entries = self._n(entries, None, 32, "entries")
        slots = self.lib.mldsa_crl_table_slots(max_entries)
        table = torch.empty(slots, dtype=torch.int32, device=self.device)
        if totals is None:
            totals = torch.zeros(5, dtype=torch.int64, device=self.device)
        _crl_lib.check(self.lib.mldsa_crl_table(self.hp._h, _ptr(entries), max_entries, _ptr(table), slots, _ptr(totals), _stream(self.device)))
        return table, totals

    def check_device(self, blob, certs, cert_fields, cert_crl, items, crl_fields, crl_status, crl_ok, entries, table, revocation=None):
        """mldsa_crl_check, asynchronous on the current stream: revocation uint8 [n_certs], one of _crl_lib.GOOD ... SCOPE per
        certificate.  certs, cert_fields: MlDsaCertificates' rows; cert_crl: an int32 CUDA tensor, the CRL that covers each certificate
        or -1 (MLDSA_CRL_NONE); crl_ok: MlDsaRecords' verdicts on the CRLs' ops, or None."""
        n_certs = self._n(certs, None, 16, "certs")
        n_crls = self._n(items, None, 16, "items")
        if cert_crl.dtype != torch.int32 or cert_crl.numel() < n_certs:
            raise ValueError("cert_crl: an int32 tensor of n_certs elements expected")
        if revocation is None:
            revocation = torch.empty(max(n_certs, 1), dtype=torch.uint8, device=self.device)
        _crl_lib.check(self.lib.mldsa_crl_check(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), _ptr(cert_fields), _ptr(cert_crl), n_certs,
                                                _ptr(items), _ptr(crl_fields), _ptr(crl_status), None if crl_ok is None else _ptr(crl_ok), n_crls,
                                                _ptr(entries), entries.numel() // 32, _ptr(table), table.numel(), _ptr(revocation),
                                                _stream(self.device)))
        return revocation[:n_certs]

    def check(self, cert_ders, cert_issuers, crl_ders, crl_issuers, cert_crl, pad=0, check_names=True):
        """Host lists of DER certificates with their issuers' indices, DER CRLs with the index of the CA certificate that signs each,
        and for every certificate the index of the CRL that covers it (None: none) -> (revocation, cert_ok, cert_status, crl_ok,
        crl_status): everything is laid out in one blob, the certificates' and the CRLs' signatures are verified from it
        (mldsa_x509_ops, mldsa_crl_ops, mldsa_rec_verify on each), the table is built and every certificate looked up."""
        n_certs, n_crls = len(cert_ders), len(crl_ders)
        if len(cert_crl) != n_certs:
            raise ValueError("check: one CRL index (or None) per certificate expected")
        if n_certs == 0:
            return (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=bool),
                    np.zeros(0, dtype=np.uint8))
        blob_h, rows = certificates_blob(list(cert_ders) + list(crl_ders), list(cert_issuers) + list(crl_issuers), pad=pad)
        blob = torch.from_numpy(blob_h.copy()).to(self.device)
        certs, items = self.certificates.certs_tensor(rows[:n_certs]), self.items_tensor(_crl_items(rows[n_certs:]))[:n_crls * 16]
        covered = np.array([_crl_lib.NONE if c is None else int(c) for c in cert_crl], dtype=np.uint32).view(np.int32)
        cert_ok = torch.zeros(n_certs, dtype=torch.uint8, device=self.device)
        crl_ok = torch.zeros(max(n_crls, 1), dtype=torch.uint8, device=self.device)
        cert_ops, cert_status, cert_fields = self.certificates.ops_device(blob, certs, n_certs, check_names)
        self.records.verify_device(blob, cert_ops, cert_ok, n_certs, MODE_PURE)
        max_entries = int(sum(self.lib.mldsa_crl_entries_bound(len(d)) for d in crl_ders))
        crl_ops, crl_status, crl_fields, entries, totals = self.ops_device(blob, items, cert_fields, n_crls, max_entries, check_names)
        if n_crls:
            self.records.verify_device(blob, crl_ops, crl_ok, n_crls, MODE_PURE)
        table, totals = self.table_device(entries, totals)
        revocation = self.check_device(blob, certs, cert_fields, torch.from_numpy(covered.copy()).to(self.device), items, crl_fields, crl_status,
                                       crl_ok, entries, table)
        torch.cuda.synchronize(self.device)
        if int(totals.cpu().numpy().view(_crl_lib.TOTALS_DTYPE)[0]["overflow"]):
            raise RuntimeError("mldsa_crl_table: the lookup table overflowed")
        return (revocation.cpu().numpy(), cert_ok.cpu().numpy().astype(bool), cert_status.cpu().numpy(), crl_ok[:n_crls].cpu().numpy().astype(bool),
                crl_status.cpu().numpy())


# ---- path validation: validity, CA constraints, chain verdicts (include/mldsa_path.h) ---------------------------------------------------
class MlDsaPathValidator:
    """The last leg of X.509 path validation on one GPU: libmldsa_path.so (include/mldsa_path.h) behind libmldsa_x509.so, libmldsa_crl.so
    and libmldsa_rec.so.  blob = uint8 CUDA tensor that holds the certificates and the CRLs (any alignment), certs = uint8 CUDA tensor
    of mldsa_x509_cert rows (MlDsaCertificates.certs_tensor).  `now` and every time are seconds since 1970-01-01T00:00:00Z.  Name and
    policy constraints, extended key usage, AKI / SKI, cRLSign, delta and indirect CRLs are not looked at."""

    def __init__(self, device=0, hotpath=None):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _path_lib.load()
        self.lists = MlDsaRevocationLists(hotpath=self.hp)
        self.certificates = self.lists.certificates
        self.records = self.lists.records
        self.builder = None  # an MlDsaPathBuilder, made by the first validate that has to find issuers

    _n = staticmethod(MlDsaRevocationLists._n)

    def parse_device(self, blob, certs, n=None, allow_unknown_critical=False):
        """mldsa_path_parse, asynchronous on the current stream: policy uint8 [n * 48], to be read as _path_lib.FIELDS_DTYPE."""
        n = self._n(certs, n, 16, "certs")
        fields = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device=self.device)
        _path_lib.check(self.lib.mldsa_path_parse(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), n,
                                                  _path_lib.ALLOW_UNKNOWN_CRITICAL if allow_unknown_critical else 0, _ptr(fields),
                                                  _stream(self.device)))
        return fields[:n * 48]

    def times_device(self, blob, offs):
        """mldsa_path_times, asynchronous on the current stream: (seconds int64 [n], status uint8 [n]) of the Time TLVs at the blob
        offsets offs (an int64 CUDA tensor)."""
        if offs.dtype != torch.int64:
            raise ValueError("offs: an int64 tensor expected")
        n = offs.numel()
        seconds = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        _path_lib.check(self.lib.mldsa_path_times(self.hp._h, _ptr(blob), blob.numel(), _ptr(offs), n, _ptr(seconds), _ptr(status),
                                                  _stream(self.device)))
        return seconds[:n], status[:n]

    def crl_times_device(self, blob, crl_fields, crl_status, crl_ok, now, require_next_update=False):
        """mldsa_path_crl_times, asynchronous on the current stream: (this_s int64 [n], next_s int64 [n], time_status uint8 [n],
        fresh_ok uint8 [n]).  crl_fields, crl_status: MlDsaRevocationLists.ops_device's; crl_ok: the verdicts on its ops, or None.
        fresh_ok goes into MlDsaRevocationLists.check_device in the place of crl_ok."""
        n = self._n(crl_fields, None, 88, "crl_fields")
        this_s = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        next_s = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        time_status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        fresh_ok = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        _path_lib.check(self.lib.mldsa_path_crl_times(self.hp._h, _ptr(blob), blob.numel(), _ptr(crl_fields), _ptr(crl_status),
                                                      None if crl_ok is None else _ptr(crl_ok), n, int(now),
                                                      _path_lib.REQUIRE_NEXT_UPDATE if require_next_update else 0, _ptr(this_s), _ptr(next_s),
                                                      _ptr(time_status), _ptr(fresh_ok), _stream(self.device)))
        return this_s[:n], next_s[:n], time_status[:n], fresh_ok[:n]

    def chain_device(self, certs, policy, cert_status, cert_ok, revocation, anchor, now, allow_no_crl=False, scratch=None):
        """mldsa_path_chain, asynchronous on the current stream: results uint8 [n * 8], to be read as _path_lib.RESULT_DTYPE.
        revocation: MlDsaRevocationLists.check_device's answers, or None; anchor: uint8 [n], nonzero for a trust anchor."""
        n = self._n(certs, None, 16, "certs")
        results = torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=self.device)
        if scratch is None:
            scratch = torch.empty(max(self.lib.mldsa_path_scratch_bytes(n), 256), dtype=torch.uint8, device=self.device)
        _path_lib.check(self.lib.mldsa_path_chain(self.hp._h, _ptr(certs), _ptr(policy), _ptr(cert_status), _ptr(cert_ok),
                                                  None if revocation is None else _ptr(revocation), _ptr(anchor), n, int(now),
                                                  _path_lib.ALLOW_NO_CRL if allow_no_crl else 0, _ptr(results), _ptr(scratch), scratch.numel(),
                                                  _stream(self.device)))
        return results[:n * 8]

    def validate(self, cert_ders, cert_issuers, anchors, now, crl_ders=(), crl_issuers=(), cert_crl=None, pad=0, allow_no_crl=False):
        """Host lists of DER certificates with their issuers' indices, the indices of the trust anchors, the time, and optionally DER
        CRLs with the index of the CA certificate that signs each and for every certificate the index of the CRL that covers it (None:
        none) -> (verdict, where, depth, details).  On one stream: mldsa_x509_ops, mldsa_rec_verify, mldsa_path_parse, and with CRLs
        mldsa_crl_ops, mldsa_rec_verify, mldsa_crl_table, mldsa_path_crl_times and mldsa_crl_check on fresh_ok, then mldsa_path_chain.
        Without CRLs revocation is not checked; with them a certificate that no CRL covers is refused (REVOCATION) unless
        allow_no_crl.  details: the intermediate arrays by name.
        cert_issuers None: the issuers are found on the device (MlDsaPathBuilder, include/mldsa_find.h) in front of mldsa_x509_ops;
        crl_issuers None: the CRLs' issuers too; and where either is None and cert_crl is None, so is the CRL of every certificate.
        What was found is in details (issuers, candidates, find_status, crl_issuers, cert_crl).  With the arrays given nothing of this
        runs."""
        n, n_crls = len(cert_ders), len(crl_ders)
        find_certs, find_crls = cert_issuers is None, crl_issuers is None
        if find_certs:
            cert_issuers = [None] * n
        if find_crls:
            crl_issuers = [0] * n_crls
        if len(cert_issuers) != n or (cert_crl is not None and len(cert_crl) != n) or len(crl_issuers) != n_crls:
            raise ValueError("validate: one issuer per certificate and per CRL, one CRL index (or None) per certificate expected")
        if n == 0:
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), {}
        blob_h, rows = certificates_blob(list(cert_ders) + list(crl_ders), list(cert_issuers) + list(crl_issuers), pad=pad)
        blob = torch.from_numpy(blob_h.copy()).to(self.device)
        certs = self.certificates.certs_tensor(rows[:n])
        found = None
        if find_certs or find_crls:
            if self.builder is None:
                self.builder = MlDsaPathBuilder(hotpath=self.hp)
            found = self.builder.build_device(blob, certs)
            if find_certs:
                certs = found["certs_out"]
        anchor_h = np.zeros(n, dtype=np.uint8)
        anchor_h[list(anchors)] = 1
        anchor = torch.from_numpy(anchor_h).to(self.device)
        cert_ok = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if found is None:
            cert_ops, cert_status, cert_fields = self.certificates.ops_device(blob, certs, n)
            policy = self.parse_device(blob, certs, n)
        else:  # both walks were made for the builder, and neither reads an issuer: only the link is left
            cert_fields, policy = found["fields"], found["policy"]
            cert_ops = torch.empty(n * 40, dtype=torch.uint8, device=self.device)
            cert_status = torch.empty(n, dtype=torch.uint8, device=self.device)
            _x509_lib.check(self.certificates.lib.mldsa_x509_link(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), _ptr(cert_fields), n,
                                                                  _x509_lib.CHECK_NAMES, _ptr(cert_ops), _ptr(cert_status), _stream(self.device)))
        self.records.verify_device(blob, cert_ops, cert_ok, n, MODE_PURE)
        details = {}
        revocation = None
        if n_crls:
            items = self.lists.items_tensor(_crl_items(rows[n:]))
            if find_crls:
                items, found["crl_results"] = self.builder.crl_issuers_device(blob, items, self.builder.crl_parse_device(blob, items), found)
            covered = np.array([_crl_lib.NONE if c is None else int(c) for c in (cert_crl or [None] * n)], dtype=np.uint32).view(np.int32)
            covered_d = torch.from_numpy(covered.copy()).to(self.device)
            if found is not None and cert_crl is None:
                covered_d = found["cert_crl"] = self.builder.cert_crls_device(certs, items, found["scratch"])
            crl_ok = torch.zeros(n_crls, dtype=torch.uint8, device=self.device)
            max_entries = int(sum(self.lists.lib.mldsa_crl_entries_bound(len(d)) for d in crl_ders))
            crl_ops, crl_status, crl_fields, entries, totals = self.lists.ops_device(blob, items, cert_fields, n_crls, max_entries)
            self.records.verify_device(blob, crl_ops, crl_ok, n_crls, MODE_PURE)
            table, totals = self.lists.table_device(entries, totals)
            this_s, next_s, time_status, fresh_ok = self.crl_times_device(blob, crl_fields, crl_status, crl_ok, now)
            revocation = self.lists.check_device(blob, certs, cert_fields, covered_d, items, crl_fields, crl_status, fresh_ok, entries, table)
            details.update(crl_ok=crl_ok, crl_status=crl_status, time_status=time_status, fresh_ok=fresh_ok, this_s=this_s, next_s=next_s,
                           revocation=revocation)
        results = self.chain_device(certs, policy, cert_status, cert_ok, revocation, anchor, now, allow_no_crl=allow_no_crl)
        torch.cuda.synchronize(self.device)
        if n_crls and int(totals.cpu().numpy().view(_crl_lib.TOTALS_DTYPE)[0]["overflow"]):
            raise RuntimeError("mldsa_crl_table: the lookup table overflowed")
        details = {k: v.cpu().numpy() for k, v in details.items()}
        if found is not None:
            details.update(MlDsaPathBuilder.host_results(found, n, n_crls))
        details.update(cert_ok=cert_ok.cpu().numpy(), cert_status=cert_status.cpu().numpy(),
                       policy=policy.cpu().numpy().view(_path_lib.FIELDS_DTYPE))
        res = results.cpu().numpy().view(_path_lib.RESULT_DTYPE)
        return res["verdict"].copy(), res["where"].copy(), res["depth"].copy(), details


class MlDsaPathBuilder:
    """The front of X.509 path validation on one GPU: libmldsa_find.so (include/mldsa_find.h) finds every certificate's issuer, every
    CRL's issuer and every certificate's CRL among an unordered bag of certificates, by subject Name, parameter set and key identifier.
    blob, certs, items: as MlDsaPathValidator's.  seed: 16 bytes that key the table's hash (drawn from the system's generator where
    None); hash_bits below 64 forces collisions, for tests.  Results never depend on either."""

    def __init__(self, device=0, hotpath=None, seed=None, hash_bits=64):
        self.hp = hotpath or HotPath(device)
        self.device = self.hp.device
        self.lib = _find_lib.load()
        self.x509, self.crl, self.path = _x509_lib.load(), _crl_lib.load(), _path_lib.load()
        self.seed = bytes(seed) if seed is not None else os.urandom(16)
        if len(self.seed) != 16:
            raise ValueError("seed: 16 bytes expected")
        self.hash_bits = int(hash_bits)

    _n = staticmethod(MlDsaRevocationLists._n)

    def _rows(self, n, size):
        return torch.empty(max(n, 1) * size, dtype=torch.uint8, device=self.device)

    def scratch_memory(self, n):
        return torch.empty(max(self.lib.mldsa_find_scratch_bytes(n), 256), dtype=torch.uint8, device=self.device)

    def parse_device(self, blob, certs):
        """mldsa_x509_parse and mldsa_path_parse, asynchronous on the current stream: (fields uint8 [n * 56], policy uint8 [n * 48])."""
        n = self._n(certs, None, 16, "certs")
        fields, policy = self._rows(n, 56), self._rows(n, 48)
        _x509_lib.check(self.x509.mldsa_x509_parse(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), n, _ptr(fields), _stream(self.device)))
        _path_lib.check(self.path.mldsa_path_parse(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), n, 0, _ptr(policy), _stream(self.device)))
        return fields[:n * 56], policy[:n * 48]

    def crl_parse_device(self, blob, items):
        """mldsa_crl_parse, asynchronous on the current stream: crl_fields uint8 [n_crls * 88]."""
        n = self._n(items, None, 16, "items")
        crl_fields = self._rows(n, 88)
        _crl_lib.check(self.crl.mldsa_crl_parse(self.hp._h, _ptr(blob), blob.numel(), _ptr(items), n, _ptr(crl_fields), _stream(self.device)))
        return crl_fields[:n * 88]

    def ids_device(self, blob, certs, policy):
        """mldsa_find_ids, asynchronous on the current stream: ids uint8 [n * 24], to be read as _find_lib.ID_DTYPE.  policy None: no
        identifiers are read."""
        n = self._n(certs, None, 16, "certs")
        ids = self._rows(n, 24)
        _find_lib.check(self.lib.mldsa_find_ids(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), None if policy is None else _ptr(policy), n,
                                                _ptr(ids), _stream(self.device)))
        return ids[:n * 24]

    def table_device(self, blob, certs, fields, ids, scratch=None):
        """mldsa_find_table, asynchronous on the current stream: (totals uint8 [16] -- _find_lib.TOTALS_DTYPE --, scratch, which holds the
        table)."""
        n = self._n(certs, None, 16, "certs")
        scratch = self.scratch_memory(n) if scratch is None else scratch
        totals = self._rows(1, 16)
        _find_lib.check(self.lib.mldsa_find_table(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), _ptr(fields), _ptr(ids), n, self.seed,
                                                  self.hash_bits, _ptr(totals), _ptr(scratch), scratch.numel(), _stream(self.device)))
        return totals, scratch

    def issuers_device(self, blob, certs, fields, ids, totals, scratch, in_place=False):
        """mldsa_find_issuers, asynchronous on the current stream: (certs_out uint8 [n * 16] -- certs itself with in_place --, results
        uint8 [n * 12], to be read as _find_lib.RESULT_DTYPE)."""
        n = self._n(certs, None, 16, "certs")
        certs_out = certs if in_place else self._rows(n, 16)
        results = self._rows(n, 12)
        _find_lib.check(self.lib.mldsa_find_issuers(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), _ptr(fields), _ptr(ids), n, self.seed,
                                                    self.hash_bits, _ptr(totals), _ptr(scratch), scratch.numel(), _ptr(certs_out), _ptr(results),
                                                    _stream(self.device)))
        return certs_out[:n * 16], results[:n * 12]

    def crl_issuers_device(self, blob, items, crl_fields, found):
        """mldsa_find_crl_issuers, asynchronous on the current stream: (items_out uint8 [n_crls * 16], results uint8 [n_crls * 12]).
        found: what build_device returned for the certificates."""
        n_crls = self._n(items, None, 16, "items")
        n = self._n(found["certs"], None, 16, "certs")
        items_out, results = self._rows(n_crls, 16), self._rows(n_crls, 12)
        _find_lib.check(self.lib.mldsa_find_crl_issuers(self.hp._h, _ptr(blob), blob.numel(), _ptr(items), _ptr(crl_fields), n_crls,
                                                        _ptr(found["certs"]), _ptr(found["fields"]), _ptr(found["ids"]), n, self.seed,
                                                        self.hash_bits, _ptr(found["totals"]), _ptr(found["scratch"]), found["scratch"].numel(),
                                                        _ptr(items_out), _ptr(results), _stream(self.device)))
        return items_out[:n_crls * 16], results[:n_crls * 12]

    def cert_crls_device(self, certs_out, items_out, scratch):
        """mldsa_find_cert_crls, asynchronous on the current stream: cert_crl int32 [n], -1 (MLDSA_CRL_NONE) where no CRL covers the
        certificate, as MlDsaRevocationLists.check_device takes it."""
        n = self._n(certs_out, None, 16, "certs")
        n_crls = self._n(items_out, None, 16, "items") if items_out is not None else 0
        cert_crl = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        _find_lib.check(self.lib.mldsa_find_cert_crls(self.hp._h, _ptr(certs_out), n, None if n_crls == 0 else _ptr(items_out), n_crls,
                                                      _ptr(cert_crl), _ptr(scratch), scratch.numel(), _stream(self.device)))
        return cert_crl[:n]

    def build_device(self, blob, certs, fields=None, policy=None, use_ids=True):
        """mldsa_find_build, asynchronous on the current stream, behind parse_device where fields is None: a dict of certs, fields,
        policy, ids, totals, certs_out, results and scratch.  use_ids False: policy NULL, matching by Name alone."""
        n = self._n(certs, None, 16, "certs")
        if fields is None:
            fields, policy = self.parse_device(blob, certs)
        ids, totals, certs_out, results, scratch = self._rows(n, 24), self._rows(1, 16), self._rows(n, 16), self._rows(n, 12), self.scratch_memory(n)
        _find_lib.check(self.lib.mldsa_find_build(self.hp._h, _ptr(blob), blob.numel(), _ptr(certs), _ptr(fields),
                                                  _ptr(policy) if use_ids and policy is not None else None, n, self.seed, self.hash_bits, _ptr(ids),
                                                  _ptr(totals), _ptr(certs_out), _ptr(results), _ptr(scratch), scratch.numel(),
                                                  _stream(self.device)))
        return dict(certs=certs, fields=fields, policy=policy, ids=ids[:n * 24], totals=totals, certs_out=certs_out[:n * 16],
                    results=results[:n * 12], scratch=scratch)

    @staticmethod
    def host_results(found, n, n_crls):
        """What a build found, as host arrays by name (after a synchronisation)."""
        res = found["results"].cpu().numpy().view(_find_lib.RESULT_DTYPE)[:n]
        out = dict(issuers=res["issuer"].copy(), candidates=res["candidates"].copy(), find_status=res["status"].copy(),
                   ids=found["ids"].cpu().numpy().view(_find_lib.ID_DTYPE)[:n], find_totals=found["totals"].cpu().numpy().view(_find_lib.TOTALS_DTYPE)[0])
        if "crl_results" in found:
            crl = found["crl_results"].cpu().numpy().view(_find_lib.RESULT_DTYPE)[:n_crls]
            out.update(crl_issuers=crl["issuer"].copy(), crl_candidates=crl["candidates"].copy(), crl_find_status=crl["status"].copy())
        if "cert_crl" in found:
            out.update(cert_crl=found["cert_crl"].cpu().numpy().view(np.uint32)[:n].copy())
        return out

    def build(self, cert_ders, crl_ders=(), pad=0, use_ids=True):
        """Host lists of DER certificates and CRLs in any order -> (issuers uint32 [n], candidates uint32 [n], cert_crl uint32 [n],
        details): for every certificate the index of its issuer (_find_lib.NO_ISSUER: none found), the number of certificates that
        matched, and the index of the lowest CRL of its issuer (_find_lib.CRL_NONE: none).  details: find_status, ids, find_totals and,
        with CRLs, crl_issuers, crl_candidates, crl_find_status."""
        n, n_crls = len(cert_ders), len(crl_ders)
        if n == 0:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), {}
        blob_h, rows = certificates_blob(list(cert_ders) + list(crl_ders), [None] * (n + n_crls), pad=pad)
        blob = torch.from_numpy(blob_h.copy()).to(self.device)
        certs = torch.from_numpy(np.ascontiguousarray(rows[:n]).view(np.uint8).reshape(-1).copy()).to(self.device)
        found = self.build_device(blob, certs, use_ids=use_ids)
        items_out = None
        if n_crls:
            items = torch.from_numpy(_crl_items(rows[n:]).view(np.uint8).reshape(-1).copy()).to(self.device)
            items_out, found["crl_results"] = self.crl_issuers_device(blob, items, self.crl_parse_device(blob, items), found)
        found["cert_crl"] = self.cert_crls_device(found["certs_out"], items_out, found["scratch"])
        torch.cuda.synchronize(self.device)
        out = self.host_results(found, n, n_crls)
        return out.pop("issuers"), out.pop("candidates"), out.pop("cert_crl"), out
