"""What the three test_gpu_vfy_*.py files share: the verify layer (include/mldsa_vfy.h) and the core's mldsa_verify called alike, the
stale verdict buffer and its reader, the per-op key gather and a library-signed batch.  Their `vfy` fixtures differ on purpose (one
forces parts of 64 ops, the others the shipped size) and stay with them.  Import by name, as with gpu_common."""
from fips204_amd import _lib, _vfy_lib
from fips204_amd.hotpath import _optr, _ptr, _stream
from fips204_amd.ml_dsa import MODE_PURE, PublicKeys, _cat_with_offsets
from gpu_common import filled, host, np, orc, shake, torch


def vfy_verify(lib, m, pks, mb, mo, sigs, ok, n, cb=None, co=None, kidx=None, mode=MODE_PURE, scratch=None):
    """the layer's call on torch's current stream, nothing waited for; on a pre-filled scratch of its own where none is given"""
    if scratch is None:
        scratch = filled(lib.mldsa_vfy_scratch_bytes(m.pset, n))
    _vfy_lib.check(lib.mldsa_vfy_verify(m.hp._h, m.pset, mode, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(kidx),
                                        _ptr(mb), _ptr(mo), _optr(cb), _optr(co), _ptr(sigs), _ptr(ok), n, _ptr(scratch), scratch.numel(),
                                        _stream(m.device)))
    return ok


def core_verify(m, pks, mb, mo, sigs, ok, n, cb=None, co=None, kidx=None, mode=MODE_PURE):
    _lib.check(m.lib.mldsa_verify(m.hp._h, m.pset, mode, _ptr(pks.rho), _ptr(pks.tr), _ptr(pks.t1_d2_hat_mont), len(pks), _optr(kidx), _ptr(mb),
                                  _ptr(mo), _optr(cb), _optr(co), _ptr(sigs), _ptr(ok), n, _stream(m.device)))
    return ok


def fresh(n):
    """a verdict buffer of stale bytes: every one must be overwritten"""
    return torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")


def verdicts(ok, n):
    got = host(ok)[:n]
    assert set(got.tolist()) <= {0, 1}
    return got.astype(bool)


def gathered(pks, kidx):
    """one key per op: the table's keys in the order of kidx"""
    g = torch.from_numpy(kidx.astype(np.int64)).cuda()
    return PublicKeys(pks.pset, pks.rho[g].contiguous(), pks.tr[g].contiguous(), pks.t1_d2_hat_mont[g].contiguous())


def vfy_expand_a(lib, m, rho):
    p = m.params
    n = rho.shape[0]
    out = torch.full((n, p.k * p.l, 256), -1, dtype=torch.int32, device="cuda")
    _vfy_lib.check(lib.mldsa_vfy_expand_a(m.hp._h, m.pset, _ptr(rho), _ptr(out), n, _stream(m.device)))
    return out


def signed_batch(m, tag, n, nk, msg_len):
    """n ops signed by the library under nk keys dealt 3 i mod nk, message i of msg_len(i) bytes, every byte derived from `tag`: the key
    table, the messages on the host and the device, the key indices and the signatures on the host, the oracle's keys"""
    xi = [shake(tag + b"-key%d" % m.pset, i) for i in range(nk)]
    pk, sk = m.keygen_from_seed(xi)
    pks, sks = m.public_keys_from_bytes(pk), m.private_keys_from_bytes(sk)
    msgs = [shake(tag + b"-msg%d" % m.pset, i, msg_len(i)) for i in range(n)]
    rnd = [shake(tag + b"-rnd", i) for i in range(n)]
    kidx = (np.arange(n) * 3 % nk).astype(np.uint32)
    sig = host(m.try_sign_with_seed(sks, msgs, rnd, key_idx=kidx, mode=MODE_PURE)).copy()
    mb, mo = _cat_with_offsets(msgs, m.device)
    okeys = [orc.pk_try_from_bytes(m.pset, host(pk)[i].tobytes()) for i in range(nk)]
    return dict(pks=pks, msgs=msgs, kidx=kidx, sig=sig, mb=mb, mo=mo, okeys=okeys)
