"""mldsa_vfy_verify (include/mldsa_vfy.h) as the order plan enqueues it: a call of one part is one chain on the caller's stream (ExpandA,
k_verify_main, the c~ hash) with the front on a library stream beside it, a call of several parts is the three-stream pipeline.  Either
way the call must behave as one item of the caller's stream: behind what the stream held, ahead of what follows, calls on one scratch one
after the other.  257 ops over 5 keys per parameter set, every 7th signature damaged (in c~, in z, in the hint section, in turn), at 1,
64, 65 and 257 ops, against mldsa_verify on the same inputs and the oracle op for op.  The layer is called directly, so the routing
threshold does not apply; every call is a few hundred ops at most."""
from fips204_amd import _vfy_lib
from fips204_amd.ml_dsa import MODE_PURE
from gpu_common import *
from sig_cases import spans
from vfy_calls import core_verify, fresh, signed_batch, verdicts, vfy_verify

pytestmark = pytest.mark.gpu

N_OPS, N_KEYS = 257, 5
SIZES = (1, 64, 65, 257)
FIRST_BAD = 3  # ops 3, 10, 17, ... are damaged: op 0 is good, so a call of one op has a verdict to lose


# ------------------------------------------------------------------------------------------------- the damaged batch, on the CPU
def damaged_batch(p, sig):
    """(a copy of the signatures [n, sig_len] with every 7th damaged by one flipped bit, the damaged ops): the t-th damage lies in c~, z and
    the hint section in turn, and walks through its section with t"""
    out = sig.copy()
    ops = list(range(FIRST_BAD, sig.shape[0], 7))
    for t, op in enumerate(ops):
        lo, hi = spans(p)[t % 3]
        out[op, lo + (131 * (t // 3)) % (hi - lo)] ^= 1 << (t % 8)
    return out, ops


def all_damaged(sig):
    """every signature refused: one bit of c~ flipped in each"""
    out = sig.copy()
    out[:, 5] ^= 0x04
    return out


# --------------------------------------------------------------------------------------------------------------- the calls
@pytest.fixture(scope="module")
def vfy():
    lib = _vfy_lib.load()
    lib.mldsa_vfy_set_part_ops(0)  # the part size the library ships with: every call below is one part unless a test says otherwise
    return lib


def vfy_enqueue(lib, m, b, sigs, ok, n, scratch):
    """the layer's call on torch's current stream, nothing waited for"""
    vfy_verify(lib, m, b["pks"], b["mb"], b["mo"], sigs, ok, n, kidx=b["kidx"], scratch=scratch)


_batches = {}


def batch(m):
    """Per parameter set, built once and never changed: 257 ops signed under 5 keys, the damaged copy, and for both the oracle's verdicts
    op for op and the core's at every size of SIZES (and at 200 ops, the several-parts case)."""
    if m.pset in _batches:
        return _batches[m.pset]
    s = signed_batch(m, b"chain", N_OPS, N_KEYS, lambda i: (0, 1, 33, 70, 135, 136, 300)[i % 7])
    assert len(s["pks"]) == N_KEYS
    clean, kidx, msgs, okeys = s["sig"], s["kidx"], s["msgs"], s["okeys"]
    bad, ops = damaged_batch(m.params, clean)
    b = dict(pks=s["pks"], kidx=kidx_dev(kidx), mb=s["mb"], mo=s["mo"], clean=dev(clean), bad=dev(bad), none=dev(all_damaged(clean)), ops=ops)
    # ---- the oracle, op for op: the clean signatures pass, the damaged ones are refused and nothing else is
    for name, sg in (("clean", clean), ("bad", bad)):
        b["want_" + name] = [bool(orc.verify_internal(m.pset, okeys[int(kidx[i])], msgs[i], bytes(sg[i]), mode=MODE_PURE)) for i in range(N_OPS)]
    assert all(b["want_clean"])
    assert b["want_bad"] == [i not in ops for i in range(N_OPS)] and len(ops) == 37
    # ---- the core on the same inputs, at every size: the same verdicts
    for n in SIZES + (200,):
        for name in ("clean", "bad"):
            ok = core_verify(m, b["pks"], b["mb"], b["mo"], b[name], fresh(n), n, kidx=b["kidx"])
            assert verdicts(ok, n).tolist() == b["want_" + name][:n], (n, name)
    _batches[m.pset] = b
    return b


def scratch_for(lib, m, n):
    return filled(lib.mldsa_vfy_scratch_bytes(m.pset, n))


# --------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_on_the_default_stream_and_on_a_side_stream(vfy, sets, pset, n):
    m = sets[pset]
    b = batch(m)
    assert (n + _vfy_lib.part_ops() - 1) // _vfy_lib.part_ops() == 1  # one part: the chain on the caller's stream
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    ok = fresh(n)
    vfy_enqueue(vfy, m, b, b["bad"], ok, n, scratch_for(vfy, m, n))
    assert verdicts(ok, n).tolist() == b["want_bad"][:n]
    side = torch.cuda.Stream()
    ok, scratch = fresh(n), scratch_for(vfy, m, n)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vfy_enqueue(vfy, m, b, b["bad"], ok, n, scratch)
    side.synchronize()  # the caller's stream alone: the call has folded the library's stream back into it
    assert ok.cpu().numpy()[:n].astype(bool).tolist() == b["want_bad"][:n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_between_a_producer_and_a_consumer_on_the_callers_stream(vfy, sets, pset, n):
    """the signatures are written by an asynchronous copy right ahead of the call and overwritten by one right behind it, nothing waited
    for in between: a call that read early would see the stale bytes, one that read late the overwritten ones -- both refuse every op"""
    m = sets[pset]
    b = batch(m)
    assert b["want_bad"][0]
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        sigs = torch.full_like(b["bad"][:n], 0x5A)
        ok, scratch = fresh(n), scratch_for(vfy, m, n)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            sigs.copy_(b["bad"][:n], non_blocking=True)
            vfy_enqueue(vfy, m, b, sigs, ok, n, scratch)
            sigs.copy_(b["none"][:n], non_blocking=True)
        stream.synchronize()
        assert ok.cpu().numpy()[:n].astype(bool).tolist() == b["want_bad"][:n]
        assert torch.equal(sigs, b["none"][:n])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset", [44, 65, 87])
def test_three_calls_back_to_back_on_one_scratch(vfy, sets, pset, n):
    m = sets[pset]
    b = batch(m)
    scratch = scratch_for(vfy, m, n)
    oks = [fresh(n) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for ok, name in zip(oks, ("clean", "bad", "clean")):
            vfy_enqueue(vfy, m, b, b[name], ok, n, scratch)
    side.synchronize()
    for ok, name in zip(oks, ("clean", "bad", "clean")):
        assert ok.cpu().numpy()[:n].astype(bool).tolist() == b["want_" + name][:n], name


@pytest.mark.parametrize("pset", [44, 65, 87])
def test_four_parts_of_64_ops_reuse_the_ring(vfy, sets, pset):
    """200 ops in parts of 64: parts 2 and 3 write the ring halves parts 0 and 1 read.  A call of one part runs right behind it on the
    same scratch and the same library streams."""
    m = sets[pset]
    b = batch(m)
    n = 200
    assert vfy.mldsa_vfy_set_part_ops(64) == _vfy_lib.part_ops()
    try:
        scratch = scratch_for(vfy, m, n)
        ok, ok2, ok3 = fresh(n), fresh(n), fresh(64)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vfy_enqueue(vfy, m, b, b["bad"], ok, n, scratch)
            vfy_enqueue(vfy, m, b, b["clean"], ok2, n, scratch)
            vfy_enqueue(vfy, m, b, b["bad"], ok3, 64, scratch)  # one part
        side.synchronize()
        assert ok.cpu().numpy()[:n].astype(bool).tolist() == b["want_bad"][:n]
        assert ok2.cpu().numpy()[:n].astype(bool).tolist() == b["want_clean"][:n]
        assert ok3.cpu().numpy()[:64].astype(bool).tolist() == b["want_bad"][:64]
    finally:
        assert vfy.mldsa_vfy_set_part_ops(0) == 64
