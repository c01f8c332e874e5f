"""Cases for the wire-record library (include/mldsa_rec.h) and a numpy restatement of what it must produce, written from the rules the
header states and not from the kernels: the range check and class of every descriptor, slots by input order within a class, the
totals, and every packed array and offset table.  Not a test file: test_records_cpu.py and test_gpu_records.py import it by name."""
import hashlib

import numpy as np

from fips204_amd import _rec_lib
from fips204_amd.ml_dsa import records_blob

PK_LEN = {44: 1312, 65: 1952, 87: 2592}
SIG_LEN = {44: 2420, 65: 3309, 87: 4627}
SETS = (44, 65, 87)          # class 0, 1, 2; class 3 = refused
REFUSED = 3
MSG_LENS = (0, 1, 3, 4, 15, 16, 17, 64, 1000)
CTX_LENS = (0, 1, 255)
SCAN_BLOCK = 256             # MLDSA_REC_SCAN_BLOCK
SEAM_SIZES = (1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 3)
PATTERN = 0x5E               # fills the region refused ops point into


def _bytes(tag, i, n):
    return hashlib.shake_256(tag + int(i).to_bytes(8, "little")).digest(n)


# ------------------------------------------------------------------------------------------------------------------- restatement
def inside(off, length, blob_len):
    """[off, off + length) lies in [0, blob_len): Python integers, so nothing wraps"""
    return 0 <= off and off + length <= blob_len


def class_of(op, blob_len):
    """0 / 1 / 2 for an accepted ML-DSA-44 / 65 / 87 op, 3 for a refused one"""
    pset = int(op["set"])
    if pset not in SETS or int(op["reserved"]) != 0 or int(op["ctx_len"]) > 255:
        return REFUSED
    ranges = ((op["pk_off"], PK_LEN[pset]), (op["sig_off"], SIG_LEN[pset]), (op["msg_off"], op["msg_len"]), (op["ctx_off"], op["ctx_len"]))
    if not all(inside(int(o), int(n), blob_len) for o, n in ranges):
        return REFUSED
    return SETS.index(pset)


def expected(blob, ops):
    """dict(class_slot uint32 [n], totals [10], packed {pset: dict(n, pk, sigs, msgs, msg_off, ctxs, ctx_off)}) for a blob (uint8
    array) and its descriptors"""
    blob_len = blob.size
    raw = blob.tobytes()
    count = [0, 0, 0, 0]
    rows = {c: dict(pk=[], sigs=[], msgs=[], ctxs=[]) for c in range(3)}
    class_slot = np.zeros(len(ops), dtype=np.uint32)
    for i, op in enumerate(ops):
        c = class_of(op, blob_len)
        class_slot[i] = (c << 30) | count[c]
        count[c] += 1
        if c == REFUSED:
            continue
        pset = SETS[c]
        cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
        rows[c]["pk"].append(cut(op["pk_off"], PK_LEN[pset]))
        rows[c]["sigs"].append(cut(op["sig_off"], SIG_LEN[pset]))
        rows[c]["msgs"].append(cut(op["msg_off"], op["msg_len"]))
        rows[c]["ctxs"].append(cut(op["ctx_off"], op["ctx_len"]))
    packed, msg_bytes, ctx_bytes = {}, [], []
    for c, pset in enumerate(SETS):
        r = rows[c]
        off = lambda items: np.concatenate([[0], np.cumsum([len(b) for b in items], dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
        u8 = lambda items: np.frombuffer(b"".join(items), dtype=np.uint8)  # noqa: E731
        packed[pset] = dict(n=count[c], pk=u8(r["pk"]).reshape(-1, PK_LEN[pset]), sigs=u8(r["sigs"]).reshape(-1, SIG_LEN[pset]),
                            msgs=u8(r["msgs"]), msg_off=off(r["msgs"]), ctxs=u8(r["ctxs"]), ctx_off=off(r["ctxs"]))
        msg_bytes.append(int(packed[pset]["msg_off"][-1]))
        ctx_bytes.append(int(packed[pset]["ctx_off"][-1]))
    return dict(class_slot=class_slot, totals=count + msg_bytes + ctx_bytes, packed=packed)


def records_of(packed):
    """the packed arrays of one class back as a list of (pk, message, sig, ctx)"""
    out = []
    for s in range(packed["n"]):
        m0, m1 = int(packed["msg_off"][s]), int(packed["msg_off"][s + 1])
        c0, c1 = int(packed["ctx_off"][s]), int(packed["ctx_off"][s + 1])
        out.append((packed["pk"][s].tobytes(), packed["msgs"][m0:m1].tobytes(), packed["sigs"][s].tobytes(), packed["ctxs"][c0:c1].tobytes()))
    return out


def arena_bytes(n44, n65, n87, msg_bytes, ctx_bytes):
    """mldsa_rec_scratch_bytes as the header spells it"""
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    per = sum(r(n * PK_LEN[s]) + r(n * SIG_LEN[s]) + 2 * r(8 * (n + 1)) + r(n) for s, n in zip(SETS, (n44, n65, n87)))
    return per + r(msg_bytes) + r(ctx_bytes)


def arena_bytes_max(n, msg_bytes, ctx_bytes):
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r(2592 * n) + r(4627 * n) + 2 * r(8 * n + 24) + r(n) + 5 * 512 + r(msg_bytes) + r(ctx_bytes)


def plan_bytes(n):
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r(80 * ((n + SCAN_BLOCK - 1) // SCAN_BLOCK)) + 2 * r(8 * n)


def front_bytes(n):
    return (4 * n + 255) // 256 * 256 + 256 + plan_bytes(n)


# ------------------------------------------------------------------------------------------------------------------- cases
MIXES = ("only44", "only65", "only87", "all_refused", "mod3", "tenth_refused")


def mix_sets(mix, n):
    """the parameter set of every op, and which ops are to be refused"""
    if mix.startswith("only"):
        return [int(mix[4:])] * n, set()
    sets = [SETS[i % 3] for i in range(n)]
    if mix == "all_refused":
        return sets, set(range(n))
    if mix == "tenth_refused":
        return sets, set(range(9, n, 10))
    return sets, set()


def seam_case(n, mix, seed=0):
    """(blob, ops) of n records of arbitrary bytes -- the seam moves bytes, it does not read them --: gaps of 0 ... 15 bytes cycling in
    front of every field (starting at the seed; the odd signature lengths then bring every source residue to every destination
    residue), message and context lengths cycling through MSG_LENS and CTX_LENS at different periods, the blob's first field at offset `seed % 5`.
    Refused ops take one of six defects in turn; their offsets point into a region of PATTERN bytes behind the records.
    From three ops on: ops 1 and 2 share one message range; from six on, ops 3 + 3 k of one set share a key range and op 5's message
    overlaps op 4's signature partially."""
    sets, refused = mix_sets(mix, n)
    recs = []
    for i, pset in enumerate(sets):
        recs.append((pset, _bytes(b"rec-pk%d" % seed, i, PK_LEN[pset]), _bytes(b"rec-msg%d" % seed, i, MSG_LENS[(i + seed) % len(MSG_LENS)]),
                     _bytes(b"rec-sig%d" % seed, i, SIG_LEN[pset]), _bytes(b"rec-ctx%d" % seed, i, CTX_LENS[(i // 2 + seed) % len(CTX_LENS)])))
    gaps = [(j + seed) % 16 for j in range(16)]
    blob, ops = records_blob(recs, pad=gaps, front=seed % 5)
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, PATTERN, dtype=np.uint8)])
    ops = ops.copy()
    if n >= 3:
        ops[2]["msg_off"], ops[2]["msg_len"] = ops[1]["msg_off"], ops[1]["msg_len"]
    if n >= 6:
        same = [j for j in range(3, n, 3) if sets[j] == sets[3]][:3]
        for j in same[1:]:
            ops[j]["pk_off"] = ops[3]["pk_off"]
        ops[5]["msg_off"], ops[5]["msg_len"] = int(ops[4]["sig_off"]) + 5, 100
    for r, i in enumerate(sorted(refused)):
        make_refused(ops, i, r % len(DEFECTS), blob.size, region)
    return blob, ops


DEFECTS = ("unknown_set", "reserved", "ctx_len_256", "pk_one_past_end", "sig_off_top", "msg_wraps")


def make_refused(ops, i, defect, blob_len, region):
    """damages descriptor i with DEFECTS[defect]; every offset of the op then points into the pattern region from `region` on (where
    that is compatible with the defect), so that a byte read for it would show"""
    name = DEFECTS[defect] if isinstance(defect, int) else defect
    pset = int(ops[i]["set"])
    ops[i]["pk_off"], ops[i]["sig_off"], ops[i]["msg_off"], ops[i]["ctx_off"] = region + 1, region + 7, region + 11, region + 13
    ops[i]["msg_len"] = min(int(ops[i]["msg_len"]), 64)
    if name == "unknown_set":
        ops[i]["set"] = (43, 0, 66, 255)[i % 4]
    elif name == "reserved":
        ops[i]["reserved"] = 1 + i % 255
    elif name == "ctx_len_256":
        ops[i]["ctx_len"] = 256
    elif name == "pk_one_past_end":
        ops[i]["pk_off"] = blob_len + 1 - PK_LEN[pset]
    elif name == "sig_off_top":
        ops[i]["sig_off"] = 2 ** 64 - 1
    elif name == "msg_wraps":
        ops[i]["msg_off"], ops[i]["msg_len"] = 2 ** 64 - 8, 64
    else:
        raise ValueError(name)


def ops_dtype():
    return _rec_lib.OP_DTYPE
