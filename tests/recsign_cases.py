"""Cases for the request-signing library (include/mldsa_recsign.h) and a numpy restatement of what it must produce, written from the
rules the header states and not from the kernels: class and status of every descriptor, slots by input order within a class, the totals,
every packed array and offset table, and -- for given per-class signatures and status words -- the whole output buffer and the status
array.  Not a test file: test_recsign_cpu.py and test_gpu_recsign.py import it by name."""
import numpy as np

import rec_cases as rc
from fips204_amd import _recsign_lib
from fips204_amd.ml_dsa import sign_requests_blob

SIG_LEN = rc.SIG_LEN
SETS = rc.SETS               # class 0, 1, 2; class 3 = refused
REFUSED = 3
SCAN_BLOCK = 256             # MLDSA_RECSIGN_SCAN_BLOCK
PATTERN = rc.PATTERN         # fills the region refused ops point into
OK, ERR_PARAM, ERR_CTX_LEN = 0, -1, -2
FLAG_RND = 1
_bytes = rc._bytes


# ------------------------------------------------------------------------------------------------------------------- restatement
def verdict(op, blob_len, out_len, n_keys):
    """(class, status) of a descriptor by the header's five rules, in their order: Python integers, so nothing wraps.  n_keys: the rows
    of the three key tables in class order"""
    pset, flags = int(op["set"]), int(op["flags"])
    if pset not in SETS or flags & ~FLAG_RND or int(op["reserved"]) != 0:
        return REFUSED, ERR_PARAM
    if int(op["ctx_len"]) > 255:
        return REFUSED, ERR_CTX_LEN
    c = SETS.index(pset)
    if int(op["key"]) >= n_keys[c]:
        return REFUSED, ERR_PARAM
    ranges = [(op["msg_off"], op["msg_len"]), (op["ctx_off"], op["ctx_len"])] + ([(op["rnd_off"], 32)] if flags & FLAG_RND else [])
    if not all(rc.inside(int(o), int(n), blob_len) for o, n in ranges):
        return REFUSED, ERR_PARAM
    if not rc.inside(int(op["sig_off"]), SIG_LEN[pset], out_len):
        return REFUSED, ERR_PARAM
    return c, OK


def expected(blob, ops, n_keys, out_len):
    """dict(class_slot uint32 [n], status int32 [n] -- the refusal's code, 0 for an accepted op --, totals [10], packed {pset: dict(n,
    key_idx, rnd, msgs, msg_off, ctxs, ctx_off)}) for a blob (uint8 array) and its descriptors"""
    raw = blob.tobytes()
    count = [0, 0, 0, 0]
    rows = {c: dict(key=[], rnd=[], msgs=[], ctxs=[]) for c in range(3)}
    class_slot = np.zeros(len(ops), dtype=np.uint32)
    status = np.zeros(len(ops), dtype=np.int32)
    for i, op in enumerate(ops):
        c, status[i] = verdict(op, blob.size, out_len, n_keys)
        class_slot[i] = (c << 30) | count[c]
        count[c] += 1
        if c == REFUSED:
            continue
        cut = lambda off, n: raw[int(off):int(off) + int(n)]  # noqa: E731
        rows[c]["key"].append(int(op["key"]))
        rows[c]["rnd"].append(cut(op["rnd_off"], 32) if int(op["flags"]) & FLAG_RND else bytes(32))
        rows[c]["msgs"].append(cut(op["msg_off"], op["msg_len"]))
        rows[c]["ctxs"].append(cut(op["ctx_off"], op["ctx_len"]))
    packed, msg_bytes, ctx_bytes = {}, [], []
    for c, pset in enumerate(SETS):
        r = rows[c]
        off = lambda items: np.concatenate([[0], np.cumsum([len(b) for b in items], dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
        u8 = lambda items: np.frombuffer(b"".join(items), dtype=np.uint8)  # noqa: E731
        packed[pset] = dict(n=count[c], key_idx=np.array(r["key"], dtype=np.uint32), rnd=u8(r["rnd"]).reshape(-1, 32), msgs=u8(r["msgs"]),
                            msg_off=off(r["msgs"]), ctxs=u8(r["ctxs"]), ctx_off=off(r["ctxs"]))
        msg_bytes.append(int(packed[pset]["msg_off"][-1]))
        ctx_bytes.append(int(packed[pset]["ctx_off"][-1]))
    return dict(class_slot=class_slot, status=status, totals=count + msg_bytes + ctx_bytes, packed=packed)


def requests_of(packed):
    """the packed arrays of one class back as a list of (key, message, ctx, rnd)"""
    out = []
    for s in range(packed["n"]):
        m0, m1 = int(packed["msg_off"][s]), int(packed["msg_off"][s + 1])
        c0, c1 = int(packed["ctx_off"][s]), int(packed["ctx_off"][s + 1])
        out.append((int(packed["key_idx"][s]), packed["msgs"][m0:m1].tobytes(), packed["ctxs"][c0:c1].tobytes(), packed["rnd"][s].tobytes()))
    return out


def scattered(out_before, ops, want, sigs, status):
    """(out, status) after the scatter: out_before (uint8 array) with, for every accepted op in input order, row `slot` of
    sigs[pset] (uint8 [n_c, SIG_LEN]) at its sig_off; status[i] = status[pset][slot] of an accepted op, the refusal's code of a refused
    one.  want: expected() of the same descriptors."""
    out = np.array(out_before, dtype=np.uint8, copy=True)
    st = want["status"].copy()
    for i, op in enumerate(ops):
        c, slot = int(want["class_slot"][i]) >> 30, int(want["class_slot"][i]) & 0x3FFFFFFF
        if c == REFUSED:
            continue
        pset = SETS[c]
        at = int(op["sig_off"])
        out[at:at + SIG_LEN[pset]] = np.asarray(sigs[pset])[slot]
        st[i] = int(np.asarray(status[pset])[slot])
    return out, st


def _r(x):
    return (x + 255) // 256 * 256


def arena_bytes(n44, n65, n87, msg_bytes, ctx_bytes):
    """mldsa_recsign_arena_bytes as the header spells it"""
    per = sum(_r(4 * n) + 2 * _r(8 * (n + 1)) + _r(n * SIG_LEN[s]) + _r(4 * n) for s, n in zip(SETS, (n44, n65, n87)))
    return per + _r(32 * (n44 + n65 + n87)) + _r(msg_bytes) + _r(ctx_bytes)


def arena_bytes_max(n, msg_bytes, ctx_bytes):
    return 2 * _r(4 * n) + 2 * _r(8 * n + 24) + _r(4627 * n) + 5 * 512 + _r(32 * n) + _r(msg_bytes) + _r(ctx_bytes)


def plan_bytes(n):
    return _r(80 * ((n + SCAN_BLOCK - 1) // SCAN_BLOCK)) + 2 * _r(8 * n)


def front_bytes(n):
    return _r(4 * n) + 256 + plan_bytes(n)


# ------------------------------------------------------------------------------------------------------------------- cases
MIXES = rc.MIXES
N_KEYS = (4, 4, 4)  # rows of the three key tables of the seam cases


def seam_case(n, mix, seed=0, n_keys=N_KEYS):
    """(blob, ops, out_len) of n requests of arbitrary bytes -- the seam moves bytes, it does not read them --, the signature holes in a
    separate output buffer: gaps of 0 ... 15 bytes cycling in front of every field and every hole (starting at the seed), message and
    context lengths cycling through rc.MSG_LENS and rc.CTX_LENS at different periods, every third op without the rnd flag, keys dealt
    round-robin over the rows of the op's table.  The first hole lies at offset 0 of the output buffer and the last is flush with
    out_len.  Refused ops take one of DEFECTS in turn; their blob offsets point into a region of PATTERN bytes behind the requests.
    From three ops on, ops 1 and 2 share one message range; from six on, op 4's rnd range is op 3's message range's beginning."""
    sets, refused = rc.mix_sets(mix, n)
    reqs = []
    for i, pset in enumerate(sets):
        reqs.append((pset, i % n_keys[SETS.index(pset)], _bytes(b"rs-msg%d" % seed, i, rc.MSG_LENS[(i + seed) % len(rc.MSG_LENS)]),
                     _bytes(b"rs-ctx%d" % seed, i, rc.CTX_LENS[(i // 2 + seed) % len(rc.CTX_LENS)]),
                     None if i % 3 == 2 else _bytes(b"rs-rnd%d" % seed, i, 32)))
    gaps = [(j + seed) % 16 for j in range(16)]
    blob, ops, _ = sign_requests_blob(reqs, pad=gaps, front=seed % 5)
    region = blob.size
    blob = np.concatenate([blob, np.full(6000, PATTERN, dtype=np.uint8)])
    ops = ops.copy()
    at = 0
    for i, pset in enumerate(sets):  # the holes: the first at offset 0, the last flush with out_len
        gap = 0 if i == 0 else gaps[(3 * i) % 16]
        ops[i]["sig_off"] = at + gap
        at += gap + SIG_LEN[pset]
    out_len = at
    if n >= 3:
        ops[2]["msg_off"], ops[2]["msg_len"] = ops[1]["msg_off"], ops[1]["msg_len"]
    if n >= 6:
        ops[4]["rnd_off"] = ops[3]["msg_off"]
    for r, i in enumerate(sorted(refused)):
        make_refused(ops, i, r % len(DEFECTS), blob.size, out_len, region, n_keys)
    return blob, ops, out_len


# every defect but the last refuses its op under N_KEYS; "unserved_set" needs a call whose table of that set is empty
DEFECTS = ("unknown_set", "flag_bit_1", "reserved", "ctx_len_256", "key_is_n_keys", "msg_wraps", "rnd_one_past_end", "sig_off_top",
           "sig_one_past_out_len")
DEFECT_STATUS = {name: ERR_CTX_LEN if name == "ctx_len_256" else ERR_PARAM for name in DEFECTS}


def make_refused(ops, i, defect, blob_len, out_len, region, n_keys=N_KEYS):
    """damages descriptor i with DEFECTS[defect]; every blob offset of the op then points into the pattern region from `region` on
    (where that is compatible with the defect), so that a byte read for it would show; its hole stays where it was (where that is
    compatible with the defect), so that a byte written for it would show"""
    name = DEFECTS[defect] if isinstance(defect, int) else defect
    pset = int(ops[i]["set"])
    ops[i]["msg_off"], ops[i]["ctx_off"], ops[i]["rnd_off"] = region + 11, region + 13, region + 17
    ops[i]["msg_len"] = min(int(ops[i]["msg_len"]), 64)
    if name == "unknown_set":
        ops[i]["set"] = (43, 0, 66, 255)[i % 4]
    elif name == "flag_bit_1":
        ops[i]["flags"] = int(ops[i]["flags"]) | 2
    elif name == "reserved":
        ops[i]["reserved"] = 1 + i
    elif name == "ctx_len_256":
        ops[i]["ctx_len"] = 256
    elif name == "key_is_n_keys":
        ops[i]["key"] = n_keys[SETS.index(pset)]
    elif name == "msg_wraps":
        ops[i]["msg_off"], ops[i]["msg_len"] = 2 ** 64 - 8, 64
    elif name == "rnd_one_past_end":
        ops[i]["flags"], ops[i]["rnd_off"] = FLAG_RND, blob_len + 1 - 32
    elif name == "sig_off_top":
        ops[i]["sig_off"] = 2 ** 64 - 1
    elif name == "sig_one_past_out_len":
        ops[i]["sig_off"] = out_len + 1 - SIG_LEN[pset]
    else:
        raise ValueError(name)


ORACLE_N_KEYS = (2, 2, 2)


def oracle_key_seeds():
    """{pset: the two key seeds of oracle_requests()}"""
    return {pset: [bytes([16 * c + j + 1]) * 32 for j in range(2)] for c, pset in enumerate(SETS)}


def oracle_requests():
    """twelve requests, four per parameter set, two keys per set from the oracle: dict(keys {pset: [(pk, sk)]}, requests [(pset, key,
    message, ctx, rnd or None)], sigs: the oracle's signature of every request's own inputs)"""
    from oracle import oracle as orc
    keys = {pset: [orc.keygen_from_seed(pset, xi) for xi in seeds] for pset, seeds in oracle_key_seeds().items()}
    reqs, sigs = [], []
    for i in range(12):
        pset, key = SETS[i % 3], (i // 3) % 2
        msg = _bytes(b"rs-cpu-msg", i, rc.MSG_LENS[i % len(rc.MSG_LENS)])
        ctx = _bytes(b"rs-cpu-ctx", i, (0, 1, 255)[i % 3 if i < 9 else 0])
        rnd = None if i % 3 == 2 else bytes([0x80 + i]) * 32
        reqs.append((pset, key, msg, ctx, rnd))
        sigs.append(orc.sign_internal(pset, keys[pset][key][1], msg, rnd or bytes(32), ctx=ctx, mode=orc.MODE_PURE))
    return dict(keys=keys, requests=reqs, sigs=sigs)


def ops_dtype():
    return _recsign_lib.OP_DTYPE
