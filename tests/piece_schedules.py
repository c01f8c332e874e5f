"""What the incremental pre-hash and incremental-mu inputs (ph_stream_cases, mus_cases) share: the pieces of one update of a schedule
(ops, cuts), and seeded cuts and their pieces vectorised for the batches of 65 536 ops.  Pure numpy."""
import numpy as np


def pieces_of(messages, ops, cuts, u):
    """update u of a schedule as byte strings, one per op of the schedule"""
    return [messages[i][cs[u]:cs[u + 1]] for i, cs in zip(ops, cuts)]


def random_cuts(lens, n_updates, rng):
    """[n, n_updates + 1] cut positions for messages of the given lengths, vectorised"""
    n = lens.size
    inner = np.sort(rng.integers(0, lens[:, None] + 1, (n, n_updates - 1)), axis=1) if n_updates > 1 else np.zeros((n, 0), dtype=np.int64)
    return np.concatenate([np.zeros((n, 1), dtype=np.int64), inner, lens[:, None].astype(np.int64)], axis=1)


def gather_pieces(buf, off, cuts, u):
    """(flat, offsets) of update u: piece i = buf[off[i] + cuts[i, u] : off[i] + cuts[i, u + 1]], packed back to back"""
    start = off[:-1].astype(np.int64) + cuts[:, u]
    plen = cuts[:, u + 1] - cuts[:, u]
    poff = np.zeros(plen.size + 1, dtype=np.uint64)
    np.cumsum(plen, out=poff[1:])
    idx = np.repeat(start - poff[:-1].astype(np.int64), plen) + np.arange(int(poff[-1]), dtype=np.int64)
    return buf[idx], poff
