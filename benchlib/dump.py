"""--dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds can be compared output for output.

Every array is written as float32 (8- and 16-bit integers, bool) or float64 (wider integers): both hold every value exactly.  When the
arrays together would take more than MAX_BYTES, the same fixed, seeded sample of rows (first axis) is taken from each of them, and the
row numbers taken are written beside them as DIR/<name>_rows.npy."""
import os

import numpy as np

MAX_BYTES = 64 * 10**6
SAMPLE_SEED = 204


def _out_dtype(dt):
    if dt.kind in "iu" and dt.itemsize > 2 or dt == np.float64:
        return np.float64
    return np.float32


def _out_bytes(a):
    return a.size * np.dtype(_out_dtype(a.dtype)).itemsize


def to_host(tensors):
    """{name: device tensor} -> {name: numpy array}; called right after the timed region's final synchronize"""
    return {name: t.detach().cpu().numpy() for name, t in tensors.items()}


def write(out_dir, arrays, max_bytes=MAX_BYTES):
    """writes {name: numpy array}; returns {name: shape written}"""
    os.makedirs(out_dir, exist_ok=True)
    total = sum(_out_bytes(a) for a in arrays.values())
    frac = 1.0 if total <= max_bytes else 0.98 * max_bytes / total   # (2 % left for the row numbers)
    written = {}
    for name, a in arrays.items():
        rows = None
        if frac < 1.0 and a.ndim >= 1 and a.shape[0] > 1:
            k = max(1, int(a.shape[0] * frac))
            rows = np.sort(np.random.default_rng(SAMPLE_SEED).choice(a.shape[0], size=k, replace=False))
            a = a[rows]
        out = a.astype(_out_dtype(a.dtype))
        np.save(os.path.join(out_dir, name + ".npy"), out)
        written[name] = list(out.shape)
        if rows is not None:
            np.save(os.path.join(out_dir, name + "_rows.npy"), rows.astype(np.float64))
            written[name + "_rows"] = [int(rows.size)]
    return written
