"""CPU reference of the device quantiles (kernels.quantiles / rdmi_quantiles): the key order, the rank rule and
the select, restated with numpy.  Nothing here calls the library."""
import numpy as np


def keys(v: np.ndarray) -> np.ndarray:
    """f32 values (no NaN) → uint32 keys whose unsigned order is the values' numeric order: −0 is made +0, negatives
    have all bits flipped, non-negatives the sign bit (csrc/select_key.h)."""
    v = np.ascontiguousarray(v, dtype=np.float32) + np.float32(0.0)  # −0 + 0 = +0
    b = v.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def values(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return b.view(np.float32)


def rank(q: float, cnt: int) -> int:
    """0-based rank of the fraction q among cnt ≥ 1 values: floor(q · (double)(cnt − 1)), one f64 multiply."""
    return int(np.floor(np.float64(q) * np.float64(cnt - 1)))


def select(x: np.ndarray, q, mask=None) -> np.ndarray:
    """f32 [len(q)]: per fraction the value of rank(q, cnt) among the kept (mask ≠ 0), non-NaN elements of x
    (f16 / f32, widened exactly), ordered by key — so −0 and +0 are one value, returned as +0 — by np.partition;
    NaN when nothing is kept."""
    v = np.asarray(x).astype(np.float32).reshape(-1)
    if mask is not None:
        v = v[np.asarray(mask).reshape(-1).astype(bool)]
    v = v[~np.isnan(v)]
    out = np.full(len(q), np.nan, np.float32)
    if v.size == 0:
        return out
    k = keys(v)
    ranks = [rank(f, k.size) for f in q]
    part = np.partition(k, sorted(set(ranks)))  # every listed rank holds its sorted value
    return values(part[ranks]).astype(np.float32)


def renorm_clip(x: np.ndarray, lo, hi) -> np.ndarray:
    """rdmi_renormalize_clip_f32 restated: f32 operations in the kernel's order, then the clamp."""
    lo, hi = np.float32(lo), np.float32(hi)
    v = x.astype(np.float32) - lo
    v = v / (hi - lo)
    v = v * np.float32(2.0) - np.float32(1.0)
    return np.clip(v, np.float32(-1.0), np.float32(1.0))
