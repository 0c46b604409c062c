"""Reference for the median merge (rdmi_aligner_merge_median and its sharded forms).  The covering terms of a
frame come from tests/uncertainty_util.py::frame_terms, which re-forms them bitwise; the reference sorts them
per pixel with np.sort and applies the rule of include/rdmi.h:
  median  c odd: the middle term; c even: (float)(((double)lo + (double)hi) · 0.5) of the two middle terms;
          c = 0: 0
  MAD     d_i = |a_i − median| as one f32 subtraction, then the median of the d_i by the same rule (raw: no
          1.4826 factor); 0 for c ≤ 1
Every step is exact or a single rounding that numpy performs as the device does, so the device result must
equal the reference under np.array_equal on the f32 values: no tolerance (a zero's sign is not compared)."""
import numpy as np

F32, F64 = np.float32, np.float64


def median_rule(a):
    """a [c, ...] f32 → the median over axis 0 by the rule above, f32 [...]."""
    a = np.asarray(a, F32)
    c = a.shape[0]
    if c == 0:
        return np.zeros(a.shape[1:], F32)
    srt = np.sort(a, axis=0)
    if c % 2:
        return srt[c // 2].copy()
    return ((srt[c // 2 - 1].astype(F64) + srt[c // 2].astype(F64)) * F64(0.5)).astype(F32)


def median_mad(a):
    """a [c, ...] f32 → (median, MAD), both f32 [...]."""
    a = np.asarray(a, F32)
    med = median_rule(a)
    if a.shape[0] == 0:
        return med, np.zeros_like(med)
    dev = np.abs((a - med[None]).astype(F32))
    return med, median_rule(dev)


def median_reference(frames):
    """frame_terms(...) → (median [N, HW] f32, MAD [N, HW] f32, cover counts [N])."""
    out = [median_mad(a) for a in frames]
    return (np.stack([m for m, _ in out]), np.stack([d for _, d in out]),
            np.array([a.shape[0] for a in frames]))
