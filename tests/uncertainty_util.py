"""Reference and tolerance for the merge's per-pixel spread (rdmi_aligner_merge_moments and its sharded
forms).  numpy re-forms every covering term a_i = s_k·(x − shift) + t_k bitwise, in the merge's order
(dilation ascending, slot descending), then takes a two-pass population standard deviation in longdouble.
The terms are the ones merge_k forms: x − shift rounded to f32, then — modes 1 and 2 — ONE rounding of
s·xs + t (the compiler turns merge_k's mulrn / addrn pair into a single fused multiply-add, and the mean
must stay merge_k's bitwise, so the spread is that of the same terms: fma32 below, exact in longdouble);
mode 0 follows the kernel's f16 chain, every step rounded through f16.

Tolerance, derived and not measured:  tol = 2⁻²²·ref + min(√E, E / ref),  E = (c + 4)·2⁻⁵²·max a_i².
E bounds the error of the kernel's variance Σa²/c − (Σa/c)²: the two f64 sums of c terms carry at most
(c − 1) roundings each, the two divisions, the product and the difference four more, every one at most
2⁻⁵³ relative to a quantity ≤ max a_i².  |√x − √y| ≤ |x − y| / √y gives E / ref, and |√x − √y| ≤ √|x − y|
covers ref → 0.  2⁻²²·ref covers the f64 sqrt and the one rounding to f32 with room to spare."""
import numpy as np

F32, F16 = np.float32, np.float16


def starts(N, w, dil, ss):
    """First frames of a dilation's snippets: every ss frames, plus the last window (csrc/aligner_index.h)."""
    last = N - ((w - 1) * dil + 1)
    st = list(range(0, last + 1, ss))
    if st[-1] < last:
        st.append(last)
    return st


def fma32(x, s, t):
    """round_f32(x·s + t) with one rounding, x / s / t f32.  The product of two f32 is exact in longdouble
    (48 of its 64 bits); the sum is checked for exactness with a two-sum and the few elements where it is
    not (exponents far apart) are redone in rational arithmetic."""
    from fractions import Fraction

    L = np.longdouble
    x, s, t = np.broadcast_arrays(np.asarray(x, F32), np.asarray(s, F32), np.asarray(t, F32))
    p = x.astype(L) * s.astype(L)
    tl = t.astype(L)
    sm = p + tl
    bb = sm - p
    err = (p - (sm - bb)) + (tl - bb)
    out = sm.astype(F32)
    for i in zip(*np.nonzero(err)):
        v = Fraction(float(x[i])) * Fraction(float(s[i])) + Fraction(float(t[i]))
        c0 = F32(float(v))  # within one f32 step of the answer: settle among the neighbours exactly, ties to even
        cand = [float(np.nextafter(c0, F32(-np.inf))), float(c0), float(np.nextafter(c0, F32(np.inf)))]
        best = min(cand, key=lambda c: (abs(Fraction(c) - v), int(F32(c).view(np.uint32)) & 1))
        out[i] = F32(best)
    return out


def terms(x, s, t, shift, mode):
    """The terms of x (any shape; f32 for mode 1, f16 for modes 0 / 2) under scale s and translation t (f32,
    broadcastable) after the shift, as f32 — bitwise what merge_k forms."""
    sh = F32(shift)
    if mode == 1:
        assert x.dtype == F32
        return fma32((x - sh).astype(F32), s, t)
    assert x.dtype == F16
    if mode == 2:
        return fma32((x.astype(F32) - sh).astype(F32), s, t)
    xs = (x.astype(F32) - sh).astype(F16)
    prod = (xs.astype(F32) * s.astype(F16).astype(F32)).astype(F16)
    return (prod.astype(F32) + t.astype(F16).astype(F32)).astype(F16).astype(F32)


def frame_terms(xf, sc, tr, dil, ss, N, shift, mode):
    """xf[d] [n_d, w_d, HW] → per frame the [c, HW] f32 covering terms in the merge's order (c may be 0)."""
    HW = xf[0].shape[-1]
    at = [{q: k for k, q in enumerate(starts(N, x.shape[1], d, s))} for x, d, s in zip(xf, dil, ss)]
    out = []
    for f in range(N):
        rows = []
        for d, x in enumerate(xf):
            for j in range(x.shape[1] - 1, -1, -1):
                k = at[d].get(f - j * dil[d])
                if k is not None:
                    rows.append(terms(x[k, j], sc[d][k], tr[d][k], shift, mode))
        out.append(np.stack(rows) if rows else np.zeros((0, HW), F32))
    return out


def spread_reference(frames):
    """frame_terms(...) → (std, tol, count): [N, HW] longdouble reference and tolerance, [N] cover counts."""
    N, HW = len(frames), frames[0].shape[1]
    ref = np.zeros((N, HW), np.longdouble)
    tol = np.zeros((N, HW), np.longdouble)
    cnt = np.array([a.shape[0] for a in frames])
    for f, a in enumerate(frames):
        c = a.shape[0]
        if c == 0:
            continue
        al = a.astype(np.longdouble)
        m = al.sum(0) / c
        ref[f] = np.sqrt(((al - m) ** 2).sum(0) / c)
        E = (c + 4) * np.longdouble(2.0) ** -52 * (al ** 2).max(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            lin = np.where(ref[f] > 0, E / ref[f], np.inf)
        tol[f] = np.longdouble(2.0) ** -22 * ref[f] + np.minimum(np.sqrt(E), lin)
    return ref, tol, cnt


def worst_ratio(got, ref, tol):
    """max |got − ref| / tol over the pixels with tol > 0, and whether got is exactly 0 wherever tol == 0."""
    err = np.abs(got.astype(np.longdouble) - ref)
    pos = tol > 0
    ratio = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    return ratio, bool((err[~pos] == 0).all())
