"""numpy f64 reference of the alignment spaces and the temporal pass of rollingdepth_amd.metrics (rdmi.h
"Alignment space", "Temporal consistency"), and the seeded inputs the CPU and GPU tests share.

The reference reads the dtype-rounded operands as f64 and the float32-rounded lo / hi, as the device does.  Where
the device rounds once (d = fma(s, p, t)) numpy rounds twice (s * p + t): that is the 2⁻⁵³ per aligned value which
the tests' relative 1e-10 on the sums covers.  The bilinear formula is evaluated operation by operation, as the
device evaluates it.
"""
import functools
import math

import numpy as np
import torch

SHAPES = [(3, 7, 9, 0), (2, 33, 31, 1), (5, 64, 48, 2), (2, 96, 96, 4)]
F16, F32 = torch.float16, torch.float32
DT = {F16: "f16", F32: "f32", None: "none"}
SPACES = ("depth", "disparity", "log")
THR = (1.25, 1.25 ** 2, 1.25 ** 3)
LO = 1e-3
U = 2.0 ** -53


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(shape, space="depth"):
    """p on the 2⁻¹⁰ grid in [1/8, 1), target = φ⁻¹((1.5 p + 0.25)·r) in f64 (the caller rounds it to the target
    dtype), r in [1/2, 2), and a mask of density 3/4 — the construction of tests/test_metrics_gpu.py."""
    N, H, W, seed = shape
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(128, 1024, (N, H, W), generator=g) / 1024
    r = torch.randint(512, 2048, (N, H, W), generator=g) / 1024
    lin = (1.5 * p.double() + 0.25) * r.double()
    gt = {"depth": lin, "disparity": 1.0 / lin, "log": torch.exp(lin)}[space]
    m = torch.randint(0, 4, (N, H, W), generator=g) > 0
    return p, gt, m


@functools.lru_cache(maxsize=None)
def temporal_inputs(shape, k):
    """flow [N − k, H, W, 2] on the ¼-pixel grid with |dx|, |dy| ≤ 3, and the temporal masks of density 7/8: one
    per frame [N, H, W] and one per pair [N − k, H, W]."""
    N, H, W, seed = shape
    g = torch.Generator().manual_seed(1000 + 10 * seed + k)
    flow = torch.randint(-12, 13, (N - k, H, W, 2), generator=g).float() / 4
    mask = torch.randint(0, 8, (N, H, W), generator=g) > 0
    pair_mask = torch.randint(0, 8, (N - k, H, W), generator=g) > 0
    return flow, mask, pair_mask


# every pred / target dtype × mask combination on the first two shapes, one on the rest
SPACE_CASES = [(s, pd, td, mk) for s in SHAPES[:2] for pd in (F16, F32) for td in (F16, F32) for mk in (False, True)]
SPACE_CASES += [(s, F32, F32, True) for s in SHAPES[2:]]
SPACE_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{DT[pd]}-{DT[td]}-{'mask' if mk else 'nomask'}" for s, pd, td, mk in SPACE_CASES]
CLIP = (0.1, 10.0)  # of the disparity-space temporal cases

# (shape index, pred dtype, target dtype or None, mask, flow, pair_mask, frame_step, align, space): the temporal
# pass's options spread over the four shapes, not their product
TEMPORAL_CASES = [
    (0, F32, F32, 0, 0, 0, 1, "video", "depth"),
    (0, F16, F16, 1, 0, 1, 2, "frame", "depth"),
    (0, F32, F16, 0, 1, 0, 1, "video", "depth"),
    (0, F16, F32, 1, 1, 0, 1, "frame", "disparity"),
    (0, F32, None, 1, 1, 0, 2, "none", "depth"),
    (0, F16, None, 0, 0, 1, 1, "none", "depth"),
    (0, F32, F32, 0, 1, 1, 1, "video", "disparity"),
    (1, F32, F32, 1, 1, 1, 1, "video", "depth"),
    (1, F16, F32, 0, 1, 0, 1, "frame", "depth"),
    (1, F32, F16, 1, 0, 0, 1, "video", "disparity"),
    (1, F16, F16, 0, 1, 1, 1, "frame", "disparity"),
    (1, F32, None, 0, 1, 1, 1, "none", "depth"),
    (1, F16, None, 1, 0, 0, 1, "none", "disparity"),
    (1, F32, F32, 1, 1, 0, 1, "none", "log"),
    (1, F16, F16, 1, 0, 1, 1, "video", "depth"),
    (2, F32, F32, 1, 1, 1, 1, "video", "depth"),
    (2, F16, F32, 0, 1, 0, 2, "frame", "depth"),
    (2, F32, F16, 1, 0, 1, 2, "video", "disparity"),
    (2, F32, None, 1, 1, 1, 2, "none", "depth"),
    (2, F16, F16, 1, 1, 0, 1, "frame", "disparity"),
    (2, F32, F32, 0, 0, 0, 1, "frame", "log"),
    (3, F32, F32, 1, 1, 1, 1, "video", "depth"),
    (3, F16, F16, 0, 0, 0, 1, "frame", "depth"),
    (3, F32, F16, 1, 1, 0, 1, "frame", "disparity"),
    (3, F16, None, 0, 1, 1, 1, "none", "depth"),
    (3, F16, F32, 1, 0, 1, 1, "video", "disparity"),
]
TEMPORAL_IDS = [f"{'x'.join(map(str, SHAPES[c[0]][:3]))}-{DT[c[1]]}-{DT[c[2]]}-{'mask' if c[3] else 'nomask'}-"
                f"{'flow' if c[4] else 'noflow'}-{'pm' if c[5] else 'nopm'}-k{c[6]}-{c[7]}-{c[8]}"
                for c in TEMPORAL_CASES]


def temporal_case(ci):
    """Host tensors of a temporal case: pred, target or None, mask or None, flow or None, pair_mask or None, and the
    keyword arguments of temporal_metrics."""
    si, pd, td, mk, fl, pm, k, align, space = TEMPORAL_CASES[ci]
    shape = SHAPES[si]
    p, gt, _ = inputs(shape, space)
    flow, mask, pair_mask = temporal_inputs(shape, k)
    kw = {"frame_step": k, "align": align, "space": space, "clip": CLIP if space == "disparity" else None}
    return (p.to(pd), None if td is None else gt.to(td), mask if mk else None, flow if fl else None,
            pair_mask if pm else None, kw)


@functools.lru_cache(maxsize=None)
def temporal_reference(ci):
    """Computed once per case and shared: (s, t) of the numpy fit and the [N − k, 8] sums."""
    p, g, m, flow, pm, kw = temporal_case(ci)
    N, H, W = p.shape
    pn, gn = f64(p), (None if g is None else f64(g))
    mn = None if m is None else m.numpy().reshape(N, -1)
    if kw["align"] == "none":
        s, t = np.ones(N), np.zeros(N)
    else:
        mom, mom_abs = ref_moments(pn, gn, ref_valid(pn, gn, mn, space=kw["space"]), kw["space"])
        s, t, _ = ref_fit(mom, mom_abs, kw["align"])
    sums = ref_temporal(pn, gn, mn, None if flow is None else flow.numpy(), None if pm is None else pm.numpy(), (s, t),
                        kw["frame_step"], H, W, kw["space"], kw["clip"])
    return s, t, sums


def f64(t):
    return t.detach().cpu().double().numpy().reshape(t.shape[0], -1)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ----------------------------------------------------------------------------- spaces
def to_space(g, space):
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"depth": lambda: g, "disparity": lambda: 1.0 / g, "log": lambda: np.log(g)}[space]()


def from_space(d, space):
    if space == "disparity":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(d > 0, 1.0 / d, np.inf)
    return np.exp(d) if space == "log" else d


def aligned(p, s, t, space, clip=None):
    """a = clamp(φ⁻¹(s·p + t)) of one frame."""
    d = s * p + t
    a = from_space(d, space)
    return a if clip is None else np.clip(a, clip[0], clip[1])


def ref_valid(p, g, m, lo=LO, hi=math.inf, space="depth"):
    v = np.isfinite(p)
    if g is not None:
        v = v & np.isfinite(g) & (g > float(np.float32(lo))) & (g < float(np.float32(hi)))
        if space != "depth":
            v = v & (g > 0)
    return v if m is None else v & (m.reshape(v.shape) != 0)


# ----------------------------------------------------------------------------- moments, fit, errors
def ref_moments(p, g, v, space):
    """[N, 6] sums of 1, p, φ, p², pφ, φ² over the valid pixels, and [N, 6] sums of |terms|."""
    phi = np.where(v, to_space(np.where(v, g, 1.0), space), 0.0)
    p = np.where(v, p, 0.0)
    terms = np.stack([v.astype(np.float64), p, phi, p * p, p * phi, phi * phi], -1)
    return terms.sum(1), np.abs(terms).sum(1)


def ref_solve(mom, mom_abs):
    """(s, t, conditioning) of moments [..., 6]: conditioning = the factor from a relative error of the moments (relative
    to their sums of |terms|) to the relative error of s and of t, the numerators' and the determinant's
    cancellation both counted."""
    n, sp, sg, spp, spg = (mom[..., k] for k in range(5))
    ap, ag, apg = mom_abs[..., 1], mom_abs[..., 2], mom_abs[..., 4]
    det = n * spp - sp * sp
    ok = (n >= 2) & (det > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ns, nt = n * spg - sp * sg, spp * sg - sp * spg
        s, t = np.where(ok, ns / det, np.nan), np.where(ok, nt / det, np.nan)
        cdet = (n * spp + 2 * ap * ap) / det
        cs = (n * apg + 2 * ap * ag) / np.abs(ns) + cdet
        ct = (spp * ag + 2 * ap * apg) / np.abs(nt) + cdet
    return s, t, np.where(ok, np.maximum(cs, ct), np.nan)


def ref_fit(mom, mom_abs, align):
    N = mom.shape[0]
    if align == "none":
        return np.ones(N), np.zeros(N), np.ones(N)
    if align == "video":
        s, t, c = ref_solve(mom.sum(0), mom_abs.sum(0))
        return np.full(N, s), np.full(N, t), np.full(N, c)
    return ref_solve(mom, mom_abs)


def ref_errors(p, g, v, s, t, space="depth", clip=None):
    """[N, 8] sums of rdmi_depth_errors_space, the smallest distance of a ratio max(a/g, g/a) to a δ threshold,
    and the smallest aligned value d = s·p + t in the fit space."""
    out = np.zeros((p.shape[0], 8))
    dist, dmin = math.inf, math.inf
    for f in range(p.shape[0]):
        if math.isnan(s[f]) or math.isnan(t[f]):
            continue
        pf, gf = p[f][v[f]], g[f][v[f]]
        a = aligned(pf, s[f], t[f], space, clip)
        if pf.size:
            dmin = min(dmin, (s[f] * pf + t[f]).min())
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(a - gf)
            ratio = np.where((a > 0) & np.isfinite(a), np.maximum(a / gf, gf / a), np.inf)
            out[f, :5] = [pf.size, d.sum(), (d / gf).sum(), (d * d).sum(), (d * d / gf).sum()]
        for k, c in enumerate(THR):
            out[f, 5 + k] = (ratio < c).sum()
            if ratio.size:
                dist = min(dist, np.abs(ratio - c).min())
    return out, dist, dmin


def ref_metrics(sums):
    tot = sums.sum(0)
    n = tot[0]
    return {"mae": tot[1] / n, "abs_rel": tot[2] / n, "rmse": math.sqrt(tot[3] / n), "sq_rel": tot[4] / n,
            "delta1": tot[5] / n, "delta2": tot[6] / n, "delta3": tot[7] / n}


# ----------------------------------------------------------------------------- temporal pass
def _bilerp(wx, wy, v00, v01, v10, v11):
    with np.errstate(invalid="ignore"):
        return (1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11)


def ref_temporal(p, g, m, flow, pair_mask, st, k, H, W, space="depth", clip=None, lo=LO, hi=math.inf):
    """[N − k, 8] sums of rdmi_depth_temporal.  p, g (or None) [N, P] f64; m [N, P] or None; flow [N − k, H, W, 2]
    or None; pair_mask [N − k, P] or None; st = (s [N], t [N])."""
    s, t = st
    N, P = p.shape
    v = ref_valid(p, g, m, lo, hi, space)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.stack([aligned(p[f], s[f], t[f], space, clip) for f in range(N)])
    yy, xx = np.divmod(np.arange(P), W)
    out = np.zeros((N - k, 8))
    for i in range(N - k):
        f0, f1 = i, i + k
        if any(math.isnan(x) for x in (s[f0], t[f0], s[f1], t[f1])):
            continue
        ok = v[f0].copy()
        if pair_mask is not None:
            ok &= pair_mask[i].reshape(-1) != 0
        if flow is None:
            ok &= v[f1]
            a1, g1 = a[f1], (None if g is None else g[f1])
        else:
            fl = flow[i].reshape(P, 2).astype(np.float64)
            with np.errstate(invalid="ignore"):
                X, Y = xx + fl[:, 0], yy + fl[:, 1]
                inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)  # False for NaN and ±inf
            X, Y = np.where(inside, X, 0.0), np.where(inside, Y, 0.0)
            x0, y0 = np.floor(X), np.floor(Y)
            wx, wy = X - x0, Y - y0
            x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
            need = {(0, 0): np.ones(P, bool), (0, 1): wx != 0, (1, 0): wy != 0, (1, 1): (wx != 0) & (wy != 0)}
            ok &= inside
            taps_a, taps_g = {}, {}
            for (dy, dx), nd in need.items():
                q = np.where(nd, (y0 + dy) * W + (x0 + dx), 0)  # a tap of weight 0 is neither read nor required
                assert (q >= 0).all() and (q < P).all()
                ok &= ~nd | v[f1][q]
                taps_a[dy, dx] = np.where(nd, a[f1][q], 0.0)
                taps_g[dy, dx] = None if g is None else np.where(nd, g[f1][q], 0.0)
            a1 = _bilerp(wx, wy, *(taps_a[j] for j in ((0, 0), (0, 1), (1, 0), (1, 1))))
            g1 = None if g is None else _bilerp(wx, wy, *(taps_g[j] for j in ((0, 0), (0, 1), (1, 0), (1, 1))))
        with np.errstate(invalid="ignore", over="ignore"):
            da = (a1 - a[f0])[ok]
            out[i, :3] = [da.size, np.abs(da).sum(), (da * da).sum()]
            if g is not None:
                dg = (g1 - g[f0])[ok]
                r = da - dg
                out[i, 3:] = [np.abs(r).sum(), (r * r).sum(), np.abs(dg).sum(), (dg * dg).sum(), (da * dg).sum()]
    return out


def ref_temporal_metrics(sums, has_target=True):
    tot = sums.sum(0)
    n = tot[0]
    nan = math.nan
    if n == 0:
        return dict.fromkeys(("flicker", "flicker_rmse", "tge", "tge_rmse", "target_change", "change_corr"), nan)
    out = {"flicker": tot[1] / n, "flicker_rmse": math.sqrt(tot[2] / n), "tge": nan, "tge_rmse": nan,
           "target_change": nan, "change_corr": nan}
    if has_target:
        out.update(tge=tot[3] / n, tge_rmse=math.sqrt(tot[4] / n), target_change=tot[5] / n)
        if tot[2] > 0 and tot[6] > 0:
            out["change_corr"] = tot[7] / math.sqrt(tot[2] * tot[6])
    return out
