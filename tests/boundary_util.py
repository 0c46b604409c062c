"""numpy f64 restatement of rollingdepth_amd.metrics.boundary_metrics (rdmi.h "Depth boundaries") and the seeded
inputs that tests/test_boundary_cpu.py and tests/test_boundary_gpu.py share.

The restatement follows the definition with whole-array shifted comparisons, one threshold and one direction at a
time: no levels, no histograms, nothing of the kernel's one-pass scheme.  It takes the scale and shift as inputs and
reads the dtype-rounded operands as f64 and the float32-rounded lo / hi, as the device does.  Where the device
rounds once (d = fma(s, p, t)) numpy rounds twice, and the device's exp may differ from numpy's in the last bits:
that is a relative 1e-16 of an aligned value, and it can change a count only where a(j) lies that close to τ·a(i).
restate() also counts the pairs within a relative 1e-9 of any threshold — a wide guard band around those 1e-16, not a
measurement — and the CPU test requires 0 of them for every GPU case that aligns or leaves depth space; with
align="none" in depth space a = p exactly and there is nothing to guard.
"""
import functools
import math

import numpy as np
import torch

from tests import temporal_util as T

F16, F32 = torch.float16, torch.float32
DEFAULT_THRESHOLDS = np.linspace(1.05, 1.25, 10)
LO = 1e-3
TIE = 1e-9
DIRS = ("R", "L", "D", "U")


# ----------------------------------------------------------------------------- the restatement
def aligned(p, s, t, space, clip):
    """a = clamp(φ⁻¹(s·p + t)) of one frame [H, W]; fmax / fmin as the device's clamp."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = T.from_space(s * p + t, space)
    if clip is not None:
        a = np.fmin(np.fmax(a, clip[0]), clip[1])
    return a


def valid_pixels(p, g, m, a, s, t, space, lo=LO, hi=math.inf):
    """[H, W] bool: the rule of depth_errors_k (mask, finiteness, lo < g < hi, g > 0 outside depth space, a frame with
    a fit) and a finite and > 0."""
    if math.isnan(s) or math.isnan(t):
        return np.zeros(p.shape, bool)
    with np.errstate(invalid="ignore"):
        v = np.isfinite(p) & np.isfinite(g) & (g > float(np.float32(lo))) & (g < float(np.float32(hi)))
        if space != "depth":
            v &= g > 0
        v &= np.isfinite(a) & (a > 0)
    return v if m is None else v & (m != 0)


def _shift(x, k):
    """The neighbour of every pixel in direction k and whether it exists: (x_j [H, W], inside [H, W])."""
    out = np.zeros_like(x)
    inside = np.zeros(x.shape, bool)
    if k == "R":
        out[:, :-1], inside[:, :-1] = x[:, 1:], True
    elif k == "L":
        out[:, 1:], inside[:, 1:] = x[:, :-1], True
    elif k == "D":
        out[:-1, :], inside[:-1, :] = x[1:, :], True
    else:
        out[1:, :], inside[1:, :] = x[:-1, :], True
    return out, inside


def edge_maps(d, v, tau):
    """[4, H, W] bool: pixel i has an edge of map d in direction k at τ iff its neighbour j there is a valid pixel
    like i and d(j) > τ·d(i)."""
    out = []
    for k in DIRS:
        dj, inside = _shift(d, k)
        vj, _ = _shift(v, k)
        with np.errstate(invalid="ignore", over="ignore"):
            out.append(v & vj & inside & (dj > tau * d))
    return np.stack(out)


def restate(p, g, m, s, t, thresholds=DEFAULT_THRESHOLDS, space="depth", clip=None, lo=LO, hi=math.inf,
            edge_index=None):
    """p, g [N, H, W] f64 (the dtype-rounded operands), m [N, H, W] or None, s, t [N] → counts int64 [N, M, 4, 3]
    (TP, NP, NG), pairs int64 [N, 2], edges uint8 [N, H, W] for thresholds[edge_index] (None without one), and the
    number of near-tie pairs of a."""
    N, H, W = p.shape
    M = len(thresholds)
    counts = np.zeros((N, M, 4, 3), np.int64)
    pairs = np.zeros((N, 2), np.int64)
    edges = None if edge_index is None else np.zeros((N, H, W), np.uint8)
    ties = 0
    for f in range(N):
        a = aligned(p[f], s[f], t[f], space, clip)
        v = valid_pixels(p[f], g[f], None if m is None else m[f], a, s[f], t[f], space, lo, hi)
        pairs[f] = [(v[:, :-1] & v[:, 1:]).sum(), (v[:-1, :] & v[1:, :]).sum()]
        a0, g0 = np.where(v, a, 1.0), np.where(v, g[f], 1.0)
        for mi, tau in enumerate(thresholds):
            ea, eg = edge_maps(a0, v, tau), edge_maps(g0, v, tau)
            counts[f, mi, :, 0] = (ea & eg).sum((1, 2))
            counts[f, mi, :, 1] = ea.sum((1, 2))
            counts[f, mi, :, 2] = eg.sum((1, 2))
            if mi == edge_index:
                for k in range(4):
                    edges[f] |= (ea[k].astype(np.uint8) << k) | (eg[k].astype(np.uint8) << (4 + k))
            for k in DIRS:
                aj, inside = _shift(a0, k)
                vj, _ = _shift(v, k)
                with np.errstate(over="ignore", invalid="ignore"):
                    ties += int((v & vj & inside & (np.abs(aj - tau * a0) <= TIE * tau * a0)).sum())
    return counts, pairs, edges, ties


def pool(counts, pairs, thresholds):
    """The pooled floats of the definition from the integer counts, in f64: precision(τ) = ¼ Σ_k TP_k / max(NP_k, 1),
    recall(τ) = ¼ Σ_k TP_k / max(NG_k, 1), f1(τ) = 2PR / (P + R) or 0, the scalars weighted by τ_m / Σ τ; all NaN
    without a valid pair."""
    M = len(thresholds)
    tot = [[[int(counts[:, m, k, c].sum()) for c in range(3)] for k in range(4)] for m in range(M)]
    n_pairs = int(pairs.sum())
    nan = math.nan
    if n_pairs == 0:
        return dict(f1=nan, precision=nan, recall=nan, f1_per_threshold=[nan] * M, precision_per_threshold=[nan] * M,
                    recall_per_threshold=[nan] * M, n_pairs=0)
    tau = [float(x) for x in thresholds]
    tau_sum = 0.0
    for x in tau:
        tau_sum = tau_sum + x
    P, R, F = [], [], []
    for m in range(M):
        p = ((tot[m][0][0] / max(tot[m][0][1], 1) + tot[m][1][0] / max(tot[m][1][1], 1))
             + tot[m][2][0] / max(tot[m][2][1], 1)) + tot[m][3][0] / max(tot[m][3][1], 1)
        r = ((tot[m][0][0] / max(tot[m][0][2], 1) + tot[m][1][0] / max(tot[m][1][2], 1))
             + tot[m][2][0] / max(tot[m][2][2], 1)) + tot[m][3][0] / max(tot[m][3][2], 1)
        p, r = 0.25 * p, 0.25 * r
        P.append(p)
        R.append(r)
        F.append(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0)
    w = [x / tau_sum for x in tau]
    acc = lambda vals: functools.reduce(lambda a, b: a + b, (w[m] * vals[m] for m in range(M)), 0.0)
    return dict(f1=acc(F), precision=acc(P), recall=acc(R), f1_per_threshold=F, precision_per_threshold=P,
                recall_per_threshold=R, n_pairs=n_pairs)


def f64(t):
    return t.detach().cpu().double().numpy()


def fit(p, g, m, align, space, lo=LO, hi=math.inf):
    """(s [N], t [N]) of the f64 restatement's least-squares fit (tests/temporal_util.py), frames as [N, H, W]."""
    N = p.shape[0]
    if align == "none":
        return np.ones(N), np.zeros(N)
    pf, gf = p.reshape(N, -1), g.reshape(N, -1)
    v = T.ref_valid(pf, gf, None if m is None else m.reshape(N, -1), lo, hi, space)
    mom, mom_abs = T.ref_moments(pf, gf, v, space)
    s, t, _ = T.ref_fit(mom, mom_abs, align)
    return s, t


# ----------------------------------------------------------------------------- inputs
# (N, H, W): the smallest shapes at which the tiling (8-pixel octets of a row, strips of 4 rows, 256 units per
# workgroup) can go wrong
SHAPES = [(1, 1, 9), (1, 9, 1), (2, 5, 7), (2, 8, 8), (3, 17, 67), (2, 33, 259), (1, 70, 131), (1, 3, 4099)]
CLIP = (0.05, 40.0)  # of the disparity cases


@functools.lru_cache(maxsize=None)
def scene(shape, seed):
    """(target depth, prediction depth) f64 [N, H, W].  The target is random axis-aligned rectangles whose depths come
    from a geometric ladder with neighbour ratios in [1.03, 1.4], times a smooth factor within ±1 %; the prediction is
    the same scene with every third rectangle moved by one pixel, times exp(0.03·noise)."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    ladder = np.cumprod(np.concatenate([[1.0], rng.uniform(1.03, 1.4, 9)]))
    ys, xs = np.arange(H)[:, None] / max(H, 2), np.arange(W)[None, :] / max(W, 2)
    gt, pr = np.empty(shape), np.empty(shape)
    for f in range(N):
        lab_g = np.full((H, W), rng.integers(0, 10))
        lab_p = lab_g.copy()
        for i in range(int(min(40, max(4, H * W // 24)))):
            h, w = rng.integers(1, max(2, H // 2 + 1)), rng.integers(1, max(2, W // 3 + 1))
            y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
            level = rng.integers(0, 10)
            lab_g[y:y + h, x:x + w] = level
            dy, dx = ((0, 0), (0, 1), (1, 0), (0, -1), (-1, 0))[rng.integers(1, 5) if i % 3 == 0 else 0]
            y2, x2 = min(max(y + dy, 0), H - h), min(max(x + dx, 0), W - w)
            lab_p[y2:y2 + h, x2:x2 + w] = level
        smooth = 1.0 + 0.01 * np.sin(2 * math.pi * (xs + 0.7 * ys) + f)
        gt[f] = ladder[lab_g] * smooth
        pr[f] = ladder[lab_p] * smooth * np.exp(0.03 * rng.standard_normal((H, W)))
    return gt, pr


# One dict per GPU case: shape index, seed, pred / target dtype, mask, non-finite sprinkles, a fully masked frame,
# align, space, M.  Every shape runs plain (f32, align none: exact whatever the ties) and in further variants; the
# options are spread over the shapes, not multiplied.
def _case(si, seed, pd=F32, td=F32, mask=False, bad=False, dead=None, align="none", space="depth", M=10):
    return dict(si=si, seed=seed, pd=pd, td=td, mask=mask, bad=bad, dead=dead, align=align, space=space, M=M)


CASES = [
    _case(0, 24), _case(0, 24, pd=F16, align="video"), _case(0, 31, mask=True, M=1),
    _case(1, 2), _case(1, 2, td=F16, align="frame", M=16), _case(1, 2, space="log", align="video"),
    _case(2, 1), _case(2, 1, pd=F16, td=F16, mask=True, bad=True), _case(2, 3, space="disparity", align="video"),
    _case(3, 1), _case(3, 2, mask=True, align="frame", M=16), _case(3, 3, pd=F16, space="log", align="frame", M=1),
    _case(4, 1), _case(4, 2, pd=F16, mask=True, bad=True, dead=1, align="frame"),
    _case(4, 3, td=F16, space="disparity", align="frame", mask=True),
    _case(5, 1), _case(5, 2, pd=F16, td=F16, bad=True, align="video", M=16), _case(5, 3, mask=True, space="log", align="video"),
    _case(6, 1), _case(6, 2, pd=F16, mask=True, bad=True, align="video"), _case(6, 3, space="disparity", align="video", M=1),
    _case(7, 1), _case(7, 2, td=F16, mask=True, align="video"), _case(7, 3, pd=F16, bad=True, space="log", align="frame", M=16),
]
DT = {F16: "f16", F32: "f32"}
IDS = ["x".join(map(str, SHAPES[c["si"]])) + f"-{DT[c['pd']]}-{DT[c['td']]}-{'mask' if c['mask'] else 'nomask'}"
       f"{'-nonfinite' if c['bad'] else ''}{'-deadframe' if c['dead'] is not None else ''}-{c['align']}-{c['space']}"
       f"-M{c['M']}" for c in CASES]


def thresholds_of(M):
    """M = 10: the default; 1: its middle value; 16: a finer ladder over a wider range."""
    return {10: DEFAULT_THRESHOLDS, 1: DEFAULT_THRESHOLDS[5:6], 16: np.linspace(1.02, 1.32, 16)}[M]


@functools.lru_cache(maxsize=None)
def case_inputs(ci):
    """Host tensors of GPU case ci → (pred, target, mask or None, kwargs of boundary_metrics).  In log and disparity
    space the prediction is an affine function of φ(depth), so that the fit has something to find; with an alignment
    in depth space it is an affine function of the depth."""
    c = CASES[ci]
    shape = SHAPES[c["si"]]
    gt, pr = scene(shape, c["seed"])
    rng = np.random.default_rng(1000 + ci)
    if c["space"] == "log":
        p = 0.5 + 2.0 * np.log(pr)
    elif c["space"] == "disparity":
        p = 0.5 + 2.0 / pr
    elif c["align"] != "none":
        p = 0.25 + 1.5 * pr
    else:
        p = pr.copy()
    g = gt.copy()
    if c["bad"]:
        for arr in (p, g):
            hit = rng.random(shape) < 0.02
            arr[hit] = rng.choice([np.nan, np.inf, -np.inf], size=int(hit.sum()))
    m = None
    if c["mask"]:
        m = rng.random(shape) < 0.8
        if c["dead"] is not None:
            m[c["dead"]] = False
    kw = dict(align=c["align"], space=c["space"], clip=CLIP if c["space"] == "disparity" else None,
              thresholds=[float(x) for x in thresholds_of(c["M"])])
    return (torch.from_numpy(p).to(c["pd"]), torch.from_numpy(g).to(c["td"]),
            None if m is None else torch.from_numpy(m), kw)


def restate_case(ci, s=None, t=None, edge_index=None):
    """The restatement of GPU case ci with the given scale and shift (default: the f64 restatement's own fit)."""
    pred, target, mask, kw = case_inputs(ci)
    p, g = f64(pred), f64(target)
    m = None if mask is None else mask.numpy()
    if s is None:
        s, t = fit(p, g, m, kw["align"], kw["space"])
    return restate(p, g, m, s, t, kw["thresholds"], kw["space"], kw["clip"], edge_index=edge_index), (s, t)
