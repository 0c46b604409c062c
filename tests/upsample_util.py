"""CPU restatements of rdmi_joint_bilateral_upsample (include/rdmi.h "Guided upsampling") and the shared inputs of
tests/test_upsample_cpu.py and tests/test_upsample_gpu.py.

restate(..., dt=F64) is the definition in f64: natural-base exponents e_q, w_q = exp(−(e_q − m)), Σ w·v / Σ w.  Only
the source coordinates yl, xl are formed as the header prescribes — in f32, (Y + 0.5)·(h / H) − 0.5 with each
operation rounded once — so that ⌊yl⌋ picks the device's taps; and the guide value is the device's one f32 product
element · guide_scale.  restate(..., dt=F32) is the same formula in torch f32 on the CPU: torch's vectorised sums
add the (2r)² terms in another order than the device's one-lane chain, and its exp is libm's, not v_exp_f32.

Tolerance of the device against the f64 restatement, per pixel and channel:
    |device − f64| ≤ TOL_REL · range,   range = max − min of v over the pixel's in-image taps, floored at 2⁻²⁰ · max|v|.
F32_RATIO is the worst |f32 restatement − f64| / range over every GPU case (5 shapes × {f16, f32} values × {u8, f32}
guide), measured once on the CPU and re-measured by test_upsample_cpu.py::test_f32_ratio_behind_the_gpu_tolerance;
TOL_REL = 4 · F32_RATIO, the margin covering the device's exp2 and its summation order."""
import math

import torch
import torch.nn.functional as Fn

F16, F32, F64 = torch.float16, torch.float32, torch.float64

# (N, h, w, H, W, r, C)
GPU_CASES = [
    (1, 5, 7, 5, 7, 1, 1),        # equal size: a joint bilateral filter
    (2, 9, 11, 23, 31, 2, 1),     # non-integer factors, two frames
    (1, 13, 17, 37, 45, 2, 2),    # shared weights
    (3, 7, 5, 29, 19, 3, 4),      # factor > 4, the widest window, borders everywhere
    (1, 24, 40, 70, 130, 2, 1),   # several tiles with remainders both ways
]
SIGMA_SPATIAL, SIGMA_RANGE = 1.0, 0.1
# (h, w, H, W, X0) of the edge-preservation condition
EDGE_CASES = [(9, 11, 23, 31, 13), (13, 17, 37, 45, 20), (7, 5, 29, 19, 8)]

# Measured over the 20 variants: 1.055e-5, on the equal-size case (5 × 7, r = 1, f32 values, f32 guide), where a
# border pixel's two in-image taps differ by a few 1e-3 and one f32 ulp of |v| is that large a share of the range;
# every case that upsamples stays below 1.7e-7, the (2r)²·2⁻²⁴ the error model predicts.
F32_RATIO = 1.06e-5
TOL_REL = 4 * F32_RATIO


def src_coord(out_size: int, in_size: int) -> torch.Tensor:
    """f32 [out_size]: ((i + 0.5)·(in / out)) − 0.5, every operation a separate f32 rounding."""
    scale = torch.tensor(float(in_size), dtype=F32) / torch.tensor(float(out_size), dtype=F32)
    return (torch.arange(out_size, dtype=F32) + 0.5) * scale - 0.5


def guide_values(guide_hi: torch.Tensor) -> torch.Tensor:
    """The device's G: f32 [N, 3, H, W] from uint8 [N, H, W, 3] (element · f32(1/255), one rounding) or planar f32."""
    if guide_hi.dtype == torch.uint8:
        return guide_hi.permute(0, 3, 1, 2).to(F32) * torch.tensor(1.0 / 255.0, dtype=F32)
    return guide_hi.to(F32)


def _taps(values, guide_lo, G, r):
    N, C, h, w = values.shape
    H, W = G.shape[-2:]
    yl, xl = src_coord(H, h), src_coord(W, w)
    off = torch.arange(-r + 1, r + 1)
    qy = torch.floor(yl).long()[:, None] + off[None]   # [H, T]
    qx = torch.floor(xl).long()[:, None] + off[None]   # [W, T]
    valid = ((qy >= 0) & (qy < h))[:, None, :, None] & ((qx >= 0) & (qx < w))[None, :, None, :]   # [H, W, T, T]
    iy = qy.clamp(0, h - 1)[:, None, :, None]
    ix = qx.clamp(0, w - 1)[None, :, None, :]
    return yl, xl, qy, qx, valid, iy, ix


def restate(values, guide_lo, guide_hi, r, sigma_spatial=SIGMA_SPATIAL, sigma_range=SIGMA_RANGE, dt=F64):
    """values [N, C, h, w] (f16 / f32), guide_lo f32 [N, 3, h, w], guide_hi uint8 [N, H, W, 3] or f32 [N, 3, H, W]
    → [N, C, H, W] in dt."""
    G = guide_values(guide_hi)
    yl, xl, qy, qx, valid, iy, ix = _taps(values, guide_lo, G, r)
    dy2 = (qy.to(dt) - yl.to(dt)[:, None]) ** 2
    dx2 = (qx.to(dt) - xl.to(dt)[:, None]) ** 2
    e = (dy2[:, None, :, None] + dx2[None, :, None, :]) / (2.0 * sigma_spatial * sigma_spatial)   # [H, W, T, T]
    gl = guide_lo.to(dt)[:, :, iy, ix]                                                            # [N, 3, H, W, T, T]
    dr = ((G.to(dt)[..., None, None] - gl) ** 2).sum(1)
    e = e[None] + dr / (2.0 * sigma_range * sigma_range)
    e = torch.where(valid[None], e, torch.full_like(e, math.inf))
    m = e.amin((-1, -2), keepdim=True)
    wgt = torch.exp(-(e - m))
    v = values.to(dt)[:, :, iy, ix]                                                               # [N, C, H, W, T, T]
    return (wgt[:, None] * v).sum((-1, -2)) / wgt.sum((-1, -2))[:, None]


def tap_range(values, guide_hi, r) -> torch.Tensor:
    """f64 [N, C, H, W]: max − min of the values over each pixel's in-image taps, floored at 2⁻²⁰ · max|v|."""
    G = guide_values(guide_hi)
    _, _, _, _, valid, iy, ix = _taps(values, None, G, r)
    v = values.to(F64)[:, :, iy, ix]
    hi = torch.where(valid, v, torch.full_like(v, -math.inf)).amax((-1, -2))
    lo = torch.where(valid, v, torch.full_like(v, math.inf)).amin((-1, -2))
    return (hi - lo).clamp_min(2.0 ** -20 * values.to(F64).abs().max().item())


def downsample(G: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """f32 [N, 3, H, W] → its antialiased bilinear downsample f32 [N, 3, h, w] (torch's, on the CPU)."""
    if G.shape[-2:] == (h, w):
        return G.clone()
    return Fn.interpolate(G, size=(h, w), mode="bilinear", antialias=True, align_corners=False)


_INPUTS = {}


def gpu_inputs(ci: int, u8_guide: bool, vdtype):
    """Deterministic inputs of GPU case ci → (values [N, C, h, w] in [−1, 1], guide_lo f32, guide_hi).  The guide is a
    smooth random field plus a slanted step of 0.4 in every channel, so the weights are neither all 1 nor all 0;
    guide_lo is its antialiased downsample.  Cached: every test shares one copy and leaves it unchanged."""
    key = (ci, u8_guide, vdtype)
    if key not in _INPUTS:
        N, h, w, H, W, r, C = GPU_CASES[ci]
        g = torch.Generator().manual_seed(4100 + ci)
        ys = torch.arange(H, dtype=F64)[:, None] / H
        xs = torch.arange(W, dtype=F64)[None, :] / W
        ph = torch.rand((N, 3, 4), generator=g, dtype=F64) * 2 * math.pi
        fr = 1.0 + 2.0 * torch.rand((N, 3, 2), generator=g, dtype=F64)
        p = lambda k: ph[:, :, k, None, None]
        f = lambda k: fr[:, :, k, None, None]
        field = 0.3 + 0.1 * torch.sin(2 * math.pi * f(0) * xs + p(0)) * torch.cos(2 * math.pi * f(1) * ys + p(1)) \
            + 0.05 * torch.sin(2 * math.pi * (xs + ys) * 3 + p(2))
        step = ((xs * W + 0.35 * ys * H) >= 0.45 * W + 0.1 * H).to(F64) * 0.4
        G = (field + step).clamp(0, 1)
        if u8_guide:
            guide_hi = (G * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        else:
            guide_hi = G.to(F32).contiguous()
        guide_lo = downsample(guide_values(guide_hi), h, w).contiguous()
        values = (torch.rand((N, C, h, w), generator=g, dtype=F64) * 2 - 1).to(vdtype)
        _INPUTS[key] = (values, guide_lo, guide_hi)
    return _INPUTS[key]


def all_gpu_variants():
    return [(ci, u8, vd) for ci in range(len(GPU_CASES)) for u8 in (True, False) for vd in (F16, F32)]


_REFS = {}


def gpu_reference(ci: int, u8_guide: bool, vdtype):
    """(f64 restatement, tolerance range) of a GPU case, computed once."""
    key = (ci, u8_guide, vdtype)
    if key not in _REFS:
        values, guide_lo, guide_hi = gpu_inputs(*key)
        r = GPU_CASES[ci][5]
        _REFS[key] = (restate(values, guide_lo, guide_hi, r), tap_range(values, guide_hi, r))
    return _REFS[key]


def f32_ratio(ci: int, u8_guide: bool, vdtype) -> float:
    values, guide_lo, guide_hi = gpu_inputs(ci, u8_guide, vdtype)
    ref, rng = gpu_reference(ci, u8_guide, vdtype)
    got = restate(values, guide_lo, guide_hi, GPU_CASES[ci][5], dt=F32)
    return ((got.to(F64) - ref).abs() / rng).max().item()


def edge_inputs(ei: int):
    """The edge condition's inputs → (values f32 [1, 1, h, w], guide_lo, guide_hi f32 [1, 3, H, W], side [H, W]):
    a vertical step 0 | 1 at column X0 in all three channels, its antialiased downsample, and the values 1 where
    that downsample is above 0.5 and 0 elsewhere.  side is the value every output pixel has to keep."""
    h, w, H, W, X0 = EDGE_CASES[ei]
    G = torch.zeros((1, 3, H, W), dtype=F32)
    G[..., X0:] = 1.0
    guide_lo = downsample(G, h, w).contiguous()
    values = (guide_lo[:, :1] > 0.5).to(F32).contiguous()
    side = (torch.arange(W) >= X0).to(F64)[None, :].expand(H, W)
    return values, guide_lo, G, side


def bilinear_ramp_pixels(values: torch.Tensor, H: int, W: int) -> int:
    """Pixels a plain bilinear upsample of the values leaves strictly between 0.05 and 0.95."""
    up = Fn.interpolate(values.to(F64), size=(H, W), mode="bilinear", align_corners=False)
    return int(((up > 0.05) & (up < 0.95)).sum())
