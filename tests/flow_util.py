"""Torch restatement of the optical-flow specification (include/rdmi.h "Optical flow"), operation by
operation, on the CPU, and the seeded inputs the CPU and GPU tests share.

Every function takes the arithmetic dtype `dt`: torch.float64 is the reference, torch.float32 the same operations
in the device's precision (torch's summation order, no fma) — the distance between the two runs is the measure of
what f32 does to this algorithm, from which tests/test_flow_gpu.py takes its tolerance.  The window sums add the
taps one by one in row-major order; a tap outside the image adds an exact zero.
"""
import functools
import math

import torch

F16, F32, F64, U8 = torch.float16, torch.float32, torch.float64, torch.uint8
DEFAULTS = dict(radius=5, iterations=3, damping=0.01)
FB_TOL = (0.01, 0.5)
MAX_LEVELS = 5
# the largest difference between the restatement in f64 and in f32 over GPU_CASES × GPU_DTYPES, in pixels (measured:
# 9.72e-5, on 33 × 31 at r = 1 from uint8 frames; tests/test_flow_cpu.py re-measures it), and the device's allowance: 4 ×
F32_SPREAD = 9.8e-5
TOL_PX = 4 * F32_SPREAD


# ----------------------------------------------------------------------------- the specification
def level_rule(H, W, r=5, levels=None):
    n, h, w = 1, (H + 1) // 2, (W + 1) // 2
    while n < MAX_LEVELS and min(h, w) >= 4 * (2 * r + 1):
        n, h, w = n + 1, (h + 1) // 2, (w + 1) // 2
    return n if levels is None else max(1, min(levels, n))


def luma(frames, dt):
    """[N, 3, H, W] f16 / f32 or uint8 [N, H, W, 3] → [N, H, W] in dt: the stored values widened exactly, then
    (0.299 R + 0.587 G) + 0.114 B with the f32 constants."""
    x = frames.permute(0, 3, 1, 2) if frames.dtype == U8 else frames
    x = x.to(dt)
    c = [torch.tensor(v, dtype=F32).to(dt) for v in (0.299, 0.587, 0.114)]
    return (c[0] * x[:, 0] + c[1] * x[:, 1]) + c[2] * x[:, 2]


def down(I):
    """[..., H, W] → [..., ⌈H/2⌉, ⌈W/2⌉]: ¼·((a + b) + (c + d)) of the 2 × 2 block at (2y, 2x), indices clamped."""
    H, W = I.shape[-2:]
    y0 = torch.arange(0, H, 2)
    x0 = torch.arange(0, W, 2)
    y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
    a, b = I[..., y0, :][..., x0], I[..., y0, :][..., x1]
    c, d = I[..., y1, :][..., x0], I[..., y1, :][..., x1]
    return 0.25 * ((a + b) + (c + d))


def pyramid(Y, levels):
    out = [Y]
    for _ in range(levels - 1):
        out.append(down(out[-1]))
    return out


def _bilerp(v00, v01, v10, v11, wx, wy):
    return (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11)


def sample(I, X, Y):
    """Bilinear sample of I [H, W] (or [H, W, C]) at coordinates already inside [0, W − 1] × [0, H − 1]."""
    H, W = I.shape[:2]
    x0, y0 = X.floor(), Y.floor()
    wx, wy = X - x0, Y - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    if I.dim() == 3:
        wx, wy = wx[..., None], wy[..., None]
    return _bilerp(I[y0, x0], I[y0, x1], I[y1, x0], I[y1, x1], wx, wy)


def upsample_flow(coarse, H, W):
    """Coarse flow [Hc, Wc, 2] → the start of the next finer level [H, W, 2]: 2 · the bilinear sample at
    ((x + ½)/2 − ½, (y + ½)/2 − ½), clamped."""
    dt = coarse.dtype
    Hc, Wc = coarse.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    X = ((xs + 0.5) * 0.5 - 0.5).clamp(0, Wc - 1)
    Y = ((ys + 0.5) * 0.5 - 0.5).clamp(0, Hc - 1)
    return 2 * sample(coarse, X, Y)


def lk_level(I0, I1, u, r, iterations, damping):
    """One level: I0, I1 [H, W], u [H, W, 2] the start (zeros on the coarsest level) → the level's flow."""
    dt = I0.dtype
    H, W = I0.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xi = torch.arange(W)
    yi = torch.arange(H)
    Ix = 0.5 * (I0[:, (xi + 1).clamp(max=W - 1)] - I0[:, (xi - 1).clamp(min=0)])
    Iy = 0.5 * (I0[(yi + 1).clamp(max=H - 1), :] - I0[(yi - 1).clamp(min=0), :])
    taps = []  # row-major: j outer
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            qy, qx = ys + j, xs + i
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qyc, qxc = qy.clamp(0, H - 1), qx.clamp(0, W - 1)
            zero = torch.zeros((), dtype=dt)
            taps.append((qy.to(dt), qx.to(dt), inside, torch.where(inside, Ix[qyc, qxc], zero),
                         torch.where(inside, Iy[qyc, qxc], zero), I0[qyc, qxc]))
    axx = torch.zeros((H, W), dtype=dt)
    axy, ayy = axx.clone(), axx.clone()
    for _, _, _, gx, gy, _ in taps:
        axx = axx + gx * gx
        axy = axy + gx * gy
        ayy = ayy + gy * gy
    lam = damping * (0.5 * (axx + ayy)) + 1e-12
    a11, a22 = axx + lam, ayy + lam
    det = a11 * a22 - axy * axy
    ux, uy = u[..., 0].clone(), u[..., 1].clone()
    for _ in range(iterations):
        bx = torch.zeros((H, W), dtype=dt)
        by = bx.clone()
        for qy, qx, inside, gx, gy, i0 in taps:
            X = (qx + ux).clamp(0, W - 1)
            Y = (qy + uy).clamp(0, H - 1)
            d = sample(I1, X, Y) - i0
            bx = bx + gx * d  # gx, gy are exact zeros outside the image
            by = by + gy * d
        dux = -(a22 * bx - axy * by) / det
        duy = -(a11 * by - axy * bx) / det
        n = (dux * dux + duy * duy).sqrt()
        long_ = n > 1
        dux = torch.where(long_, dux / n, dux)
        duy = torch.where(long_, duy / n, duy)
        ux, uy = ux + dux, uy + duy
    return torch.stack([ux, uy], -1)


def flow_pair(P0, P1, r=5, iterations=3, damping=0.01):
    """P0, P1: the two frames' pyramids (lists of [H_l, W_l], fine to coarse) → the flow [H, W, 2] from 0 to 1."""
    u = None
    for I0, I1 in zip(reversed(P0), reversed(P1)):
        H, W = I0.shape
        start = torch.zeros((H, W, 2), dtype=I0.dtype) if u is None else upsample_flow(u, H, W)
        u = lk_level(I0, I1, start, r, iterations, damping)
    return u


def fb_check(uf, ub, alpha=FB_TOL[0], beta=FB_TOL[1]):
    """→ (valid bool [H, W], margin [H, W] = lhs − rhs of the inequality; +inf where the target leaves the frame)."""
    dt = uf.dtype
    H, W = uf.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    X, Y = xs + uf[..., 0], ys + uf[..., 1]
    inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    b = sample(ub, torch.where(inside, X, torch.zeros_like(X)), torch.where(inside, Y, torch.zeros_like(Y)))
    sx, sy = uf[..., 0] + b[..., 0], uf[..., 1] + b[..., 1]
    lhs = sx * sx + sy * sy
    rhs = alpha * ((uf[..., 0] * uf[..., 0] + uf[..., 1] * uf[..., 1]) + (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1])) + beta
    margin = torch.where(inside, lhs - rhs, torch.full_like(lhs, math.inf))
    return inside & (lhs <= rhs), margin


def estimate(frames, frame_step=1, levels=None, r=5, iterations=3, damping=0.01, fb_tol=FB_TOL, dt=F64,
             backward=True):
    """The whole chain on a video → (flow [N − k, H, W, 2], flow_backward, valid bool [N − k, H, W], margin), in dt.
    levels: None for the rule; a number is taken as given."""
    Y = luma(frames, dt)
    N, H, W = Y.shape
    levels = level_rule(H, W, r) if levels is None else levels
    pyr = pyramid(Y, levels)
    fw, bw, va, ma = [], [], [], []
    for i in range(N - frame_step):
        P0 = [p[i] for p in pyr]
        P1 = [p[i + frame_step] for p in pyr]
        fw.append(flow_pair(P0, P1, r, iterations, damping))
        if backward:
            bw.append(flow_pair(P1, P0, r, iterations, damping))
            v, m = fb_check(fw[-1], bw[-1], *fb_tol)
            va.append(v)
            ma.append(m)
    if not backward:
        return torch.stack(fw), None, None, None
    return torch.stack(fw), torch.stack(bw), torch.stack(va), torch.stack(ma)


# ----------------------------------------------------------------------------- the synthetic texture
@functools.lru_cache(maxsize=None)
def waves(scale=1.0):
    """24 plane waves: fx, fy uniform in ±0.6·scale rad/px, φ in [0, 2π), a in [0.5, 1.5); f64 rand(24) calls in the
    order fx, fy, φ, a from Generator().manual_seed(1)."""
    g = torch.Generator().manual_seed(1)
    fx = (torch.rand(24, generator=g, dtype=F64) * 2 - 1) * 0.6 * scale
    fy = (torch.rand(24, generator=g, dtype=F64) * 2 - 1) * 0.6 * scale
    ph = torch.rand(24, generator=g, dtype=F64) * 2 * math.pi
    a = torch.rand(24, generator=g, dtype=F64) + 0.5
    return fx, fy, ph, a


def texture(X, Y, scale=1.0):
    """Σ aᵢ·sin(fxᵢ·X + fyᵢ·Y + φᵢ) / 24 at f64 coordinates."""
    fx, fy, ph, a = waves(scale)
    return (a * torch.sin(X[..., None] * fx + Y[..., None] * fy + ph)).sum(-1) / 24


def coords(H, W, d=(0.0, 0.0), z=1.0, n=1):
    """Frame n's sampling coordinates ((X − c)·zⁿ + c − n·d), c the image centre: frame 0 is the texture itself."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    cx, cy = (W - 1) / 2, (H - 1) / 2
    zn = z ** n
    return (xs - cx) * zn + cx - n * d[0], (ys - cy) * zn + cy - n * d[1]


def true_flow(H, W, d, z=1.0):
    """u(p) = (p − c + d)/z + c − p, [H, W, 2] f64, from frame 0 to frame 1."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return torch.stack([(xs - cx + d[0]) / z + cx - xs, (ys - cy + d[1]) / z + cy - ys], -1)


GAINS = (1.0, 0.8, 0.6)  # the texture's gain per RGB channel


@functools.lru_cache(maxsize=None)
def video(N, H, W, d=(1.5, 1.0), z=1 / 1.03, dtype=F32):
    """N frames of the moving texture as the estimator's input: [N, 3, H, W] in about [−1, 1] for f32 / f16 (rounded
    to the dtype), uint8 [N, H, W, 3] as 127.5 + 100·gain·texture rounded."""
    tex = torch.stack([texture(*coords(H, W, d, z, n)) for n in range(N)])  # [N, H, W], |·| < 1.5
    rgb = torch.stack([g * tex for g in GAINS], 1)
    if dtype == U8:
        return (127.5 + 100 * rgb).round().clamp(0, 255).to(U8).permute(0, 2, 3, 1).contiguous()
    return rgb.to(dtype)


ACCURACY_CASES = [  # d, z, (mean, max) EPE required on the interior — the issue's table
    ((2.5, -1.75), 1.0, (0.05, 0.25)),
    ((5.25, 3.5), 1.0, (0.05, 0.25)),
    ((1.5, 1.0), 1 / 1.03, (0.1, 0.5)),
]
ACC_SHAPE, ACC_LEVELS, MARGIN = (96, 128), 3, 12


@functools.lru_cache(maxsize=None)
def accuracy_run(ci, iterations=3, dt=F64):
    """The restatement on accuracy case ci (the f32 RGB frames of `video`), three levels given outright →
    (flow, flow_backward, valid, margin, true flow)."""
    d, z, _ = ACCURACY_CASES[ci]
    H, W = ACC_SHAPE
    out = estimate(video(2, H, W, d, z, F32), 1, ACC_LEVELS, iterations=iterations, dt=dt)
    return out + (true_flow(H, W, d, z),)


def interior(t, m=MARGIN):
    return t[..., m:-m, m:-m] if t.dim() == 2 or t.shape[-1] != 2 else t[..., m:-m, m:-m, :]


def epe(u, truth):
    return (u.double() - truth).pow(2).sum(-1).sqrt()


# GPU cases: (N, H, W, frame_step, radius) — the issue's table; radii 1 and 7 on the second shape, 5 elsewhere
GPU_CASES = [(2, 7, 9, 1, 5), (2, 33, 31, 1, 1), (2, 33, 31, 1, 7), (3, 37, 45, 1, 5), (5, 64, 48, 2, 5),
             (2, 96, 128, 1, 5)]
GPU_DTYPES = (F32, F16, U8)
DT_NAME = {F32: "f32", F16: "f16", U8: "u8"}


def gpu_video(case, dtype):
    N, H, W, k, r = case
    if (H, W) == ACC_SHAPE:
        return video(N, H, W, ACCURACY_CASES[0][0], 1.0, dtype)
    return video(N, H, W, (0.75, 0.5), 1 / 1.02, dtype)  # per frame; frame_step 2 doubles it


@functools.lru_cache(maxsize=None)
def gpu_reference(case, dtype, dt=F64, levels=None):
    """Shared by the GPU tests, computed once: the restatement on the case's stored frames."""
    N, H, W, k, r = case
    return estimate(gpu_video(case, dtype), k, levels, r, dt=dt)


# the end-to-end video: a pure translation whose depth moves with the texture
E2E = dict(N=3, H=64, W=96, d=(2.5, -1.75))


@functools.lru_cache(maxsize=None)
def e2e_inputs():
    """frames f32 [N, 3, H, W]; pred = target f32 [N, H, W]: a smooth positive depth (the texture at ¼ of its
    frequencies, + 2) carried by the same translation."""
    N, H, W, d = E2E["N"], E2E["H"], E2E["W"], E2E["d"]
    frames = video(N, H, W, d, 1.0, F32)
    depth = torch.stack([texture(*coords(H, W, d, 1.0, n), scale=0.25) for n in range(N)]) + 2.0
    return frames, depth.float()


def undecidable(uf, ub, margin, alpha, tol):
    """Pixels of one pair whose validity a flow error of `tol` px per component can turn: the target within tol of
    the frame's border, or |lhs − rhs| within the error's effect.  uf, ub: the reference flows [H, W, 2] (f64); margin
    from fb_check.  With G the largest difference between neighbouring backward flows, the sampled u_b is off by at
    most e = tol·(1 + 2G) per component (its own error, and the sample point moving by tol in x and in y), so
    s = u_f + u_b by tol + e, lhs = |s|² by 2·|s|₁·(tol + e) + 2·(tol + e)², and rhs by α·(2·|u_f|₁·tol + 2·|u_b|₁·e)
    + 2α·(tol² + e²)."""
    H, W = uf.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    X, Y = xs + uf[..., 0], ys + uf[..., 1]
    border = (X.abs() <= tol) | ((X - (W - 1)).abs() <= tol) | (Y.abs() <= tol) | ((Y - (H - 1)).abs() <= tol)
    G = max((ub[1:] - ub[:-1]).abs().max().item() if H > 1 else 0.0, (ub[:, 1:] - ub[:, :-1]).abs().max().item())
    e = tol * (1 + 2 * G)
    inside = torch.isfinite(margin)
    b = sample(ub, X.clamp(0, W - 1), Y.clamp(0, H - 1))
    s1 = (uf + b).abs().sum(-1)
    slack = 2 * s1 * (tol + e) + 2 * (tol + e) ** 2 + alpha * (2 * uf.abs().sum(-1) * tol + 2 * b.abs().sum(-1) * e) \
        + 2 * alpha * (tol ** 2 + e ** 2)
    return border | (inside & (margin.abs() <= slack))
