"""CPU restatements of rdmi_temporal_filter (include/rdmi.h "Temporal filter") and the shared inputs of
tests/test_stabilize_cpu.py and tests/test_stabilize_gpu.py.

restate(..., dt=F64) is the definition in f64.  Only what picks the taps is formed as the header prescribes, in f32:
X = (float)x + dx and Y, the in-frame test, x0 = min((int)X, W − 1) and wx = X − (float)x0 (alike in y), so that the
taps and their weights are the device's.  Everything after that — the lerp, δ, the exponent, the weights, the sums
and the quotient — is in dt; ct and cd are log₂e / (2σ²) formed in f64 and rounded to dt, the weight is exp2(−e).
restate(..., dt=F32) is the same formula in torch f32 on the CPU: no fma, libm's exp2 instead of v_exp_f32.

Tolerance of the device against the f64 restatement, at every pixel:
    |device − f64| ≤ TOL_REL · tap_range,
    tap_range = max_k |d_k − d0| over the neighbours used (f64), floored at 2⁻²⁰ · max(|d0|, |taps of those neighbours|).
F32_RATIO is the worst |f32 restatement − f64| / tap_range over every GPU case × {f16, f32}, measured once on the CPU
and re-measured by test_stabilize_cpu.py::test_f32_ratio_behind_the_gpu_tolerance; TOL_REL = 4 · F32_RATIO, the
project's margin covering the device's v_exp_f32 and its contraction."""
import math

import torch

F16, F32, F64 = torch.float16, torch.float32, torch.float64
LOG2E = 1.4426950408889634074

# (N, H, W, R)
GPU_CASES = [
    (1, 8, 8, 1),       # identity: no neighbour exists
    (2, 5, 7, 1),       # every frame lacks a neighbour; borders everywhere
    (5, 9, 70, 2),      # three tiles across, with a remainder
    (7, 19, 33, 3),     # the widest radius, N = 2R + 1
    (4, 40, 130, 2),    # several tiles both ways, with remainders
]
SIGMA_TIME, SIGMA_DEPTH = 1.0, 0.05
NOISE = 0.02

# Measured over the 10 variants: 3.371e-3, on (5, 9, 70, 2) with f32 depth, at a pixel whose only used neighbour lies
# within 3.5e-6 of d0 (tap_range sits close to its floor there), so that the f32 roundings of d_k and of the result,
# each half an ulp of |d| ≈ 1.5, are that large a share of the spread.  Where the spread is the noise's (a few 1e-2,
# the bulk of the pixels) the ratio is a few 1e-6: see the per-case figures the CPU test prints.
F32_RATIO = 3.4e-3
TOL_REL = 4 * F32_RATIO


def slot_offset(s: int, R: int) -> int:
    """Slot s = 0 … 2R − 1 → k = −R, …, −1, +1, …, +R."""
    return s - R if s < R else s - R + 1


def slot_of(k: int, R: int) -> int:
    return k + R if k < 0 else k + R - 1


def _run(depth, flow, valid, R, sigma_time, sigma_depth, f0, n, dt):
    N, H, W = depth.shape
    n = N - f0 if n is None else n
    assert tuple(flow.shape) == (2 * R, n, H, W, 2) and flow.dtype == F32
    D = depth.to(dt)  # f16 and f32 widen exactly
    D64 = depth.to(F64)
    ct = torch.tensor(LOG2E / (2.0 * sigma_time * sigma_time), dtype=F64).to(dt)
    cd = torch.tensor(LOG2E / (2.0 * sigma_depth * sigma_depth), dtype=F64).to(dt)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    out = torch.empty((n, H, W), dtype=dt)
    rng = torch.empty((n, H, W), dtype=F64)
    for r in range(n):
        i = f0 + r
        d0, d064 = D[i], D64[i]
        fin0 = torch.isfinite(d0)
        acc = torch.zeros((H, W), dtype=dt)
        wsum = torch.zeros((H, W), dtype=dt)
        spread = torch.zeros((H, W), dtype=F64)
        mag = torch.where(fin0, d064.abs(), torch.zeros_like(d064))
        for s in range(2 * R):
            k = slot_offset(s, R)
            j = i + k
            if not 0 <= j < N:
                continue
            u = flow[s, r]
            X, Y = xs + u[..., 0], ys + u[..., 1]  # f32, one rounding each
            ok = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)  # a NaN fails
            if valid is not None:
                ok = ok & (valid[s, r] != 0)
            Xs, Ys = torch.where(ok, X, torch.zeros_like(X)), torch.where(ok, Y, torch.zeros_like(Y))
            x0, y0 = Xs.to(torch.int64).clamp(max=W - 1), Ys.to(torch.int64).clamp(max=H - 1)  # (int): truncation
            x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
            wx, wy = (Xs - x0.to(F32)).to(dt), (Ys - y0.to(F32)).to(dt)  # f32 differences, then widened

            def lerp(T):
                a00, a01, a10, a11 = T[y0, x0], T[y0, x1], T[y1, x0], T[y1, x1]
                wx_, wy_ = wx.to(T.dtype), wy.to(T.dtype)
                t0 = a00 + wx_ * (a01 - a00)
                t1 = a10 + wx_ * (a11 - a10)
                return t0 + wy_ * (t1 - t0), torch.stack([a00, a01, a10, a11]).abs().amax(0)

            dk, _ = lerp(D[j])
            ok = ok & torch.isfinite(dk) & fin0
            dl = torch.where(ok, dk - d0, torch.zeros_like(dk))
            e = (dl * dl) * cd + float(k * k) * ct
            w = torch.where(ok, torch.exp2(-e), torch.zeros_like(e))
            acc = acc + w * dl
            wsum = wsum + w
            dk64, tmag = lerp(D64[j])
            zero = torch.zeros_like(spread)
            spread = torch.maximum(spread, torch.where(ok, (dk64 - d064).abs(), zero))
            mag = torch.maximum(mag, torch.where(ok, tmag, zero))
        out[r] = torch.where(fin0, d0 + acc / (1.0 + wsum), d0)
        rng[r] = torch.maximum(spread, 2.0 ** -20 * mag)
    return out, rng


def restate(depth, flow, valid, R, sigma_time=SIGMA_TIME, sigma_depth=SIGMA_DEPTH, f0=0, n=None, dt=F64):
    """depth [N, H, W] (f16 / f32), flow f32 [2R, n, H, W, 2], valid uint8 [2R, n, H, W] or None → [n, H, W] in dt."""
    return _run(depth, flow, valid, R, sigma_time, sigma_depth, f0, n, dt)[0]


def restate_and_range(depth, flow, valid, R, sigma_time=SIGMA_TIME, sigma_depth=SIGMA_DEPTH, f0=0, n=None):
    """(f64 restatement, tap_range) in one pass."""
    return _run(depth, flow, valid, R, sigma_time, sigma_depth, f0, n, F64)


def tap_range(depth, flow, valid, R, f0=0, n=None) -> torch.Tensor:
    """f64 [n, H, W]: max_k |d_k − d0| over the neighbours used, floored at 2⁻²⁰ · max(|d0|, |their taps|)."""
    return _run(depth, flow, valid, R, SIGMA_TIME, SIGMA_DEPTH, f0, n, F64)[1]


_INPUTS = {}


def nan_pixel(ci: int):
    """(frame, y, x) of the case's NaN depth pixel; its reader is the same pixel of the frame before (the frame
    after, for frame 0) through a planted zero flow."""
    N, H, W, R = GPU_CASES[ci]
    return (1 if N > 1 else 0), H // 2, W // 2


def gpu_inputs(ci: int, dtype):
    """Deterministic inputs of GPU case ci → (depth [N, H, W] of dtype, flow f32 [2R, N, H, W, 2], valid uint8
    [2R, N, H, W]).  Depth: a smooth field in about [1, 2] that drifts from frame to frame, plus noise of σ = 0.02,
    with one NaN pixel.  Flow: uniform in ±3 px (so border pixels leave the frame), valid: 1 with probability 0.9;
    and in slot k = +1 of frame 0 (every case with N ≥ 2 has that neighbour) the planted lanes
      (0, 0): the exact integer flow (1, 1);          (0, 2): a target outside the frame;
      (0, 3): a NaN component;                        (0, 4): valid = 0;
      (1, W − 3): X = W − 1 exactly (x1 clamped, wx = 0);   (H − 3, 1): Y = H − 1 exactly;
      (H/2, W/2): zero flow onto the NaN pixel of frame 1.
    Cached: every test shares one copy and leaves it unchanged."""
    key = (ci, dtype)
    if key not in _INPUTS:
        N, H, W, R = GPU_CASES[ci]
        g = torch.Generator().manual_seed(5200 + ci)
        ys = torch.arange(H, dtype=F64)[None, :, None] / 16
        xs = torch.arange(W, dtype=F64)[None, None, :] / 16
        t = torch.arange(N, dtype=F64)[:, None, None]
        smooth = 1.5 + 0.3 * torch.sin(xs * 1.3 + 0.2 * t) * torch.cos(ys * 0.9 - 0.1 * t) + 0.15 * torch.sin(xs + ys)
        depth = smooth + NOISE * torch.randn((N, H, W), generator=g, dtype=F64)
        flow = ((torch.rand((2 * R, N, H, W, 2), generator=g, dtype=F64) * 2 - 1) * 3).to(F32)
        valid = (torch.rand((2 * R, N, H, W), generator=g, dtype=F64) < 0.9).to(torch.uint8)
        fn, yn, xn = nan_pixel(ci)
        depth[fn, yn, xn] = math.nan
        if N > 1:
            s = slot_of(1, R)
            for (y, x), (dx, dy), ok in (((0, 0), (1.0, 1.0), 1), ((0, 2), (-10.0, 0.0), 1),
                                         ((0, 3), (math.nan, 0.5), 1), ((0, 4), (0.5, 0.5), 0),
                                         ((1, W - 3), (2.0, 0.25), 1), ((H - 3, 1), (0.5, 2.0), 1),
                                         ((yn, xn), (0.0, 0.0), 1)):
                flow[s, 0, y, x, 0], flow[s, 0, y, x, 1] = dx, dy
                valid[s, 0, y, x] = ok
        _INPUTS[key] = (depth.to(dtype).contiguous(), flow.contiguous(), valid.contiguous())
    return _INPUTS[key]


def all_gpu_variants():
    return [(ci, dt) for ci in range(len(GPU_CASES)) for dt in (F16, F32)]


_REFS = {}


def gpu_reference(ci: int, dtype):
    """(f64 restatement, tap_range) of a GPU case, computed once."""
    key = (ci, dtype)
    if key not in _REFS:
        depth, flow, valid = gpu_inputs(ci, dtype)
        _REFS[key] = _run(depth, flow, valid, GPU_CASES[ci][3], SIGMA_TIME, SIGMA_DEPTH, 0, None, F64)
    return _REFS[key]


def ratio(got: torch.Tensor, ref: torch.Tensor, rng: torch.Tensor) -> float:
    """The worst |got − ref| / rng over the pixels whose reference is finite; the others must agree in kind."""
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isfinite(got), fin)
    return ((got.to(F64) - ref).abs()[fin] / rng[fin]).max().item()


def f32_ratio(ci: int, dtype) -> float:
    depth, flow, valid = gpu_inputs(ci, dtype)
    ref, rng = gpu_reference(ci, dtype)
    return ratio(restate(depth, flow, valid, GPU_CASES[ci][3], dt=F32), ref, rng)


def variance_ratio(R: int, sigma_time: float) -> float:
    """(1 + Σ g_k²) / (1 + Σ g_k)², g_k = exp(−k²/2σt²) over k = ±1 … ±R: the error variance left by the filter on
    i.i.d. noise when the range term is switched off."""
    g = [math.exp(-k * k / (2.0 * sigma_time ** 2)) for k in range(1, R + 1)] * 2
    return (1.0 + sum(v * v for v in g)) / (1.0 + sum(g)) ** 2
