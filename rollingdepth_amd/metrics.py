"""Affine-invariant depth metrics on the device.

A diffusion depth video is defined up to one scale and one shift, so comparing it pixel by pixel with a
ground truth — or with another build, stride or dtype of the same pipeline — mostly measures that offset.
The standard protocol (the RollingDepth paper's) fits the scale and shift by least squares, per video or per
frame, and reports AbsRel and δ < 1.25ᵏ on the valid pixels:

    m = depth_metrics(pred, target)                       # one fit for the video
    m = depth_metrics(pred, target, mask, align="frame")  # one fit per frame
    m.abs_rel, m.delta1, m.scale, m.shift

All sums run in librdmi (rdmi_depth_moments / _fit / _errors, f64, fixed summation order: the same inputs
give the same bits on every call); this module only validates, reshapes and does the last few host
divisions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

ALIGN_MODES = ("video", "frame", "none")


@dataclass
class DepthMetrics:
    """Pooled over all valid pixels of all frames (each frame's sums added in frame order, ÷ n_valid)."""
    abs_rel: float   # mean |a − g| / g, a = scale·pred + shift
    sq_rel: float    # mean (a − g)² / g
    mae: float       # mean |a − g|
    rmse: float      # sqrt(mean (a − g)²)
    delta1: float    # share of pixels with max(a/g, g/a) < 1.25
    delta2: float    # … < 1.25²
    delta3: float    # … < 1.25³
    n_valid: int
    scale: torch.Tensor      # f64 [N], host
    shift: torch.Tensor      # f64 [N], host
    # f64 [N, 8], host: n, Σ|a−g|, Σ|a−g|/g, Σ(a−g)², Σ(a−g)²/g, the three δ counts
    per_frame: torch.Tensor
    frames_skipped: List[int]  # frames without a fit (NaN scale / shift): they contribute nothing


def _prepare(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], valid_range
             ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], float, float]:
    """Validate (before any device work) and bring the operands to contiguous [N, P] tensors on the device."""
    for t, name in ((pred, "pred"), (target, "target")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a tensor expected, got {type(t).__name__}")
        if t.dtype not in (torch.float16, torch.float32):
            raise TypeError(f"{name}: float16 or float32 expected, got {t.dtype}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            raise TypeError(f"mask: a tensor expected, got {type(mask).__name__}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"mask: bool or uint8 expected, got {mask.dtype}")

    def frames(t, name):
        if t.dim() == 4 and t.shape[1] == 1:
            return t.shape[0], t.shape[2], t.shape[3]
        if t.dim() == 3:
            return tuple(t.shape)
        raise ValueError(f"{name}: [N, H, W] or [N, 1, H, W] expected, got {tuple(t.shape)}")

    shape = frames(pred, "pred")
    for t, name in ((target, "target"), (mask, "mask")):
        if t is not None and frames(t, name) != shape:
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not match pred's {tuple(pred.shape)}")
    if shape[0] < 1 or shape[1] * shape[2] < 1:
        raise ValueError(f"pred: empty input {tuple(pred.shape)}")
    lo, hi = (float(v) for v in valid_range)
    if not lo < hi:
        raise ValueError(f"valid_range: lo < hi expected, got ({lo}, {hi})")

    dev = pred.device if pred.is_cuda else (target.device if target.is_cuda else torch.device("cuda", 0))

    def flat(t):
        return t.to(dev).contiguous().view(shape[0], shape[1] * shape[2])

    m = None
    if mask is not None:
        m = flat(mask)
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
    return flat(pred), flat(target), m, lo, hi


def _pool(per_frame: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> DepthMetrics:
    """Host tensors (f64 [N, 8] frame sums, f64 [N] scale / shift) → DepthMetrics."""
    tot = [0.0] * 8
    for row in per_frame.tolist():  # frame order, f64
        for k in range(8):
            tot[k] += row[k]
    n = tot[0]
    skipped = [f for f, (s, t) in enumerate(zip(scale.tolist(), shift.tolist())) if math.isnan(s) or math.isnan(t)]
    if n > 0:
        mae, abs_rel, mse, sq_rel, d1, d2, d3 = (v / n for v in tot[1:])
        rmse = math.sqrt(mse)
    else:
        mae = abs_rel = rmse = sq_rel = d1 = d2 = d3 = math.nan
    return DepthMetrics(abs_rel=abs_rel, sq_rel=sq_rel, mae=mae, rmse=rmse, delta1=d1, delta2=d2, delta3=d3,
                        n_valid=int(n), scale=scale, shift=shift, per_frame=per_frame, frames_skipped=skipped)


def align_scale_shift(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                      per_frame: bool = False, valid_range=(1e-3, math.inf)
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Least-squares (scale, shift) of pred onto target over the valid pixels — mask ≠ 0, both finite,
    valid_range[0] < target < valid_range[1] — for the whole video, or per frame.

    pred, target: [N, H, W] or [N, 1, H, W], f16 or f32, on the host or the device (host tensors are moved to
    cuda:0); mask: bool / uint8 of the same shape.  Returns host tensors (scale f64 [N], shift f64 [N],
    moments f64 [N, 6] = n, Σp, Σg, Σp², Σpg, Σg² per frame); the video fit is repeated in every row.  A frame
    (video) with fewer than two valid pixels or a constant pred has no fit: NaN."""
    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range)
    from . import kernels as K

    ws = K.depth_moments(p, g, m, lo, hi)
    moments, st = K.depth_fit(ws, p.shape[0], p.shape[1], K.DEPTH_FIT_MODES["frame" if per_frame else "video"])
    st = st.cpu()
    return st[:, 0].contiguous(), st[:, 1].contiguous(), moments.cpu()


def depth_metrics(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                  align: str = "video", valid_range=(1e-3, math.inf), clip: Optional[Tuple[float, float]] = None
                  ) -> DepthMetrics:
    """AbsRel, SqRel, MAE, RMSE and δ < 1.25ᵏ of scale·pred + shift against target on the valid pixels.

    align: "video" (one least-squares fit for all frames), "frame" (one per frame) or "none" (pred as it is).
    clip: (lo, hi) clamps the aligned prediction — never the target — before the errors are taken.  Inputs as
    for align_scale_shift.  Frames without a fit are left out and listed in frames_skipped; with no valid
    pixel at all every metric is NaN."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align: one of {ALIGN_MODES} expected, got {align!r}")
    clip_lo, clip_hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    if not clip_lo <= clip_hi:
        raise ValueError(f"clip: lo <= hi expected, got ({clip_lo}, {clip_hi})")
    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range)
    from . import kernels as K

    N, P = p.shape
    ws = K.depth_metrics_workspace(N, P, p.device)
    if align != "none":
        K.depth_moments(p, g, m, lo, hi, ws)
    _, st = K.depth_fit(ws if align != "none" else None, N, P, K.DEPTH_FIT_MODES[align], device=p.device)
    sums = K.depth_errors(p, g, m, st, lo, hi, clip_lo, clip_hi, ws)
    st = st.cpu()
    return _pool(sums.cpu(), st[:, 0].contiguous(), st[:, 1].contiguous())
