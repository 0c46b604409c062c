"""Dense optical flow from the RGB frames, for the temporal metrics.

temporal_metrics compares frame i with frame i + k at the same pixel unless it is given a flow; on a moving camera
that mostly measures the camera.  This module estimates the flow, and the occlusion mask that goes with it, from
the frames every run already has on the device:

    r = optical_flow(frames)                                   # frames [N, 3, H, W] f16 / f32, or uint8 [N, H, W, 3]
    t = temporal_metrics(pred, target, flow=r.flow, pair_mask=r.valid)
    t = temporal_metrics(pred, target, frames=frames)          # the same, in one call

The estimator is a classical pyramidal Lucas–Kanade with template gradients, run per pixel over a (2·radius + 1)²
window, and a forward–backward consistency check; the algorithm is fixed operation by operation in include/rdmi.h
("Optical flow") and runs in librdmi (rdmi_flow_estimate).  It is deterministic — the same frames give the same bits,
for a pair alone or in a batch — and has no learned part: an evaluation instrument, not a competitor to learned flow.
Motions beyond the pyramid's reach (about 2^(levels − 1) · iterations pixels per level chain) are not recovered; the
forward–backward check then marks most of the affected pixels invalid.  This module only validates and allocates.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

MAX_RADIUS = 7
MAX_LEVELS = 5


@dataclass
class OpticalFlow:
    """flow: f32 [N − k, H, W, 2], (dx, dy) in pixels from frame i to frame i + k — temporal_metrics' convention.
    flow_backward: the same from frame i + k to frame i, at the pixels of frame i + k, or None.  valid: uint8
    [N − k, H, W], 1 where the forward target lies inside the frame and the two flows agree (pair_mask's
    meaning), or None without the backward flow.  levels: the pyramid levels used."""
    flow: torch.Tensor
    flow_backward: Optional[torch.Tensor]
    valid: Optional[torch.Tensor]
    levels: int


def _int(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name}: an int expected, got {type(v).__name__}")
    return v


def _real(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name}: a real number expected, got {type(v).__name__}")
    return float(v)


def check_flow_args(frames, frame_step=1, levels=None, iterations=3, radius=5, damping=0.01, backward=True,
                    fb_tol=(0.01, 0.5)) -> Tuple[int, int, int, float, float]:
    """optical_flow's checks, all before any device work → (N, H, W, alpha, beta).  TypeError for wrong types and
    bools, ValueError for shapes and ranges."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames: a tensor expected, got {type(frames).__name__}")
    if frames.dtype not in (torch.float16, torch.float32, torch.uint8):
        raise TypeError(f"frames: float16 / float32 [N, 3, H, W] or uint8 [N, H, W, 3] expected, got {frames.dtype}")
    _int(frame_step, "frame_step")
    if levels is not None:
        _int(levels, "levels")
    _int(iterations, "iterations")
    _int(radius, "radius")
    damping = _real(damping, "damping")
    if not isinstance(backward, bool):
        raise TypeError(f"backward: a bool expected, got {type(backward).__name__}")
    if isinstance(fb_tol, (str, bytes, torch.Tensor)) or not hasattr(fb_tol, "__len__"):
        raise TypeError(f"fb_tol: a pair (alpha, beta) expected, got {type(fb_tol).__name__}")
    if len(fb_tol) != 2:
        raise ValueError(f"fb_tol: a pair (alpha, beta) expected, got {len(fb_tol)} values")
    alpha, beta = _real(fb_tol[0], "fb_tol"), _real(fb_tol[1], "fb_tol")
    if frames.dim() != 4:
        raise ValueError(f"frames: [N, 3, H, W] (uint8: [N, H, W, 3]) expected, got {tuple(frames.shape)}")
    if frames.dtype == torch.uint8:
        N, H, W, Cc = frames.shape
    else:
        N, Cc, H, W = frames.shape
    if Cc != 3:
        raise ValueError(f"frames: three channels expected, got shape {tuple(frames.shape)} for {frames.dtype}")
    if H < 1 or W < 1:
        raise ValueError(f"frames: empty input {tuple(frames.shape)}")
    if H * W > 1 << 30:
        raise ValueError(f"frames: H·W = {H * W} above 2^30")
    if not 1 <= frame_step < N:
        raise ValueError(f"frame_step: 1 <= frame_step < N = {N} expected, got {frame_step}")
    if N - frame_step > 65535:
        raise ValueError(f"frames: {N - frame_step} pairs (at most 65535 pairs in one call)")
    if levels is not None and levels < 1:
        raise ValueError(f"levels: None or at least 1 expected, got {levels}")
    if iterations < 1:
        raise ValueError(f"iterations: at least 1 expected, got {iterations}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius: 1 <= radius <= {MAX_RADIUS} expected, got {radius}")
    if not (damping >= 0 and math.isfinite(damping)):
        raise ValueError(f"damping: a finite value >= 0 expected, got {damping}")
    if not (alpha >= 0 and beta >= 0 and math.isfinite(alpha) and math.isfinite(beta)):
        raise ValueError(f"fb_tol: finite values >= 0 expected, got ({alpha}, {beta})")
    return N, H, W, alpha, beta


def pyramid_levels(H: int, W: int, radius: int = 5, levels: Optional[int] = None) -> int:
    """The level rule in Python (librdmi's rdmi_flow_levels is the same rule in C; the tests hold them equal): stop
    before a level whose smaller side would fall below 4·(2·radius + 1), at most 5 levels, at least one; a
    caller's `levels` is clamped to that count."""
    n, h, w = 1, (H + 1) // 2, (W + 1) // 2
    while n < MAX_LEVELS and min(h, w) >= 4 * (2 * radius + 1):
        n, h, w = n + 1, (h + 1) // 2, (w + 1) // 2
    return n if levels is None else max(1, min(levels, n))


def optical_flow(frames: torch.Tensor, frame_step: int = 1, *, levels: Optional[int] = None, iterations: int = 3,
                 radius: int = 5, damping: float = 0.01, backward: bool = True,
                 fb_tol: Tuple[float, float] = (0.01, 0.5)) -> OpticalFlow:
    """Dense flow from frame i to frame i + frame_step for every pair of the video, on the device.

    frames: [N, 3, H, W] float16 / float32 in any affine range (the pipeline's [−1, 1] as it is), or uint8
    [N, H, W, 3]; on the host or the device (host tensors are moved to cuda:0); any strided view is read in
    place.  levels: pyramid levels, None for the rule of pyramid_levels, which also clamps a request.
    iterations: Lucas–Kanade steps per level, each at most 1 px long.  radius: the window is (2·radius + 1)²
    (1 … 7).  damping: λ = damping · ½·trace A + 1e-12 on the structure tensor's diagonal.  backward: also estimate
    the flow from i + frame_step to i and the forward–backward mask; fb_tol = (α, β): a pixel is valid iff its target
    lies inside the frame and |u_f + u_b|² <= α·(|u_f|² + |u_b|²) + β, u_b sampled at the target."""
    N, H, W, alpha, beta = check_flow_args(frames, frame_step, levels, iterations, radius, damping, backward, fb_tol)
    from . import kernels as K

    lv = K.flow_levels(H, W, radius, levels)
    x = frames if frames.is_cuda else frames.to(torch.device("cuda", 0))
    flow, bwd, valid = K.flow_estimate(x, frame_step, lv, radius, iterations, float(damping), backward, alpha, beta)
    return OpticalFlow(flow=flow, flow_backward=bwd, valid=valid, levels=lv)
