"""Flow-guided temporal stabilisation of a depth video, on the device (rdmi_temporal_filter, include/rdmi.h
"Temporal filter").

The co-aligned depth of a video still flickers a little from frame to frame (temporal_metrics reports it).  Here
every pixel is averaged with the depths its 2·radius neighbouring frames hold where the optical flow says the pixel
went: a bilateral filter along the motion, with weights exp(−k²/2σt²) over the frame distance k (sigma_time, in
frames) and exp(−δ²/2σd²) over the depth difference δ (sigma_depth, in the units of the depth), the frame's own
weight being 1.  Pixels the forward–backward check marks occluded, flows that leave the frame and non-finite
depths do not take part, so a depth edge that moves is not smeared and a pixel without neighbours stays as it is.

    d = temporal_filter(depth, frames)                       # the flow is estimated here (flow.optical_flow's chain)
    d = temporal_filter(depth, flow=flow, valid=valid)       # or given: f32 [2R, N, H, W, 2], uint8 [2R, N, H, W]

Deterministic, no learned part.  The defaults (radius 2, sigma_time 1, sigma_depth 0.05) have met synthetic scenes
only."""
from __future__ import annotations

import math
import numbers
from typing import Dict, Optional, Tuple

import torch

from .flow import check_flow_args

MAX_RADIUS = 3  # RDMI_TFILTER_MAX_RADIUS
_FLOW_KWARGS = ("levels", "iterations", "radius", "damping", "fb_tol")
# slot pixels (2·radius·n·H·W) of one launch: their packed flow (8 B) and valid (1 B) stay within 1 GiB.  The result
# does not depend on the chunking.
_CHUNK_ELEMS = (1 << 30) // 9
# the f32 constants log2 e / (2σ²) of the kernel must be finite and positive (rdmi.h): σ within these bounds
_SIGMA_MIN, _SIGMA_MAX = 1e-19, 1e22


def check_stabilize_params(radius=2, sigma_time=1.0, sigma_depth=0.05, flow_kwargs=None, return_flow=False) -> Dict:
    """The scalar arguments of temporal_filter, without any tensor → flow_kwargs as a dict.  TypeError for a wrong
    type (bools are not numbers here), ValueError for a wrong value or an unknown flow keyword."""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral):
        raise TypeError(f"radius must be an int, got {radius!r}")
    for name, s in (("sigma_time", sigma_time), ("sigma_depth", sigma_depth)):
        if isinstance(s, bool) or not isinstance(s, numbers.Real):
            raise TypeError(f"{name} must be a number, got {s!r}")
        if not (math.isfinite(s) and _SIGMA_MIN <= s <= _SIGMA_MAX):
            raise ValueError(f"{name} must be a finite number in [{_SIGMA_MIN}, {_SIGMA_MAX}], got {s!r}")
    if not isinstance(return_flow, bool):
        raise TypeError(f"return_flow must be a bool, got {type(return_flow).__name__}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must lie in 1 … {MAX_RADIUS}, got {radius}")
    fk = {} if flow_kwargs is None else flow_kwargs
    if not isinstance(fk, dict):
        raise TypeError(f"flow_kwargs must be None or a dict, got {type(flow_kwargs).__name__}")
    bad = [k for k in fk if k not in _FLOW_KWARGS]
    if bad:
        raise ValueError(f"flow_kwargs: unknown keys {bad}; known: {_FLOW_KWARGS}")
    check_flow_args(torch.empty((2, 3, 1, 1), dtype=torch.float32, device="meta"), 1, **fk)
    return dict(fk)


def check_stabilize_args(depth, frames=None, flow=None, valid=None, radius=2, sigma_time=1.0, sigma_depth=0.05,
                         flow_kwargs=None, return_flow=False) -> Tuple[int, int, int]:
    """Everything temporal_filter can refuse without a device → (N, H, W).  TypeError for a wrong type, ValueError
    for a wrong value or shape."""
    for name, t, need in (("depth", depth, True), ("frames", frames, False), ("flow", flow, False),
                          ("valid", valid, False)):
        if (need or t is not None) and not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a tensor expected, got {type(t).__name__}")
    if depth.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"depth: float16 or float32 expected, got {depth.dtype}")
    if frames is not None and frames.dtype != torch.uint8 and not frames.is_floating_point():
        raise TypeError(f"frames: uint8 [N, H, W, 3] or float [N, 3, H, W] expected, got {frames.dtype}")
    if flow is not None and flow.dtype != torch.float32:
        raise TypeError(f"flow: float32 expected, got {flow.dtype}")
    if valid is not None and valid.dtype != torch.uint8:
        raise TypeError(f"valid: uint8 expected, got {valid.dtype}")
    fk = check_stabilize_params(radius, sigma_time, sigma_depth, flow_kwargs, return_flow)
    if (frames is None) == (flow is None):
        raise ValueError("exactly one of frames and flow must be given")
    if valid is not None and flow is None:
        raise ValueError("valid belongs to flow: with frames the mask is estimated")
    if fk and frames is None:
        raise ValueError("flow_kwargs belong to frames: a given flow is taken as it is")
    if depth.dim() == 4 and depth.shape[1] == 1:
        N, _, H, W = depth.shape
    elif depth.dim() == 3:
        N, H, W = depth.shape
    else:
        raise ValueError(f"depth: [N, H, W] or [N, 1, H, W] expected, got {tuple(depth.shape)}")
    if min(N, H, W) < 1:
        raise ValueError(f"depth: empty input {tuple(depth.shape)}")
    if H * W > 1 << 30:
        raise ValueError(f"depth: H·W = {H * W} above 2^30")
    if frames is not None:
        if frames.dim() != 4:
            raise ValueError(f"frames: uint8 [N, H, W, 3] or float [N, 3, H, W] expected, got {tuple(frames.shape)}")
        if frames.dtype == torch.uint8:
            Nf, Hf, Wf, Cf = frames.shape
        else:
            Nf, Cf, Hf, Wf = frames.shape
        if Cf != 3:
            raise ValueError(f"frames: three channels expected (uint8 [N, H, W, 3] or float [N, 3, H, W]), got "
                             f"{tuple(frames.shape)}")
        if Nf != N:
            raise ValueError(f"frames: {N} frames expected as in depth, got {Nf}")
        if (Hf, Wf) != (H, W):
            raise ValueError(f"frames of {Hf} x {Wf} against a depth of {H} x {W}: resize the frames to the depth's "
                             f"resolution first")
    else:
        if tuple(flow.shape) != (2 * radius, N, H, W, 2):
            raise ValueError(f"flow: {(2 * radius, N, H, W, 2)} expected, got {tuple(flow.shape)}")
        if valid is not None and tuple(valid.shape) != (2 * radius, N, H, W):
            raise ValueError(f"valid: {(2 * radius, N, H, W)} expected, got {tuple(valid.shape)}")
    return N, H, W


def chunk_flow(frames: torch.Tensor, a: int, b: int, R: int, levels=None, iterations: int = 3, radius: int = 5,
               damping: float = 0.01, fb_tol=(0.01, 0.5)) -> Tuple[torch.Tensor, torch.Tensor]:
    """The packed flow f32 [2R, b − a, H, W, 2] and mask uint8 [2R, b − a, H, W] of the output frames [a, b) from
    device frames (f16 / f32 [N, 3, H, W] or uint8 [N, H, W, 3]).  One luma pyramid of frames [a − R, b + R) serves
    all offsets; per offset k the level chain of optical_flow runs in both directions over the pairs (p, p + k) the
    chunk needs, then the forward–backward check both ways.  Slot +k, row i is the forward flow of pair (i, i + k);
    slot −k, row i the backward flow of pair (i − k, i).  Rows without a neighbour inside the video stay zero
    (valid 0).  The chain gives a pair the same bits alone or in a batch (rdmi.h), so slot +k equals
    optical_flow(frames, k).flow and slot −k its flow_backward, whatever the chunk."""
    from . import kernels as K

    u8 = frames.dtype == torch.uint8
    N = frames.shape[0]
    H, W = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
    dev = frames.device
    flow = torch.zeros((2 * R, b - a, H, W, 2), dtype=torch.float32, device=dev)
    valid = torch.zeros((2 * R, b - a, H, W), dtype=torch.uint8, device=dev)
    lo, hi = max(a - R, 0), min(b + R, N)
    if hi - lo < 2:
        return flow, valid
    lv = K.flow_levels(H, W, radius, levels)
    pyr = K.flow_pyramid(frames[lo:hi], lv)
    alpha, beta = float(fb_tol[0]), float(fb_tol[1])
    for k in range(1, R + 1):
        p0, p1 = max(a - k, 0), min(b, N - k)  # the pairs (p, p + k), p0 ≤ p < p1
        if p1 <= p0:
            continue
        fwd = bwd = None
        for l in range(lv - 1, -1, -1):
            fwd = K.flow_lk_level(pyr[l], p0 - lo, p0 + k - lo, p1 - p0, fwd, radius, iterations, float(damping))
            bwd = K.flow_lk_level(pyr[l], p0 + k - lo, p0 - lo, p1 - p0, bwd, radius, iterations, float(damping))
        vf = K.flow_fb_check(fwd, bwd, alpha, beta)
        vb = K.flow_fb_check(bwd, fwd, alpha, beta)
        i0, i1 = max(a, p0), min(b, p1)  # slot +k: rows i = p
        if i1 > i0:
            flow[R + k - 1, i0 - a:i1 - a] = fwd[i0 - p0:i1 - p0]
            valid[R + k - 1, i0 - a:i1 - a] = vf[i0 - p0:i1 - p0]
        i0, i1 = max(a, p0 + k), min(b, p1 + k)  # slot −k: rows i = p + k
        if i1 > i0:
            flow[R - k, i0 - a:i1 - a] = bwd[i0 - k - p0:i1 - k - p0]
            valid[R - k, i0 - a:i1 - a] = vb[i0 - k - p0:i1 - k - p0]
    return flow, valid


def temporal_filter(depth: torch.Tensor, frames: Optional[torch.Tensor] = None, *,
                    flow: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, radius: int = 2,
                    sigma_time: float = 1.0, sigma_depth: float = 0.05, flow_kwargs: Optional[Dict] = None,
                    return_flow: bool = False):
    """Motion-compensated temporal filter of a depth video.

    depth: [N, H, W] or [N, 1, H, W], float16 or float32, on the host or the device.
    Exactly one of `frames` and `flow`:
      frames: the video at the depth's own resolution (the caller resizes), float [N, 3, H, W] in any affine range
        or uint8 [N, H, W, 3].  The flow between frame i and frame i ± k, k = 1 … radius, and its forward–backward
        mask are estimated with optical_flow's chain; flow_kwargs: its levels, iterations, radius, damping, fb_tol.
      flow: f32 [2·radius, N, H, W, 2], slot s for k = −radius, …, −1, +1, …, +radius, row i = (dx, dy) from frame i
        to frame i + k at the pixels of frame i; valid: uint8 [2·radius, N, H, W] or None (all ones).  Rows whose
        i + k lies outside the video are not read.
    radius 1 … 3 frames each way.  sigma_time > 0 in frames, sigma_depth > 0 in the units of depth.
    Returns the filtered depth in depth's shape, dtype and device, computed in f32 and cast once.  With
    return_flow=True: (depth, flow, valid) with the packed flow and mask of the whole video on the device of the
    computation — 9·2·radius bytes per pixel and frame, memory-hungry: meant for inspection and tests.
    The video is processed in chunks of frames; the same inputs give the same bits whatever the chunking."""
    N, H, W = check_stabilize_args(depth, frames, flow, valid, radius, sigma_time, sigma_depth, flow_kwargs,
                                   return_flow)
    from . import kernels as K

    R = int(radius)
    other = frames if frames is not None else flow
    dev = depth.device if depth.is_cuda else (other.device if other.is_cuda else torch.device("cuda", 0))
    d = depth.to(dev).reshape(N, H, W).contiguous()
    if frames is not None:
        fr = frames.to(dev)
        if fr.dtype not in (torch.float16, torch.float32, torch.uint8):
            fr = fr.float()
    out = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    step = max(1, _CHUNK_ELEMS // (2 * R * H * W))
    keep = []
    for a in range(0, N, step):
        b = min(a + step, N)
        if frames is not None:
            fl, va = chunk_flow(fr, a, b, R, **(flow_kwargs or {}))
        else:
            fl = flow[:, a:b].to(dev).contiguous()
            va = None if valid is None else valid[:, a:b].to(dev).contiguous()
        K.temporal_filter(d, fl, va, R, float(sigma_time), float(sigma_depth), f0=a, n=b - a, out=out[a:b])
        if return_flow:
            keep.append((fl, va))
    res = out.to(depth.dtype).reshape(depth.shape).to(depth.device)
    if not return_flow:
        return res
    fl = keep[0][0] if len(keep) == 1 else torch.cat([f for f, _ in keep], dim=1)
    if keep[0][1] is None:
        va = None
    else:
        va = keep[0][1] if len(keep) == 1 else torch.cat([v for _, v in keep], dim=1)
    return res, fl, va
