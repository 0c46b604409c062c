"""Edge-aware restore of a low-resolution depth video: joint bilateral upsampling (Kopf et al. 2007) along the
full-resolution frames, on the device (rdmi_joint_bilateral_upsample, include/rdmi.h "Guided upsampling").

An antialiased resize turns every depth discontinuity into a ramp about (output size / processing size) pixels wide;
here each output pixel averages its (2·radius)² nearest low-resolution depths with weights that fall off with the
distance in the low-resolution grid (sigma_spatial, in low-resolution pixels) and with the colour difference between
the full-resolution frame at the pixel and the frame resized to the depth's resolution at the tap (sigma_range, in
units of the frame's [0, 1] range), so the depth edge lands on the image edge.  Deterministic, no learned part.

The defaults (radius 2, sigma_spatial 1, sigma_range 0.1) have met synthetic guides only."""
from __future__ import annotations

import math
import numbers

import torch

MAX_RADIUS = 3    # RDMI_JBU_MAX_RADIUS
MAX_CHANNELS = 4
_CHUNK_ELEMS = 1 << 28  # f32 output elements per launch (1 GiB): the result does not depend on the chunking


def check_upsample_args(depth, frames, radius=2, sigma_spatial=1.0, sigma_range=0.1):
    """Everything guided_upsample can refuse without a device → (N, C, h, w, H, W).  TypeError for a wrong type,
    ValueError for a wrong value or shape."""
    for name, t in (("depth", depth), ("frames", frames)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a tensor expected, got {type(t).__name__}")
    if depth.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"depth: float16 or float32 expected, got {depth.dtype}")
    if frames.dtype != torch.uint8 and not frames.is_floating_point():
        raise TypeError(f"frames: uint8 [N, H, W, 3] or float [N, 3, H, W] expected, got {frames.dtype}")
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral):
        raise TypeError(f"radius must be an int, got {radius!r}")
    for name, s in (("sigma_spatial", sigma_spatial), ("sigma_range", sigma_range)):
        if isinstance(s, bool) or not isinstance(s, numbers.Real):
            raise TypeError(f"{name} must be a number, got {s!r}")
        if not (s > 0 and math.isfinite(s)):
            raise ValueError(f"{name} must be a finite number > 0, got {s!r}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must lie in 1 … {MAX_RADIUS}, got {radius}")
    if depth.dim() != 4 or not 1 <= depth.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"depth: [N, C, h, w] with C in 1 … {MAX_CHANNELS} expected, got {tuple(depth.shape)}")
    if frames.dim() != 4:
        raise ValueError(f"frames: uint8 [N, H, W, 3] or float [N, 3, H, W] expected, got {tuple(frames.shape)}")
    if frames.dtype == torch.uint8:
        Nf, H, W, Cf = frames.shape
    else:
        Nf, Cf, H, W = frames.shape
    if Cf != 3:
        raise ValueError(f"frames: three channels expected (uint8 [N, H, W, 3] or float [N, 3, H, W]), got "
                         f"{tuple(frames.shape)}")
    N, C, h, w = depth.shape
    if Nf != N:
        raise ValueError(f"frames: {N} frames expected as in depth, got {Nf}")
    if min(N, h, w, H, W) < 1:
        raise ValueError(f"empty input: depth {tuple(depth.shape)}, frames {tuple(frames.shape)}")
    if H < h or W < w:
        raise ValueError(f"frames of {H} x {W} are smaller than the depth's {h} x {w}: guided_upsample only upsamples")
    return N, C, h, w, H, W


def upsample_on_device(depth: torch.Tensor, frames: torch.Tensor, radius: int, sigma_spatial: float,
                       sigma_range: float, out_dtype) -> torch.Tensor:
    """guided_upsample's device part: depth [N, C, h, w] (f16 / f32) and frames (uint8 [N, H, W, 3] or f32
    [N, 3, H, W] in [0, 1]) on one device → [N, C, H, W] of out_dtype there.  Frames are taken a chunk at a time so
    that the f32 result of one launch stays within 1 GiB; a frame's result does not depend on its neighbours."""
    from . import kernels as K

    N, C, h, w = depth.shape
    u8 = frames.dtype == torch.uint8
    H, W = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
    depth = depth.contiguous()
    out = torch.empty((N, C, H, W), dtype=out_dtype, device=depth.device)
    step = max(1, _CHUNK_ELEMS // (C * H * W))
    for i0 in range(0, N, step):
        fr = frames[i0:i0 + step]
        guide_lo = K.resize(fr, (h, w), "BILINEAR", channels_last=u8)
        if u8:
            guide_lo.mul_(1.0 / 255.0)
        r = K.joint_bilateral_upsample(depth[i0:i0 + step], guide_lo, fr, radius, sigma_spatial, sigma_range,
                                       channels_last=u8)
        out[i0:i0 + step].copy_(r)
    return out


def guided_upsample(depth: torch.Tensor, frames: torch.Tensor, radius: int = 2, sigma_spatial: float = 1.0,
                    sigma_range: float = 0.1) -> torch.Tensor:
    """Joint bilateral upsampling of `depth` to the resolution of `frames`.

    depth: [N, C, h, w], float16 or float32, C = 1 … 4 maps that share one set of weights (depth and its
        uncertainty go through together), on the device or on the host.
    frames: the video at the wanted resolution, uint8 [N, H, W, 3] (decoded rgb24) or float [N, 3, H, W] in [0, 1],
        H ≥ h and W ≥ w.  The low-resolution guide is built here: the antialiased bilinear resize of the frames to
        h × w (kernels.resize), in [0, 1].
    radius 1 … 3: (2·radius)² low-resolution taps per output pixel.  sigma_spatial > 0 in low-resolution pixels,
        sigma_range > 0 in units of the frames' [0, 1] range.
    Returns [N, C, H, W] of depth's dtype on depth's device, computed in f32 and cast once.  The same inputs give
    the same bits on every call, for a frame alone or in a video, and for a map alone or among others."""
    check_upsample_args(depth, frames, radius, sigma_spatial, sigma_range)
    dev = depth.device if depth.is_cuda else (frames.device if frames.is_cuda else torch.device("cuda"))
    fr = frames.to(dev)
    if fr.dtype != torch.uint8:
        fr = fr.float()
    r = upsample_on_device(depth.to(dev), fr, int(radius), float(sigma_spatial), float(sigma_range), depth.dtype)
    return r.to(depth.device)
