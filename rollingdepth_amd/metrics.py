"""Affine-invariant depth metrics on the device.

A diffusion depth video is defined up to one scale and one shift, so comparing it pixel by pixel with a
ground truth — or with another build, stride or dtype of the same pipeline — mostly measures that offset.
The standard protocol (the RollingDepth paper's) fits the scale and shift by least squares, per video or per
frame, and reports AbsRel and δ < 1.25ᵏ on the valid pixels:

    m = depth_metrics(pred, target)                       # one fit for the video
    m = depth_metrics(pred, target, mask, align="frame")  # one fit per frame
    m.abs_rel, m.delta1, m.scale, m.shift

The fit can also be taken in disparity or log-depth (space="disparity" | "log": against 1 / target or
ln target, the aligned value brought back to depth before the errors), and temporal_metrics scores the change
from frame to frame — flicker, and the temporal-gradient error against the target's own change — optionally
along an optical flow the caller supplies or that is estimated from the RGB frames (flow.py):

    t = temporal_metrics(pred, target, mask, flow=flow)   # flow [N − 1, H, W, 2], (dx, dy) in pixels
    t = temporal_metrics(pred, target, mask, frames=rgb)  # flow and occlusion mask estimated from the frames
    t.flicker, t.tge, t.change_corr

boundary_metrics scores what the per-pixel errors hardly see, the occlusion boundaries: precision, recall and F1 of
the edges of the aligned prediction — a neighbour more than τ times farther — against the target's, pixel-exact:

    b = boundary_metrics(pred, target, mask)              # ten thresholds τ = 1.05 … 1.25
    b.f1, b.precision, b.recall, b.f1_per_threshold

All sums run in librdmi (rdmi_depth_moments / _fit / _errors / _temporal, f64, fixed summation order, and
rdmi_depth_boundary, integers: the same inputs give the same bits on every call); this module only validates,
reshapes and does the last few host divisions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

ALIGN_MODES = ("video", "frame", "none")
SPACES = ("depth", "disparity", "log")


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


def _prepare(pred: torch.Tensor, target: Optional[torch.Tensor], mask: Optional[torch.Tensor], valid_range,
             more_checks=None
             ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], float, float]:
    """Validate (before any device work) and bring the operands to contiguous [N, P] tensors on the device.
    target None is temporal_metrics' call without one; more_checks((N, H, W)) are its further checks, run after
    these and still before any device work."""
    for t, name in ((pred, "pred"), (target, "target")):
        if t is None:
            continue
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
    if more_checks is not None:
        more_checks(shape)

    dev = _device(pred, target)

    def flat(t):
        return t.to(dev).contiguous().view(shape[0], shape[1] * shape[2])

    m = None
    if mask is not None:
        m = flat(mask)
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
    return flat(pred), None if target is None else flat(target), m, lo, hi


def _device(pred: torch.Tensor, target: Optional[torch.Tensor]) -> torch.device:
    if pred.is_cuda:
        return pred.device
    return target.device if target is not None and target.is_cuda else torch.device("cuda", 0)


def _space_and_clip(space, clip) -> Tuple[float, float]:
    """The checks depth_metrics and temporal_metrics share → (clip_lo, clip_hi)."""
    if space not in SPACES:
        raise ValueError(f"space: one of {SPACES} expected, got {space!r}")
    clip_lo, clip_hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    if not clip_lo <= clip_hi:
        raise ValueError(f"clip: lo <= hi expected, got ({clip_lo}, {clip_hi})")
    if space == "disparity" and math.isinf(clip_hi):
        raise ValueError("clip: space='disparity' needs a finite upper clip (a non-positive aligned disparity has no "
                         f"finite depth: name the depth cap), got {clip}")
    return clip_lo, clip_hi


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
                      per_frame: bool = False, valid_range=(1e-3, math.inf), space: str = "depth"
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Least-squares (scale, shift) of pred onto target over the valid pixels — mask ≠ 0, both finite,
    valid_range[0] < target < valid_range[1] — for the whole video, or per frame.

    pred, target: [N, H, W] or [N, 1, H, W], f16 or f32, on the host or the device (host tensors are moved to
    cuda:0); mask: bool / uint8 of the same shape.  Returns host tensors (scale f64 [N], shift f64 [N],
    moments f64 [N, 6] = n, Σp, Σg, Σp², Σpg, Σg² per frame); the video fit is repeated in every row.  A frame
    (video) with fewer than two valid pixels or a constant pred has no fit: NaN.

    space: "depth", "disparity" or "log" — the fit is of pred onto φ(target) = target, 1 / target or ln target
    (valid pixels then also need target > 0), and scale, shift and the moments (with g = φ(target)) are those of
    that space."""
    if space not in SPACES:
        raise ValueError(f"space: one of {SPACES} expected, got {space!r}")
    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range)
    from . import kernels as K

    ws = K.depth_moments(p, g, m, lo, hi, space=K.DEPTH_SPACES[space])
    moments, st = K.depth_fit(ws, p.shape[0], p.shape[1], K.DEPTH_FIT_MODES["frame" if per_frame else "video"])
    st = st.cpu()
    return st[:, 0].contiguous(), st[:, 1].contiguous(), moments.cpu()


def depth_metrics(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None,
                  align: str = "video", valid_range=(1e-3, math.inf), clip: Optional[Tuple[float, float]] = None,
                  space: str = "depth") -> DepthMetrics:
    """AbsRel, SqRel, MAE, RMSE and δ < 1.25ᵏ of scale·pred + shift against target on the valid pixels.

    align: "video" (one least-squares fit for all frames), "frame" (one per frame) or "none" (pred as it is).
    clip: (lo, hi) clamps the aligned prediction — never the target — before the errors are taken.  Inputs as
    for align_scale_shift.  Frames without a fit are left out and listed in frames_skipped; with no valid
    pixel at all every metric is NaN.

    space: the fit is taken in "depth", "disparity" or "log" space (see align_scale_shift) and the aligned value
    a = φ⁻¹(scale·pred + shift) — the value itself, its reciprocal or its exponential — is compared with the
    target in depth; scale and shift stay those of the fit space.  "disparity" needs a clip with a finite upper
    bound: an aligned disparity ≤ 0 has no finite depth and is taken to the cap."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align: one of {ALIGN_MODES} expected, got {align!r}")
    clip_lo, clip_hi = _space_and_clip(space, clip)
    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range)
    from . import kernels as K

    N, P = p.shape
    sp = K.DEPTH_SPACES[space]
    ws = K.depth_metrics_workspace(N, P, p.device)
    if align != "none":
        K.depth_moments(p, g, m, lo, hi, ws, space=sp)
    _, st = K.depth_fit(ws if align != "none" else None, N, P, K.DEPTH_FIT_MODES[align], device=p.device)
    sums = K.depth_errors(p, g, m, st, lo, hi, clip_lo, clip_hi, ws, space=sp)
    st = st.cpu()
    return _pool(sums.cpu(), st[:, 0].contiguous(), st[:, 1].contiguous())


@dataclass
class TemporalMetrics:
    """Pooled over all valid pixels of all pairs (each pair's sums added in pair order, ÷ n_valid).  Pair i is
    frame i against frame i + frame_step; Δa and Δg are the changes of the aligned prediction and of the target
    between the two.  Without a target the four target-based fields are NaN."""
    flicker: float         # mean |Δa|
    flicker_rmse: float    # sqrt(mean Δa²)
    tge: float             # temporal-gradient error: mean |Δa − Δg|
    tge_rmse: float        # sqrt(mean (Δa − Δg)²)
    target_change: float   # mean |Δg|
    change_corr: float     # ΣΔa·Δg / sqrt(ΣΔa² · ΣΔg²); NaN when either factor is 0
    n_valid: int
    scale: torch.Tensor      # f64 [N], host
    shift: torch.Tensor      # f64 [N], host
    # f64 [N − frame_step, 8], host: n, Σ|Δa|, ΣΔa², Σ|Δa−Δg|, Σ(Δa−Δg)², Σ|Δg|, ΣΔg², ΣΔa·Δg
    per_pair: torch.Tensor
    pairs_skipped: List[int]  # pairs with a frame without a fit (NaN scale / shift): they contribute nothing


def _pool_temporal(per_pair: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, frame_step: int,
                   has_target: bool = True) -> TemporalMetrics:
    """Host tensors (f64 [N − k, 8] pair sums, f64 [N] scale / shift) → TemporalMetrics."""
    tot = [0.0] * 8
    for row in per_pair.tolist():  # pair order, f64
        for k in range(8):
            tot[k] += row[k]
    n = tot[0]
    nofit = [math.isnan(s) or math.isnan(t) for s, t in zip(scale.tolist(), shift.tolist())]
    skipped = [i for i in range(per_pair.shape[0]) if nofit[i] or nofit[i + frame_step]]
    nan = math.nan
    flicker = flicker_rmse = tge = tge_rmse = target_change = change_corr = nan
    if n > 0:
        flicker, flicker_rmse = tot[1] / n, math.sqrt(tot[2] / n)
        if has_target:
            tge, tge_rmse, target_change = tot[3] / n, math.sqrt(tot[4] / n), tot[5] / n
            if tot[2] > 0 and tot[6] > 0:
                change_corr = tot[7] / math.sqrt(tot[2] * tot[6])
    return TemporalMetrics(flicker=flicker, flicker_rmse=flicker_rmse, tge=tge, tge_rmse=tge_rmse,
                           target_change=target_change, change_corr=change_corr, n_valid=int(n), scale=scale,
                           shift=shift, per_pair=per_pair, pairs_skipped=skipped)


def temporal_metrics(pred: torch.Tensor, target: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     *, flow: Optional[torch.Tensor] = None, pair_mask: Optional[torch.Tensor] = None,
                     frame_step: int = 1, align: str = "video", space: str = "depth",
                     valid_range=(1e-3, math.inf), clip: Optional[Tuple[float, float]] = None,
                     frames: Optional[torch.Tensor] = None) -> TemporalMetrics:
    """Temporal consistency of a depth video: the change of the aligned prediction a between frame i and frame
    i + frame_step (flicker) and its difference from the target's own change (temporal-gradient error).

    pred, target, mask, align, space, valid_range and clip as for depth_metrics: the fit is the one depth_metrics
    takes and every frame is aligned with its own scale and shift.  Without a target there is nothing to fit:
    align must be "none", only the mask and the finiteness of pred decide validity, and the target-based fields
    are NaN.  flow: f32 [N − frame_step, H, W, 2], (dx, dy) in pixels from frame i to frame i + frame_step; the
    later frame is then sampled bilinearly at (x + dx, y + dy), and a pixel whose taps leave the frame or touch
    an invalid pixel is left out.  Without a flow the same pixel is compared — right for a static camera, an upper
    bound on flicker otherwise.  pair_mask: bool / uint8 [N − frame_step, H, W], pixels of frame i to use in pair i
    (an occlusion mask).  frames: the video's RGB frames ([N, 3, H, W] f16 / f32, or uint8 [N, H, W, 3], of pred's
    N, H and W) in place of a flow: the flow and its forward–backward mask are then estimated at this call's
    frame_step by rollingdepth_amd.flow.optical_flow with its defaults, the flow is used, and the mask is ANDed
    into pair_mask; frames together with a flow is a ValueError.  With no valid pixel at all every metric is
    NaN."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align: one of {ALIGN_MODES} expected, got {align!r}")
    if target is None and align != "none":
        raise ValueError(f"align: without a target only 'none' is possible, got {align!r}")
    clip_lo, clip_hi = _space_and_clip(space, clip)
    if isinstance(frame_step, bool) or not isinstance(frame_step, int):
        raise TypeError(f"frame_step: an int expected, got {type(frame_step).__name__}")
    for t, name, dtypes, what in ((flow, "flow", (torch.float32,), "float32"),
                                  (pair_mask, "pair_mask", (torch.bool, torch.uint8), "bool or uint8")):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a tensor expected, got {type(t).__name__}")
        if t.dtype not in dtypes:
            raise TypeError(f"{name}: {what} expected, got {t.dtype}")
    if frames is not None and flow is not None:
        raise ValueError("frames: give the frames or a flow, not both (the flow would be estimated from the frames)")

    def pair_checks(shape):
        N, H, W = shape
        if frames is not None:
            from .flow import check_flow_args

            if check_flow_args(frames, frame_step)[:3] != (N, H, W):
                raise ValueError(f"frames: shape {tuple(frames.shape)} does not match pred's N, H, W = {(N, H, W)}")
        if not 1 <= frame_step < N:
            raise ValueError(f"frame_step: 1 <= frame_step < N = {N} expected, got {frame_step}")
        pairs = N - frame_step
        if flow is not None and tuple(flow.shape) != (pairs, H, W, 2):
            raise ValueError(f"flow: shape {tuple(flow.shape)} does not match [N - frame_step, H, W, 2] = "
                             f"{(pairs, H, W, 2)}")
        if pair_mask is not None and tuple(pair_mask.shape) not in ((pairs, H, W), (pairs, 1, H, W)):
            raise ValueError(f"pair_mask: shape {tuple(pair_mask.shape)} does not match [N - frame_step, H, W] = "
                             f"{(pairs, H, W)}")

    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range, pair_checks)
    from . import kernels as K

    N, P = p.shape
    H, W = pred.shape[-2], pred.shape[-1]
    pairs, dev = N - frame_step, p.device
    fl = None if flow is None else flow.to(dev).contiguous()
    pm = None
    if pair_mask is not None:
        pm = pair_mask.to(dev).contiguous().view(pairs, P)
        if pm.dtype == torch.bool:
            pm = pm.view(torch.uint8)
    if frames is not None:
        from .flow import optical_flow

        est = optical_flow(frames.to(dev), frame_step)
        fl, valid = est.flow, est.valid.view(pairs, P)
        pm = valid if pm is None else ((pm != 0) & (valid != 0)).view(torch.uint8)
    sp = K.DEPTH_SPACES[space]
    ws = K.depth_metrics_workspace(N, P, dev)  # the moments' N rows; the temporal pass needs N − frame_step
    if align != "none":
        K.depth_moments(p, g, m, lo, hi, ws, space=sp)
    _, st = K.depth_fit(ws if align != "none" else None, N, P, K.DEPTH_FIT_MODES[align], device=dev)
    sums = K.depth_temporal(p, g, m, fl, pm, st, H, W, frame_step, lo, hi, sp, clip_lo, clip_hi, ws)
    st = st.cpu()
    return _pool_temporal(sums.cpu(), st[:, 0].contiguous(), st[:, 1].contiguous(), frame_step, g is not None)


# numpy.linspace(1.05, 1.25, 10), bit for bit
DEFAULT_BOUNDARY_THRESHOLDS = tuple(1.05 + (1.25 - 1.05) * i / 9 for i in range(9)) + (1.25,)
MAX_BOUNDARY_THRESHOLDS = 16  # RDMI_BOUNDARY_MAX_THRESHOLDS


@dataclass
class BoundaryMetrics:
    """Pooled over all frames with a fit: the integer counts are added over the frames, then, per threshold τ,
    precision(τ) = ¼ Σ_k TP_k / max(NP_k, 1) and recall(τ) = ¼ Σ_k TP_k / max(NG_k, 1) over the four directions
    k = R, L, D, U, f1(τ) = 2PR / (P + R) (0 when P + R = 0); the scalars are the per-threshold values weighted by
    τ_m / Σ τ.  With no valid pair at all every float field is NaN."""
    f1: float
    precision: float
    recall: float
    f1_per_threshold: torch.Tensor         # f64 [M], host
    precision_per_threshold: torch.Tensor  # f64 [M], host
    recall_per_threshold: torch.Tensor     # f64 [M], host
    thresholds: torch.Tensor               # f64 [M], host
    counts: torch.Tensor   # int64 [N, M, 4, 3], host: TP, NP, NG per frame, threshold and direction R, L, D, U
    pairs: torch.Tensor    # int64 [N, 2], host: valid horizontal and vertical pairs per frame
    n_pairs: int
    scale: torch.Tensor    # f64 [N], host
    shift: torch.Tensor    # f64 [N], host
    frames_skipped: List[int]  # frames without a fit (NaN scale / shift): their count rows are zero
    edges: Optional[torch.Tensor]  # uint8 [N, H, W] on the device, or None


def _boundary_thresholds(thresholds, edge_threshold) -> Tuple[List[float], int]:
    """The checks of boundary_metrics' thresholds → (the thresholds as floats, the index of edge_threshold)."""
    if thresholds is None:
        tau = list(DEFAULT_BOUNDARY_THRESHOLDS)
    else:
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.tolist()
        try:
            seq = list(thresholds)
        except TypeError:
            raise TypeError(f"thresholds: a sequence of numbers expected, got {type(thresholds).__name__}") from None
        for v in seq:
            if isinstance(v, bool) or not isinstance(v, (int, float)) and not hasattr(v, "__float__"):
                raise TypeError(f"thresholds: numbers expected, got {type(v).__name__}")
        tau = [float(v) for v in seq]
    if not 1 <= len(tau) <= MAX_BOUNDARY_THRESHOLDS:
        raise ValueError(f"thresholds: 1 to {MAX_BOUNDARY_THRESHOLDS} values expected, got {len(tau)}")
    for i, v in enumerate(tau):
        if not (math.isfinite(v) and v > 1.0):
            raise ValueError(f"thresholds: finite values > 1 expected, got {v} at {i}")
        if i and not v > tau[i - 1]:
            raise ValueError(f"thresholds: a strictly increasing sequence expected, got {v} after {tau[i - 1]}")
    if edge_threshold is None:
        return tau, len(tau) // 2
    if isinstance(edge_threshold, bool) or not isinstance(edge_threshold, (int, float)):
        raise TypeError(f"edge_threshold: a number expected, got {type(edge_threshold).__name__}")
    if float(edge_threshold) not in tau:
        raise ValueError(f"edge_threshold: one of the thresholds {tau} expected, got {edge_threshold}")
    return tau, tau.index(float(edge_threshold))


def _pool_boundary(counts: torch.Tensor, pairs: torch.Tensor, tau: List[float], scale: torch.Tensor,
                   shift: torch.Tensor, edges: Optional[torch.Tensor]) -> BoundaryMetrics:
    """Host tensors (int64 [N, M, 4, 3] counts, int64 [N, 2] pairs, f64 [N] scale / shift) → BoundaryMetrics: integer
    sums over the frames, then the few f64 divisions in threshold and direction order."""
    M = len(tau)
    tot = counts.sum(0).tolist()  # int64: exact in any order
    n_pairs = int(pairs.sum())
    skipped = [f for f, (s, t) in enumerate(zip(scale.tolist(), shift.tolist())) if math.isnan(s) or math.isnan(t)]
    nan = math.nan
    P, R, F = [nan] * M, [nan] * M, [nan] * M
    f1 = precision = recall = nan
    if n_pairs > 0:
        tau_sum = 0.0
        for v in tau:
            tau_sum += v
        f1 = precision = recall = 0.0
        for m in range(M):
            p = r = 0.0
            for k in range(4):
                tp, npred, ngt = tot[m][k]
                p += tp / max(npred, 1)
                r += tp / max(ngt, 1)
            P[m], R[m] = 0.25 * p, 0.25 * r
            F[m] = 2.0 * P[m] * R[m] / (P[m] + R[m]) if P[m] + R[m] > 0.0 else 0.0
            w = tau[m] / tau_sum
            f1 += w * F[m]
            precision += w * P[m]
            recall += w * R[m]
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    return BoundaryMetrics(f1=f1, precision=precision, recall=recall, f1_per_threshold=f64(F),
                           precision_per_threshold=f64(P), recall_per_threshold=f64(R), thresholds=f64(tau),
                           counts=counts, pairs=pairs, n_pairs=n_pairs, scale=scale, shift=shift,
                           frames_skipped=skipped, edges=edges)


def boundary_metrics(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                     align: str = "video", space: str = "depth", valid_range=(1e-3, math.inf),
                     clip: Optional[Tuple[float, float]] = None, thresholds=None, return_edges: bool = False,
                     edge_threshold: Optional[float] = None) -> BoundaryMetrics:
    """Precision, recall and F1 of the occlusion boundaries of the aligned prediction against the target's — after
    Depth Pro's scale-invariant boundary F1, restated from its definition.

    pred, target, mask, align, space, valid_range and clip as for depth_metrics: the fit is the one depth_metrics takes
    and a = clamp(φ⁻¹(scale·pred + shift)) is its aligned prediction.  A pixel counts when it is valid by
    depth_metrics' rule and its a is finite and > 0 (floor with clip where the fit can go negative).  Pixel i has an
    edge of a map d in direction R, L, D or U at threshold τ when its neighbour j there is also a valid pixel of the
    frame and d(j) > τ·d(i): i is the near side of a depth ratio above τ, whatever the scale of d.  TP, NP and NG
    count the pixels with an edge of both maps, of a, and of the target, per frame, threshold and direction.

    Matching is pixel-exact: a contour of the prediction displaced by one pixel from the target's is a miss in both
    precision and recall; there is no distance tolerance.

    thresholds: strictly increasing, 1 to 16 finite values > 1; default numpy.linspace(1.05, 1.25, 10).
    return_edges: also return the per-pixel edge map (uint8 [N, H, W] on the device; bits 0–3 the edge of a in R, L,
    D, U, bits 4–7 the target's, 0 for a pixel that does not count) at edge_threshold, which must be one of the
    thresholds and defaults to the middle one, thresholds[M // 2].  Frames without a fit are left out and listed in
    frames_skipped.  All counting runs in librdmi (rdmi_depth_boundary: integers only, so the same inputs give the same
    result on every call); this function adds the frames' integers and takes the last divisions in f64."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align: one of {ALIGN_MODES} expected, got {align!r}")
    clip_lo, clip_hi = _space_and_clip(space, clip)
    if not isinstance(return_edges, bool):
        raise TypeError(f"return_edges: a bool expected, got {type(return_edges).__name__}")
    tau, edge_index = _boundary_thresholds(thresholds, edge_threshold)
    if target is None:
        raise TypeError("target: a tensor expected, got NoneType")
    p, g, m, lo, hi = _prepare(pred, target, mask, valid_range)
    from . import kernels as K

    N, P = p.shape
    H, W = pred.shape[-2], pred.shape[-1]
    sp = K.DEPTH_SPACES[space]
    ws = None
    if align != "none":
        ws = K.depth_moments(p, g, m, lo, hi, space=sp)
    _, st = K.depth_fit(ws, N, P, K.DEPTH_FIT_MODES[align], device=p.device)
    counts, pairs, edges = K.depth_boundary(p, g, m, st, H, W, tau, lo, hi, sp, clip_lo, clip_hi,
                                            edge_index if return_edges else None)
    st = st.cpu()
    return _pool_boundary(counts.cpu(), pairs.cpu(), tau, st[:, 0].contiguous(), st[:, 1].contiguous(), edges)
