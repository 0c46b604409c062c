"""DepthAligner — drop-in for rollingdepth/depth_aligner.py:29-262 running on librdmi.

Same constructor keywords, same `run(snippet_ls, dilations)` contract (plus `strides`, which the
reference's pipeline refuses above 1) and return value
(merged [N,1,H,W] in the snippets' dtype, scales / translations as [n_d,1,1] f32, loss history
as a list of (loss, min(summ), max(summ)) tuples).  The 2000-iteration Adam loop is enqueued
entirely on the device (aligner.hip, merge.hip); the only host sync is reading the loss history at the end.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import kernels as K


MAX_DILATIONS = 8   # csrc/aligner_job.h MAXD
MAX_ROWS = 64       # csrc/aligner_job.h MAXR: Σ snippet lengths (rows of the reference's M / M_depth / B tensors)


def snippet_last(seq_len: int, length: int, dilation: int) -> int:
    """Start of the last window of `length` frames, `dilation` apart, in seq_len frames (csrc/aligner_index.h)."""
    return seq_len - ((length - 1) * dilation + 1)


def snippet_count(seq_len: int, length: int, dilation: int, start_step: int = 1) -> int:
    """Snippets get_snippet_indice yields with stride = start_step: range(0, last + 1, start_step), plus
    the last window when the range misses it (rollingdepth_pipeline.py:465-502)."""
    last = snippet_last(seq_len, length, dilation)
    if last < 0 or start_step < 1:
        raise ValueError(f"no snippet of length {length}, dilation {dilation}, start step {start_step} in "
                         f"{seq_len} frames")
    return last // start_step + 1 + (1 if last % start_step else 0)


def snippet_start(k: int, seq_len: int, length: int, dilation: int, start_step: int = 1) -> int:
    """First frame of snippet k."""
    return min(k * start_step, snippet_last(seq_len, length, dilation))


def check_row_layout(lengths: List[int], num_iterations: int) -> None:
    """The reference scatters dilation i's slots into rows i·w_i .. i·w_i + w_i − 1 of [Σw, N, P]
    tensors (depth_aligner.py:169-188); rows past Σw raise its IndexError (first closure call).
    Also the limits of the aligner kernels (at most 8 dilations, at most 64 rows), checked here so
    that forward() / sharded_forward() reject such a job before any inference runs rather than at
    the aligner call after it."""
    rows = sum(lengths)
    if len(lengths) > MAX_DILATIONS:
        raise NotImplementedError(f"{len(lengths)} dilations: the aligner kernels take at most {MAX_DILATIONS}")
    if num_iterations > 0:
        for i, w in enumerate(lengths):
            if (i + 1) * w > rows:
                raise IndexError(f"index {(i + 1) * w - 1} is out of bounds for dimension 0 with size {rows}")
        if rows > MAX_ROWS:
            raise NotImplementedError(f"snippet lengths {list(lengths)} sum to {rows} aligner rows: the aligner "
                                      f"kernel takes at most {MAX_ROWS}")


class DepthAligner:
    def __init__(self, device: torch.device, factor: int = 10, lmda: float = 1e-1, lmda2: float = 1e-1,
                 lmda3: float = 1e1, lr: float = 1e-3, num_iterations: int = 2000, border: int = 2,
                 verbose: bool = False, depth_loss_weight: float = 1.0, loss_scale=1.0):
        self.factor = factor
        self.lmda = lmda  # kept for signature parity; unused by the reference loss too
        self.lr = lr
        self.num_iterations = num_iterations
        self.border = border
        self.verbose = verbose
        self.device = device
        self.lmda2 = lmda2
        self.depth_loss_weight = depth_loss_weight
        self.loss_scale = loss_scale
        self.lmda3 = lmda3

    def create_triplet_indices(self, sequence_length: int, gap: int, window_size: int, stride: int = 1) -> torch.Tensor:
        """depth_aligner.py:57-66; stride: frames between snippet starts (get_snippet_indice's)."""
        gap += 1
        n = snippet_count(sequence_length, window_size, gap, stride)
        starts = [snippet_start(k, sequence_length, window_size, gap, stride) for k in range(n)]
        return torch.tensor([[i + j * gap for j in range(window_size)] for i in starts])

    @staticmethod
    def sequence_length(counts: List[int], w: int, dilations: List[int]) -> int:
        """depth_aligner.py:70-76 (from the first dilation's snippet count)."""
        return counts[0] + (w - 1) * (dilations[0] - 1) + (w - 1)

    def prepare(self, flat: List[torch.Tensor], shift: torch.Tensor) -> List[torch.Tensor]:
        """Min shift, border crop, stride subsample (:78-92): [n_d, w, H, W] → f32 [n_d, w, P]."""
        return [K.aligner_prepare(s, shift, self.border, self.factor) for s in flat]

    def optimize_prepared(self, xs: List[torch.Tensor], strides: List[int], seq_len: int,
                          start_steps: Optional[List[int]] = None):
        """The 2000-iteration Adam loop (:123-229) on prepared inputs → (scales [n_d], trans [n_d],
        history [iters, 3] device tensor, workspace to keep alive until the stream consumed it).
        strides: the frame step inside a snippet (the dilations); start_steps: frames between snippet
        starts per dilation (None: 1)."""
        dev = xs[0].device
        scales = [torch.ones(x.shape[0], dtype=torch.float32, device=dev) for x in xs]
        trans = [torch.zeros(x.shape[0], dtype=torch.float32, device=dev) for x in xs]
        hist = torch.zeros((max(self.num_iterations, 1), 3), dtype=torch.float32, device=dev)
        ws = K.aligner_optimize(xs, scales, trans, strides, seq_len, self.lr, (0.5, 0.9), 1e-8, self.lmda2,
                                self.lmda3, self.depth_loss_weight, self.loss_scale, self.num_iterations, hist,
                                start_steps=start_steps)
        return scales, trans, hist, ws

    def run(self, snippet_ls: List[torch.Tensor], dilations: List[int], strides: Optional[List[int]] = None,
            sequence_length: Optional[int] = None, merged_f32: bool = False, uncertainty: bool = False,
            merge: str = "mean"):
        """depth_aligner.py:68-120.  merged_f32=True (the pipeline's internal use): the merge of f16
        snippets runs in f32 arithmetic and is returned in f32, without the reference's f16 roundings
        of s·x+t and of the merged map (RollingDepthPipeline.merge_f32).

        Snippet lengths may differ per dilation (snippet_ls[d] is [n_d, w_d, 1, H, W]): the sequence
        length comes from the first dilation (:70-76) and the loss uses the reference's row layout
        (row i·w_i + j for slot j of dilation i, :169-188 — see aligner.hip), including its
        IndexError when those rows run past Σ w_i.

        strides (one per dilation, or one for all): the snippets of a dilation start that many frames
        apart, plus the last window (get_snippet_indice's `stride`).  sequence_length is then required —
        a snippet count no longer determines it.  Without strides everything is as above.

        uncertainty=True (the build's own): the merge also keeps how far the merged terms lie apart
        (kernels.aligner_merge_moments in place of aligner_merge, same merged map bitwise) and a fifth
        element is returned: the per-pixel population standard deviation of a frame's covering terms
        s·(x − min) + t, [N, 1, H, W] f32 in the units of the merged map before any renormalisation, 0
        where fewer than two snippets cover a frame.

        merge="median" (the build's own; "mean" | "median", anything else is a ValueError): the merged map is
        the per-pixel median of a frame's covering terms instead of their mean (kernels.aligner_merge_median;
        the mean of the two middle terms for an even count), and the fifth element under uncertainty=True is
        their median absolute deviation around it — the raw MAD, no 1.4826 factor.  Scales, translations and
        the loss history are the same."""
        if not isinstance(uncertainty, bool):
            raise TypeError(f"uncertainty must be a bool, got {type(uncertainty).__name__}")
        if not isinstance(merge, str) or merge not in ("mean", "median"):
            raise ValueError(f'merge must be "mean" or "median", got {merge!r}')
        dev = torch.device(self.device)
        snippet_ls = [s.to(dev) for s in snippet_ls]
        lengths = [s.shape[1] for s in snippet_ls]
        gaps = [d - 1 for d in dilations]
        start_steps = None
        if strides is None:
            seq_len = self.sequence_length([s.shape[0] for s in snippet_ls], lengths[0], dilations)
            if sequence_length is not None and sequence_length != seq_len:
                raise ValueError(f"sequence_length {sequence_length} != {seq_len} from the first dilation's snippets")
        else:
            if sequence_length is None:
                raise ValueError("strides need sequence_length: a snippet count does not determine it")
            start_steps = [int(v) for v in strides] * (len(dilations) if len(strides) == 1 else 1)
            if len(start_steps) != len(dilations) or min(start_steps) < 1:
                raise ValueError(f"strides {list(strides)}: one int >= 1 per dilation expected")
            seq_len = int(sequence_length)
        for i, (s, g, w) in enumerate(zip(snippet_ls, gaps, lengths)):
            expect = snippet_count(seq_len, w, g + 1, start_steps[i] if start_steps else 1)
            if s.shape[0] != expect:
                raise ValueError(f"snippet count {s.shape[0]} != {expect} for dilation {g + 1} (length {w})")
        check_row_layout(lengths, self.num_iterations)
        dtype = snippet_ls[0].dtype
        flat = [s.reshape(s.shape[0], s.shape[1], s.shape[-2], s.shape[-1]).contiguous() for s in snippet_ls]
        # global min over every snippet (depth_aligner.py:78)
        mins = torch.stack([K.minmax(s) for s in flat]).reshape(-1)
        shift = K.minmax(mins)
        xs = self.prepare(flat, shift)
        frame_steps = [g + 1 for g in gaps]
        scales, trans, hist, ws = self.optimize_prepared(xs, frame_steps, seq_len, start_steps)
        spread = None
        if merge == "median":
            merged = K.aligner_merge_median(flat, scales, trans, frame_steps, seq_len, shift, f32_arith=merged_f32,
                                            start_steps=start_steps, mad=uncertainty)
            if uncertainty:
                merged, spread = merged
        elif uncertainty:
            merged, spread = K.aligner_merge_moments(flat, scales, trans, frame_steps, seq_len, shift,
                                                     f32_arith=merged_f32, start_steps=start_steps)
        else:
            merged = K.aligner_merge(flat, scales, trans, frame_steps, seq_len, shift, f32_arith=merged_f32,
                                     start_steps=start_steps)
        merged = (merged if merged_f32 else merged.to(dtype))[:, None]
        loss_ls = [tuple(r) for r in hist[: self.num_iterations].tolist()]
        del ws
        res = (merged, [s.view(-1, 1, 1) for s in scales], [t.view(-1, 1, 1) for t in trans], loss_ls)
        return res + (spread[:, None],) if uncertainty else res
