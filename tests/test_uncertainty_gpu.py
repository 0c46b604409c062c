"""The merge's per-pixel spread on the device: rdmi_aligner_merge_moments and its sharded forms against the
numpy reference and derived tolerance of tests/uncertainty_util.py and against the existing merge (the mean
must not move by a bit), rdmi_scale_spread_f32, and depth_uncertainty through RollingDepthPipeline.forward
and shard.sharded_forward.  Layouts as in tests/test_shard_strided_gpu.py plus the start-step-1 layout:
  L-on   N = 23, dilations (1, 4, 7), lengths (3, 2, 2), start steps (2, 3, 5): 11 / 7 / 4 snippets
  L-off  the same geometry, start steps (3, 4, 2): 8 / 6 / 9, every last window off the start grid
  L-gap  N = 14, dilation (1), length (3), start step (4): frames 3 and 7 in no snippet, every other in one
  L-one  the same geometry as L-on, start steps (1, 1, 1): 21 / 19 / 16 snippets, up to 7 terms per pixel
Frame sizes: 24·20 = 480 (4 pixels per lane), 23·19 = 437 (odd: one pixel per lane, rows not 16-byte
aligned), 22·22 = 484 (4 pixels per lane, a partial last wave), 1·3."""
import json
import os
import socket

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from tests import uncertainty_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")

LAYOUTS = {"on": (23, (1, 4, 7), (3, 2, 2), (2, 3, 5), (11, 7, 4)),
           "off": (23, (1, 4, 7), (3, 2, 2), (3, 4, 2), (8, 6, 9)),
           "gap": (14, (1,), (3,), (4,), (4,)),
           "one": (23, (1, 4, 7), (3, 2, 2), (1, 1, 1), (21, 19, 16))}
SHAPES = [(24, 20), (23, 19), (22, 22), (1, 3)]
MODES = [0, 1, 2]  # rdmi.h x_f32: f16 snippets in the f16 chain, f32 snippets, f16 snippets in f32 arithmetic

_JOBS = {}


def _offset_copy(x, elems):
    """x in a buffer that starts `elems` elements into an allocation (data_ptr off the 16-byte grid)."""
    buf = torch.empty(x.numel() + elems, dtype=x.dtype, device=x.device)
    v = buf[elems:].view(x.shape)
    v.copy_(x)
    return v


def _job(layout, mode, hw, offset=False):
    """Snippets, scales, translations and min shift of one case (device tensors), the existing merge of them,
    and the reference spread with its tolerance — computed once per case and shared, never written to."""
    key = (layout, mode, hw, offset)
    if key not in _JOBS:
        from rollingdepth_amd import kernels as K

        N, dil, w, ss, counts = LAYOUTS[layout]
        H, W = hw
        rng = np.random.default_rng(3)
        base = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
        xn, sn, tn = [], [], []
        for d, wd, s in zip(dil, w, ss):
            st = U.starts(N, wd, d, s)
            x = np.stack([np.stack([base[q + j * d] for j in range(wd)]) for q in st])
            x = x * (0.5 + rng.uniform(0, 1, (len(st), 1, 1, 1))) + 0.3 * rng.standard_normal((len(st), 1, 1, 1))
            xn.append(x.astype(np.float32 if mode == 1 else np.float16))
            sn.append((1 + 0.1 * rng.standard_normal(len(st))).astype(np.float32))
            tn.append((0.1 * rng.standard_normal(len(st))).astype(np.float32))
        assert tuple(x.shape[0] for x in xn) == counts
        xf = [torch.from_numpy(x).to(DEV) for x in xn]
        if offset:  # 4 bytes off: one f32 element, two f16 elements
            xf[0] = _offset_copy(xf[0], 1 if mode == 1 else 2)
            assert xf[0].data_ptr() % 16 == 4
        sc = [torch.from_numpy(s).to(DEV) for s in sn]
        tr = [torch.from_numpy(t).to(DEV) for t in tn]
        shift_v = min(float(x.astype(np.float32).min()) for x in xn)
        shift = torch.tensor([shift_v], dtype=torch.float32, device=DEV)
        merged = K.aligner_merge(xf, sc, tr, list(dil), N, shift, f32_arith=mode == 2,
                                 start_steps=None if layout == "one" else list(ss)).reshape(N, H * W)
        frames = U.frame_terms([x.reshape(x.shape[0], x.shape[1], -1) for x in xn], sn, tn, dil, ss, N,
                               shift.item(), mode)
        ref, tol, cnt = U.spread_reference(frames)
        _JOBS[key] = dict(xf=xf, sc=sc, tr=tr, shift=shift, merged=merged, ref=ref, tol=tol, cnt=cnt, N=N, dil=list(dil),
                          w=list(w), ss=list(ss), counts=list(counts), HW=H * W, mode=mode)
    return _JOBS[key]


def _check(j, mean, std, what, factor=1.0):
    """mean bitwise the existing merge; std within factor·tol of the reference; frames in no snippet are 0 in
    both, frames in one snippet have std exactly 0."""
    N, HW = j["N"], j["HW"]
    mean, std = mean.reshape(N, HW), std.reshape(N, HW)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32
    ratio, zeros = U.worst_ratio(std.cpu().numpy(), j["ref"], j["tol"] * factor)
    print(f"{what}: worst |std − ref| / tol = {ratio:.3f} (c up to {j['cnt'].max()})")
    assert torch.equal(mean, j["merged"])
    assert bool(torch.isfinite(std).all()) and bool((std >= 0).all())
    assert ratio <= 1.0 and zeros
    none, single = np.flatnonzero(j["cnt"] == 0), np.flatnonzero(j["cnt"] == 1)
    if len(none):
        assert not mean[none].any() and not std[none].any()
    if len(single):
        assert not std[single].any()
    if j["cnt"].max() > 1:
        assert j["ref"].max() > 0.01  # the case has a spread to measure


def _fused(j):
    from rollingdepth_amd import kernels as K

    return K.aligner_merge_moments(j["xf"], j["sc"], j["tr"], j["dil"], j["N"], j["shift"], f32_arith=j["mode"] == 2,
                                   start_steps=j["ss"])


# ------------------------------------------------------------------------------------------------ fused kernel
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
def test_fused_merge_mean_bitwise_and_std_within_tol(mode, layout, hw):
    """rdmi_aligner_merge_moments in every x_f32 mode, layout and frame size: the mean is torch.equal to
    rdmi_aligner_merge(_strided), the std within the derived tolerance of the longdouble two-pass reference.
    L-gap: frames 3 and 7 (no snippet) give mean 0 and std 0, every other frame lies in one snippet: std exactly 0."""
    j = _job(layout, mode, hw)
    mean, std = _fused(j)
    if layout == "gap":
        assert j["cnt"][[3, 7]].tolist() == [0, 0] and j["cnt"].max() == 1
    _check(j, mean, std, f"mode {mode} L-{layout} {hw[0]}x{hw[1]}")


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_merge_with_a_snippet_tensor_off_the_16_byte_grid(mode):
    """HW = 480 would take 4 pixels per lane, but dilation 0's snippets start 4 bytes into an allocation: the
    call must take the one-pixel path (a 16-byte load there would be misaligned) and give the same results."""
    j = _job("on", mode, (24, 20), offset=True)
    mean, std = _fused(j)
    _check(j, mean, std, f"mode {mode} L-on 24x20, snippets + 4 bytes")
    a = _job("on", mode, (24, 20))
    assert torch.equal(std.reshape(j["N"], -1), _fused(a)[1].reshape(j["N"], -1))


def test_identical_terms_have_exactly_zero_spread():
    """Every slot of a pixel holds the same f32 value, s = 1, t = 0, shift 0, up to 7 terms per pixel (L-one):
    Σa = c·a and Σa² = c·a² are exact in f64 (a² has 48 bits, c ≤ 32 five more), so are both quotients, and
    the std is exactly 0 — any rounding in the formula would show as ~1e-8·|a|."""
    from rollingdepth_amd import kernels as K

    N, dil, w, ss, counts = LAYOUTS["one"]
    H, W = 22, 22
    rng = np.random.default_rng(11)
    v = torch.from_numpy(rng.uniform(-3, 3, (H, W)).astype(np.float32)).to(DEV)
    xf = [v.expand(n, wd, H, W).contiguous() for n, wd in zip(counts, w)]
    sc = [torch.ones(n, device=DEV) for n in counts]
    tr = [torch.zeros(n, device=DEV) for n in counts]
    shift = torch.zeros(1, device=DEV)
    mean, std = K.aligner_merge_moments(xf, sc, tr, list(dil), N, shift, start_steps=list(ss))
    assert torch.equal(mean, v.expand(N, H, W))
    assert not std.any()
    cover = [sum(1 for d, wd in zip(dil, w) for j in range(wd) if 0 <= f - j * d <= N - ((wd - 1) * d + 1))
             for f in range(N)]
    assert max(cover) == 7 and min(cover) >= 2


# ------------------------------------------------------------------------------------------------ W ranks emulated
def _windowed(j, world):
    """W ranks emulated in one process, as tests/test_shard_strided_gpu.py::_windowed, over both moments:
    per-rank window sums [rows, 2, HW], the all-to-all of shard.merge_exchange_plan done by slicing, the
    finish per frame chunk → (mean [N, HW], std [N, HW], per-rank sums, per-rank frame ranges, pieces per rank)."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.shard import chunk_bounds, merge_exchange_plan, rank_subsets

    n, dil, w, N, HW, ss = j["counts"], j["dil"], j["w"], j["N"], j["HW"], j["ss"]
    sent, all_sums, all_ranges = [], [], []
    for r in range(world):
        sub = rank_subsets(n, world, r)
        k0 = [x[0] if x else 0 for x in sub]
        rows = [j["xf"][d][k0[d]:k0[d] + len(sub[d])] for d in range(len(n))]
        ranges, send, _ = merge_exchange_plan(n, dil, w, N, world, r, ss)
        sums = torch.cat([K.aligner_merge_partial_window_moments([x if x.shape[0] else None for x in rows], k0, n,
                                                                 j["sc"], j["tr"], dil, w, a, b - a, HW, j["shift"],
                                                                 j["mode"], N, start_steps=ss)
                          for a, b in ranges]) if ranges else torch.zeros((0, 2, HW), dtype=torch.float64, device=DEV)
        assert sums.shape == (sum(send), 2, HW)
        all_sums.append(sums)
        all_ranges.append(ranges)
        o, per_dst = 0, []
        for m in send:
            per_dst.append(sums[o:o + m])
            o += m
        sent.append(per_dst)
    means, stds, npieces = [], [], []
    for r in range(world):
        f0, f1 = chunk_bounds(N, world)[r]
        _, _, recv = merge_exchange_plan(n, dil, w, N, world, r, ss)
        rbuf = torch.cat([sent[s][r] for s in range(world)])
        pieces = [pc for src in recv for pc in src]
        m, s = K.aligner_merge_finish_pieces_moments(rbuf.contiguous(), pieces, n, dil, w, f0, f1 - f0, HW, N,
                                                     start_steps=ss)
        means.append(m)
        stds.append(s)
        npieces.append((f1 - f0, len(pieces)))
    return torch.cat(means), torch.cat(stds), all_sums, all_ranges, npieces


_WINDOWED = [(mode, world, (24, 20)) for mode in (1, 2) for world in (2, 3, 8, 24)] + \
            [(0, 2, (24, 20)), (0, 3, (24, 20))] + [(mode, 3, (23, 19)) for mode in MODES]


@pytest.mark.parametrize("mode,world,hw", _WINDOWED, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sharded_moments_emulated_ranks(layout, mode, world, hw):
    """rdmi_aligner_merge_partial_window_moments per rank, the plan's slicing, and
    rdmi_aligner_merge_finish_pieces_moments: means torch.equal to the single-GPU merge, stds within tol of
    the reference (not necessarily bitwise the fused kernel's: f64 sums of squares depend on the order of
    addition in rare cases).  24 ranks over 23 (14) frames leave a rank with an empty frame chunk and ranks
    that own no snippet."""
    j = _job(layout, mode, hw)
    mean, std, _, _, npieces = _windowed(j, world)
    if world == 24:
        assert npieces[-1][0] == 0  # the last rank's frame chunk is empty
    _check(j, mean, std, f"mode {mode} L-{layout} world {world} {hw[0]}x{hw[1]}")


@pytest.mark.parametrize("mode", [1, 2])
def test_finish_moments_splits_a_piece_table_wider_than_64(mode):
    """One receiver owns all 23 frames and gets every frame of 8 sources as a piece of its own: more pieces
    than the 64 of the kernel's table, so the library splits the call by frame range — each frame still adds
    its pieces in source order, and the result is that of the plan's few wide pieces."""
    from rollingdepth_amd import kernels as K

    j = _job("one", mode, (24, 20))
    mean, std, sums, ranges, _ = _windowed(j, 8)
    pieces = [(f, 1) for rg in ranges for a, b in rg for f in range(a, b)]
    assert len(pieces) > 64
    m1, s1 = K.aligner_merge_finish_pieces_moments(torch.cat(sums).contiguous(), pieces, j["counts"], j["dil"], j["w"],
                                                   0, j["N"], j["HW"], j["N"], start_steps=j["ss"])
    _check(j, m1, s1, f"mode {mode} L-one, {len(pieces)} one-frame pieces")
    assert torch.equal(s1, std) and torch.equal(m1, mean)


# ------------------------------------------------------------------------------------------------ scale_spread_
def test_scale_spread_bitwise():
    """x ← (x / (max − min)) · 2, each operation rounded once to f32: bitwise numpy's."""
    from rollingdepth_amd import kernels as K

    rng = np.random.default_rng(5)
    x = np.abs(rng.standard_normal(1001)).astype(np.float32) * np.float32(0.05)
    x[:3] = [0.0, 1e-30, 7.5]
    mm = np.array([-0.731, 2.219], np.float32)
    got = K.scale_spread_(torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(mm).to(DEV)).cpu().numpy()
    want = (x / (mm[1] - mm[0])).astype(np.float32) * np.float32(2.0)
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ pipeline
class _Spy:
    """Records the calls of the four uncertainty entry points of rollingdepth_amd.kernels while active: the
    arguments of aligner_merge_moments, copies of every raw (unscaled) std they return, and the min / max
    handed to scale_spread_ with its input."""
    NAMES = ("aligner_merge_moments", "aligner_merge_partial_window_moments", "aligner_merge_finish_pieces_moments",
             "scale_spread_")

    def __enter__(self):
        from rollingdepth_amd import kernels as K

        self.K, self.calls, self.merge_args, self.raw, self.scaled = K, [], [], [], []
        self.orig = {n: getattr(K, n) for n in self.NAMES}

        def wrap(name):
            def f(*a, **kw):
                self.calls.append(name)
                if name == "scale_spread_":
                    self.scaled.append((a[0].clone(), a[1].clone()))
                out = self.orig[name](*a, **kw)
                if name == "aligner_merge_moments":
                    self.merge_args.append((a, kw))
                if name in ("aligner_merge_moments", "aligner_merge_finish_pieces_moments"):
                    self.raw.append(out[1].clone())
                return out
            return f

        for n in self.NAMES:
            setattr(K, n, wrap(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.K, n, f)
        return False


_PIPES = {}


def _fixture_pipe(name, snippet_batch=8):
    if name not in _PIPES:
        from rollingdepth_amd.pipeline import RollingDepthPipeline

        t = load_file(os.path.join(G, name + ".safetensors"))
        meta = json.load(open(os.path.join(G, name + ".json")))
        pipe = RollingDepthPipeline.from_synthetic(meta["unet"], meta["vae"], meta["scheduler"], device="cuda")
        pipe.empty_text_embed = t["context"]
        _PIPES[name] = (t, meta, pipe)
    t, meta, pipe = _PIPES[name]
    pipe.snippet_batch = snippet_batch
    return t, meta, pipe


def _forward(pipe, t, meta, strides, refine_step, **kw):
    return pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], list(strides), None, refine_step,
                        3, meta.get("refine_start_dilation", 6), None, False, 4, False, init_noise=t["init_noise"], **kw)


def _reference_from_call(args, kw):
    """The reference spread, tolerance and cover counts from the arguments of one aligner_merge_moments call."""
    xf, sc, tr, dil, N, shift = args[:6]
    mode = 1 if xf[0].dtype == torch.float32 else (2 if kw.get("f32_arith") else 0)
    ss = kw.get("start_steps") or [1] * len(xf)
    xn = [x.cpu().numpy().reshape(x.shape[0], x.shape[1], -1) for x in xf]
    frames = U.frame_terms(xn, [s.cpu().numpy() for s in sc], [t.cpu().numpy() for t in tr], list(dil), list(ss), N,
                           shift[0].item(), mode)
    return U.spread_reference(frames)


def _scaled(raw, mm):
    """(raw / (max − min)) · 2 in numpy f32 from device tensors → numpy."""
    m = mm.cpu().numpy()
    return (raw.cpu().numpy() / (m[1] - m[0])).astype(np.float32) * np.float32(2.0)


@pytest.mark.parametrize("strides", [[1], [2, 1]], ids=["strides1", "strides21"])
def test_forward_output_uncertainty(strides):
    """tiny_pipeline (9 frames 32², dilations [1, 3] capped to [1, 2]).  The default forward calls no _moments
    entry point and returns depth_uncertainty None; forward(output_uncertainty=True) returns depth_pred,
    depth_coaligned and snippet_ls bitwise the default's, and an f32, finite, non-negative depth_uncertainty
    whose unscaled form is within tol of the reference computed from the arguments captured at the
    kernels.aligner_merge_moments call, and which is bitwise that form scaled by the captured min / max."""
    t, meta, pipe = _fixture_pipe("tiny_pipeline")
    with _Spy() as spy0:
        base = _forward(pipe, t, meta, strides, 0)
    assert spy0.calls == [] and base.depth_uncertainty is None
    with _Spy() as spy:
        out = _forward(pipe, t, meta, strides, 0, output_uncertainty=True)
    assert spy.calls == ["aligner_merge_moments", "scale_spread_"]
    assert torch.equal(out.depth_pred, base.depth_pred) and torch.equal(out.depth_coaligned, base.depth_coaligned)
    assert len(out.snippet_ls) == len(base.snippet_ls)
    assert all(torch.equal(a, b) for a, b in zip(out.snippet_ls, base.snippet_ls))
    unc = out.depth_uncertainty
    N, _, H, W = base.depth_pred.shape
    assert unc.dtype == torch.float32 and tuple(unc.shape) == (N, 1, H, W) and not unc.is_cuda
    assert bool(torch.isfinite(unc).all()) and bool((unc >= 0).all()) and unc.max().item() > 0
    args, kw = spy.merge_args[0]
    assert (kw.get("start_steps") is not None) == (strides != [1])
    ref, tol, cnt = _reference_from_call(args, kw)
    ratio, zeros = U.worst_ratio(spy.raw[0].cpu().numpy().reshape(N, H * W), ref, tol)
    print(f"tiny_pipeline strides {strides}: worst |std − ref| / tol = {ratio:.3f}, c {cnt.min()} … {cnt.max()}, "
          f"uncertainty mean {unc.mean().item():.3e} max {unc.max().item():.3e}")
    assert ratio <= 1.0 and zeros
    raw_in, mm = spy.scaled[0]
    assert torch.equal(raw_in.reshape(-1), spy.raw[0].reshape(-1))
    assert np.array_equal(unc.numpy().reshape(-1).view(np.uint32), _scaled(raw_in, mm).reshape(-1).view(np.uint32))


def test_forward_output_uncertainty_describes_the_coaligned_stage_under_refine():
    """tiny_refine (refine_step 2): depth_uncertainty is present and equals that of the same run without
    refine, bitwise; depth_pred is the refined one (bitwise the default refine forward's)."""
    t, meta, pipe = _fixture_pipe("tiny_refine")
    base = _forward(pipe, t, meta, [1], meta["refine_step"])
    refined = _forward(pipe, t, meta, [1], meta["refine_step"], output_uncertainty=True)
    plain = _forward(pipe, t, meta, [1], 0, output_uncertainty=True)
    assert base.depth_uncertainty is None
    assert refined.depth_uncertainty is not None and refined.depth_uncertainty.dtype == torch.float32
    assert torch.equal(refined.depth_uncertainty, plain.depth_uncertainty)
    assert torch.equal(refined.depth_pred, base.depth_pred) and torch.equal(refined.depth_coaligned, plain.depth_pred)
    assert not torch.equal(refined.depth_pred, plain.depth_pred)


def test_call_restore_res_resizes_depth_uncertainty():
    """__call__(restore_res=True, output_uncertainty=True) on decoded uint8 frames (as
    tests/test_video_gpu.py::test_call_with_decoded_frames_and_restore_res): depth_uncertainty comes back at
    the video's resolution, f32 — the processing-resolution map resized as depth_pred is (rdmi_resize: ≤ 1e-5
    relative against F.interpolate, that test file's bound) — and the default call has none."""
    import torch.nn.functional as F

    from rollingdepth_amd import config as C
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    pipe = RollingDepthPipeline.from_synthetic(C.TINY_UNET, C.TINY_VAE, C.RD_SCHEDULER, device="cuda")
    fr = np.random.default_rng(1).integers(0, 256, (9, 45, 60, 3), dtype=np.uint8)
    kw = dict(dilations=[1, 3], cap_dilation=True, snippet_lengths=[3], init_infer_steps=[1], strides=[1],
              coalign_kwargs={"num_iterations": 50}, refine_step=0, processing_res=32)
    h, w = pipe.vae.latent_hw(24, 32)  # 45×60 at processing_res 32 → 24×32
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(3))
    small = pipe(fr, init_noise=noise, output_uncertainty=True, **kw)
    out = pipe(fr, restore_res=True, init_noise=noise, output_uncertainty=True, **kw)
    assert pipe(fr, restore_res=True, init_noise=noise, **kw).depth_uncertainty is None
    assert tuple(small.depth_uncertainty.shape) == (9, 1, 24, 32)
    assert tuple(out.depth_uncertainty.shape) == (9, 1, 45, 60) and out.depth_uncertainty.dtype == torch.float32
    assert out.depth_pred.shape[-2:] == (45, 60)
    want = F.interpolate(small.depth_uncertainty, size=[45, 60], mode="bilinear", align_corners=False, antialias=True)
    d = ((out.depth_uncertainty - want).abs().max() / want.abs().max()).item()
    print(f"restore_res depth_uncertainty rel {d:.2e}")
    assert d <= 1e-5, d


# ------------------------------------------------------------------------------------------------ sharded
def _worker(rank, world, port, strides, res):
    """One of `world` ranks on the one GPU (gloo).  res: [0] sharded depth_pred bitwise the single-GPU one,
    [1] worst |sharded − single-GPU| unscaled std / (2·tol), [2] worst |sharded − reference| / tol,
    [3] depth_uncertainty_full bitwise the gathered unscaled std scaled by the all-reduced min / max,
    [4] this rank's chunk has the right shape and dtype (summed over the ranks), [5] the calls made."""
    import torch.distributed as dist
    from rollingdepth_amd.shard import _all_gather_rows, chunk_bounds, sharded_forward

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t, meta, pipe = _fixture_pipe("tiny_pipeline", 3)
    N = t["frames"].shape[0]
    with _Spy() as spy:
        so = sharded_forward(pipe, t["frames"][None].cuda(), list(meta["dilations_in"]), True, 3, None,
                             init_noise=t["init_noise"].cuda(), gather=True, strides=list(strides),
                             output_uncertainty=True)
        torch.cuda.synchronize()
    f0, f1 = chunk_bounds(N, world)[rank]
    H, W = so.depth_pred.shape[-2:]
    ok = torch.tensor([float(so.depth_uncertainty.dtype == torch.float32 and
                             tuple(so.depth_uncertainty.shape) == (f1 - f0, 1, H, W) and
                             spy.calls.count("aligner_merge_finish_pieces_moments") == 1 and
                             "aligner_merge_moments" not in spy.calls)])
    dist.all_reduce(ok)
    raw_full = _all_gather_rows(spy.raw[0], N, world)
    dist.barrier()
    if rank == 0:
        with _Spy() as one:
            pipe.snippet_batch = 8
            out = _forward(pipe, t, meta, strides, 0, output_uncertainty=True)
        ref, tol, _ = _reference_from_call(*one.merge_args[0])
        single = one.raw[0].cpu().numpy().reshape(N, H * W).astype(np.longdouble)
        got = raw_full.cpu().numpy().reshape(N, H * W)
        res[0] = float(torch.equal(so.depth_pred_full.cpu(), out.depth_pred))
        res[1] = U.worst_ratio(got, single, 2 * tol)[0]
        res[2] = U.worst_ratio(got, ref, tol)[0]
        want = _scaled(raw_full, spy.scaled[0][1]) if spy.scaled else None
        res[3] = float(want is not None and np.array_equal(
            so.depth_uncertainty_full.cpu().numpy().reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32)))
        res[4] = ok.item()
        res[5] = float(torch.equal(so.depth_uncertainty_full.cpu(), out.depth_uncertainty))
        print(f"tiny_pipeline strides {list(strides)} world {world}: depth_pred bitwise {res[0]:.0f}; unscaled std "
              f"sharded vs single-GPU / (2·tol) {res[1]:.3f}, vs reference / tol {res[2]:.3f}; scaled bitwise "
              f"{res[3]:.0f}; equal to the single-GPU depth_uncertainty {res[5]:.0f}")
    dist.destroy_process_group()


@pytest.mark.parametrize("strides,world", [((1, 1), 2), ((1, 1), 3), ((2, 1), 2)])
def test_sharded_forward_output_uncertainty(strides, world):
    """sharded_forward(output_uncertainty=True) over 2 and 3 ranks on the one GPU (collectives over gloo, every
    child under its own time limit): depth_pred is bitwise the single-GPU forward's, the unscaled spread within
    2·tol of the single-GPU one (each is within tol of the reference), depth_uncertainty_full is that spread
    scaled by the all-reduced min / max, every rank's chunk is [f1 − f0, 1, H, W] f32."""
    import torch.multiprocessing as mp

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    res = ctx.Array("d", [0.0, 9.0, 9.0, 0.0, 0.0, 0.0])
    procs = [ctx.Process(target=_worker, args=(r, world, port, list(strides), res)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not any(alive) and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    res = list(res)
    assert res[0] == 1.0 and res[1] <= 1.0 and res[2] <= 1.0 and res[3] == 1.0 and res[4] == world, res
