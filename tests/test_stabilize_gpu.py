"""rdmi_temporal_filter on the device against the f64 restatement of tests/stabilize_util.py, its bitwise properties,
the public temporal_filter with its flow chain, its effect on flicker, and the pipeline's stabilize option."""
import math

import pytest
import torch

from tests import stabilize_util as U

pytestmark = pytest.mark.gpu
F16, F32 = U.F16, U.F32


def _dev(t):
    return None if t is None else t.cuda()


def _run(depth, flow, valid, R, st=U.SIGMA_TIME, sd=U.SIGMA_DEPTH, **kw):
    from rollingdepth_amd import kernels as K

    return K.temporal_filter(_dev(depth), _dev(flow), _dev(valid), R, st, sd, **kw)


def _same(a, b):
    """Bitwise equal, NaN pixels included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


@pytest.mark.parametrize("ci,dt", U.all_gpu_variants())
def test_device_matches_the_f64_restatement(ci, dt):
    """|device − f64| ≤ TOL_REL · tap_range at every pixel; the NaN pixel is NaN and nothing else is."""
    N, H, W, R = U.GPU_CASES[ci]
    depth, flow, valid = U.gpu_inputs(ci, dt)
    ref, rng = U.gpu_reference(ci, dt)
    got = _run(depth, flow, valid, R).cpu()
    assert got.shape == (N, H, W) and got.dtype == F32
    fn, yn, xn = U.nan_pixel(ci)
    assert torch.isnan(got[fn, yn, xn]) and int(torch.isnan(got).sum()) == 1
    q = U.ratio(got, ref, rng)
    fin = torch.isfinite(ref)
    med = ((got.double() - ref).abs()[fin] / rng[fin]).median().item()
    print(f"case {U.GPU_CASES[ci]} {dt}: worst |device - f64| / tap_range {q:.3e} (median {med:.3e}), allowed "
          f"{U.TOL_REL:.3e}")
    assert q <= U.TOL_REL
    if N > 1:  # the reader of the NaN pixel skips it and still uses its other neighbours
        assert torch.isfinite(got[0, yn, xn])
    else:
        assert _same(got, depth.float())


def test_bitwise_properties():
    ci = 3
    N, H, W, R = U.GPU_CASES[ci]
    depth, flow, valid = U.gpu_inputs(ci, F32)
    whole = _run(depth, flow, valid, R)
    assert _same(whole, _run(depth, flow, valid, R))
    # a chunk (f0, n) of a call is rows f0 … f0 + n − 1 of the whole-video call
    for f0, n in ((0, 1), (2, 3), (N - 1, 1), (1, N - 1)):
        part = _run(depth, flow[:, f0:f0 + n].contiguous(), valid[:, f0:f0 + n].contiguous(), R, f0=f0, n=n)
        assert _same(part, whole[f0:f0 + n]), (f0, n)
    # valid=None is all ones
    assert _same(_run(depth, flow, None, R), _run(depth, flow, torch.ones_like(valid), R))
    # out= is honoured
    out = torch.full((N, H, W), 7.0, device="cuda")
    assert _run(depth, flow, valid, R, out=out) is out and _same(out, whole)
    # f16 depth equals the same numbers widened to f32
    d16 = U.gpu_inputs(ci, F16)[0]
    assert _same(_run(d16, flow, valid, R), _run(d16.float(), flow, valid, R))


def test_sub_clip_gives_the_frames_of_the_full_video():
    """Frames a … b of the full video from the sub-clip [a − R, b + R] alone."""
    ci = 3
    N, H, W, R = U.GPU_CASES[ci]
    depth, flow, valid = U.gpu_inputs(ci, F32)
    whole = _run(depth, flow, valid, R)
    a = b = R  # N = 2R + 1: the middle frame is the only one with all its neighbours inside
    lo, hi = a - R, b + R + 1
    part = _run(depth[lo:hi], flow[:, a:b + 1].contiguous(), valid[:, a:b + 1].contiguous(), R, f0=a - lo, n=b - a + 1)
    assert _same(part, whole[a:b + 1])
    # radius 1 on the same video (the k = ∓1 slots of the pack): frames 2 … 4 from the sub-clip [1, 5]
    sl = [U.slot_of(-1, R), U.slot_of(1, R)]
    f1, v1 = flow[sl].contiguous(), valid[sl].contiguous()
    whole = _run(depth, f1, v1, 1)
    part = _run(depth[1:6].contiguous(), f1[:, 2:5].contiguous(), v1[:, 2:5].contiguous(), 1, f0=1, n=3)
    assert _same(part, whole[2:5])


def test_alignment_does_not_change_the_bits():
    """Every buffer shifted by one of its elements (flow by one 8-byte element) gives the aligned call's bits."""
    for ci, dt in ((4, F32), (2, F16)):
        N, H, W, R = U.GPU_CASES[ci]
        depth, flow, valid = U.gpu_inputs(ci, dt)
        whole = _run(depth, flow, valid, R)

        def shifted(t, by):
            buf = torch.zeros(t.numel() + by, dtype=t.dtype, device="cuda")
            buf[by:] = t.cuda().reshape(-1)
            return buf[by:].view(t.shape)

        out = shifted(torch.zeros((N, H, W), dtype=F32), 1)
        d, f, v = shifted(depth, 1), shifted(flow, 2), shifted(valid, 1)
        assert d.data_ptr() % (2 * d.element_size()) == d.element_size()
        assert f.data_ptr() % 16 == 8 and v.data_ptr() % 2 == 1 and out.data_ptr() % 8 == 4
        got = _run(d, f, v, R, out=out)
        assert _same(got, whole), (ci, dt)


def test_identities_on_the_device():
    """A constant video, N = 1, all-invalid neighbours and flows that all leave the frame come out bit for bit."""
    ci = 4
    N, H, W, R = U.GPU_CASES[ci]
    depth, flow, valid = U.gpu_inputs(ci, F32)
    for c in (0.7319, -3.0e5, 1.0e-12):
        d = torch.full((N, H, W), c, dtype=F32)
        assert torch.equal(_run(d, flow, valid, R).cpu(), d)
    assert _same(_run(depth[:1], flow[:, :1].contiguous(), valid[:, :1].contiguous(), R).cpu(), depth[:1])
    assert _same(_run(depth, flow, torch.zeros_like(valid), R).cpu(), depth)
    assert _same(_run(depth, flow + 1000.0, None, R).cpu(), depth)
    assert _same(_run(depth, torch.full_like(flow, math.nan), None, R).cpu(), depth)
    assert not _same(_run(depth, flow, valid, R).cpu(), depth)


MOTION = (0.75, 0.5)  # pixels per frame: 64 × 96 has one pyramid level, whose three steps reach 3 px at k = 3


def _moving_video(N=5, noise=0.02):
    """The translating texture of tests/flow_util.py at its end-to-end size, a depth that moves with it, the same
    plus noise, and the true flow [N − 1, H, W, 2]."""
    from tests import flow_util as F

    H, W, d = F.E2E["H"], F.E2E["W"], MOTION
    frames = F.video(N, H, W, d, 1.0, F32)
    clean = (torch.stack([F.texture(*F.coords(H, W, d, 1.0, n), scale=0.25) for n in range(N)]) + 2.0).float()
    g = torch.Generator().manual_seed(77)
    noisy = clean + noise * torch.randn(clean.shape, generator=g)
    flow = F.true_flow(H, W, d, 1.0).float()[None].expand(N - 1, H, W, 2).contiguous()
    return frames, clean, noisy, flow


def test_public_function_with_frames(monkeypatch):
    """With frames: the packed flows are optical_flow's, bitwise, for every k; the result is the kernel's on those
    flows, bitwise, and within TOL_REL of the restatement fed the same flows; the chunk size does not matter; host
    input gives a host result of the depth's dtype."""
    import rollingdepth_amd as RD
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import stabilize as S

    frames, clean, noisy, _ = _moving_video(N=6)
    N, H, W = noisy.shape
    R = 2
    kw = dict(radius=R, sigma_time=1.0, sigma_depth=0.2)
    got, flow, valid = RD.temporal_filter(noisy, frames, return_flow=True, **kw)
    assert got.dtype == F32 and not got.is_cuda and got.shape == (N, H, W)
    assert flow.is_cuda and flow.shape == (2 * R, N, H, W, 2) and valid.shape == (2 * R, N, H, W)
    for k in range(1, R + 1):
        of = RD.optical_flow(frames, k)
        assert torch.equal(flow[U.slot_of(k, R), :N - k], of.flow), k
        assert torch.equal(valid[U.slot_of(k, R), :N - k], of.valid), k
        assert torch.equal(flow[U.slot_of(-k, R), k:], of.flow_backward), k
        ob = RD.optical_flow(frames.flip(0), k)  # the reversed video's forward mask is the backward mask
        assert torch.equal(flow[U.slot_of(-k, R), k:], ob.flow.flip(0)), k
        assert torch.equal(valid[U.slot_of(-k, R), k:], ob.valid.flip(0)), k
    want = K.temporal_filter(noisy.cuda(), flow, valid, R, 1.0, 0.2)
    assert torch.equal(got, want.cpu())
    ref, rng = U.restate_and_range(noisy, flow.cpu(), valid.cpu(), R, 1.0, 0.2)
    q = U.ratio(got, ref, rng)
    print(f"temporal_filter against the restatement on its own flows: {q:.3e}, allowed {U.TOL_REL:.3e}; "
          f"{valid.float().mean().item():.3f} of the slots valid")
    assert q <= U.TOL_REL
    assert valid.float().mean().item() > 0.5 and not torch.equal(got, noisy)
    # two other chunk sizes: two frames and one frame per launch
    for frames_per_chunk in (2, 1):
        monkeypatch.setattr(S, "_CHUNK_ELEMS", frames_per_chunk * 2 * R * H * W)
        g2, f2, v2 = RD.temporal_filter(noisy, frames, return_flow=True, **kw)
        assert torch.equal(g2, got) and torch.equal(f2, flow) and torch.equal(v2, valid), frames_per_chunk
    monkeypatch.undo()
    # a flow of the caller's own, uint8 frames, f16 depth [N, 1, H, W] on the device
    assert torch.equal(RD.temporal_filter(noisy, flow=flow.cpu(), valid=valid.cpu(), **kw), got)
    from tests import flow_util as F
    fr8 = F.video(N, H, W, MOTION, 1.0, torch.uint8)
    h = RD.temporal_filter(noisy.half()[:, None].cuda(), fr8, **kw)
    assert h.dtype == F16 and h.is_cuda and h.shape == (N, 1, H, W)
    one = RD.temporal_filter(noisy[:1], frames[:1])
    assert torch.equal(one, noisy[:1])


def test_filter_lowers_flicker():
    """The depth moves with the texture and carries noise of σ = 0.02; measured along the true flow, the flicker
    after the filter (sigma_depth 0.2, flow estimated from the frames) is lower than before."""
    import rollingdepth_amd as RD

    frames, clean, noisy, flow = _moving_video(N=5)
    out = RD.temporal_filter(noisy, frames, sigma_depth=0.2)
    before = RD.temporal_metrics(noisy, clean, flow=flow)
    after = RD.temporal_metrics(out, clean, flow=flow)
    print(f"flicker {before.flicker:.5f} -> {after.flicker:.5f}, tge {before.tge:.5f} -> {after.tge:.5f}")
    assert after.flicker < before.flicker


def test_pipeline_stabilize():
    """The tiny synthetic pipeline of test_upsample_gpu.py::test_pipeline_restore_method: stabilize=False is the call
    without the keyword, bitwise; stabilize=True replaces depth_pred by temporal_filter of the plain run's depth_pred
    along the processing-resolution frames and leaves the other outputs alone; restore_res then acts on the filtered
    map."""
    import rollingdepth_amd as RD
    from rollingdepth_amd import config as C
    from rollingdepth_amd.pipeline import RollingDepthPipeline
    from rollingdepth_amd.video_io import load_video_frames
    from tests.test_video_gpu import _frames

    pipe = RollingDepthPipeline.from_synthetic(C.TINY_UNET, C.TINY_VAE, C.RD_SCHEDULER, device="cuda")
    fr = _frames(9, 45, 60)
    kw = dict(dilations=[1, 3], cap_dilation=True, snippet_lengths=[3], init_infer_steps=[1], strides=[1],
              coalign_kwargs={"num_iterations": 50}, refine_step=0, output_uncertainty=True)
    h, w = pipe.vae.latent_hw(24, 32)
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(3))
    call = lambda **extra: pipe(fr, processing_res=32, init_noise=noise, **dict(kw, **extra))
    names = ("input_rgb", "depth_pred", "depth_coaligned", "depth_uncertainty")

    # refusals come before any inference: no pipeline is needed to raise them
    with pytest.raises(TypeError, match="stabilize"):
        call(stabilize="yes")
    with pytest.raises(ValueError, match="stabilize_kwargs"):
        call(stabilize=True, stabilize_kwargs={"sigma": 2})
    with pytest.raises(ValueError, match="radius"):
        call(stabilize=True, stabilize_kwargs={"radius": 5})

    plain = call()
    off = call(stabilize=False)
    for name in names:
        assert torch.equal(getattr(plain, name), getattr(off, name)), name
    for a, b in zip(plain.snippet_ls, off.snippet_ls):
        assert torch.equal(a, b)

    frames = load_video_frames(fr, 0, 0, 32, "BILINEAR", device="cuda")[0]
    assert frames.shape[-2:] == plain.depth_pred.shape[-2:]
    on = call(stabilize=True)
    want = RD.temporal_filter(plain.depth_pred, frames=frames)
    assert on.depth_pred.dtype == plain.depth_pred.dtype and on.depth_pred.shape == plain.depth_pred.shape
    assert not on.depth_pred.is_cuda
    assert torch.equal(on.depth_pred, want) and not torch.equal(on.depth_pred, plain.depth_pred)
    for name in ("input_rgb", "depth_coaligned", "depth_uncertainty"):
        assert torch.equal(getattr(on, name), getattr(plain, name)), name
    for a, b in zip(on.snippet_ls, plain.snippet_ls):
        assert torch.equal(a, b)

    skw = dict(radius=3, sigma_depth=0.2, flow_kwargs={"radius": 2})
    wide = call(stabilize=True, stabilize_kwargs=skw)
    assert torch.equal(wide.depth_pred, RD.temporal_filter(plain.depth_pred, frames=frames, **skw))

    jb = call(stabilize=True, restore_res=True, restore_method="joint_bilateral")
    assert jb.depth_pred.shape == (9, 1, 45, 60)
    assert torch.equal(jb.depth_pred, RD.guided_upsample(want, torch.from_numpy(fr)))
    assert torch.equal(jb.depth_uncertainty, RD.guided_upsample(plain.depth_uncertainty, torch.from_numpy(fr)))
