"""rdmi_joint_bilateral_upsample on the device: against the f64 restatement of tests/upsample_util.py within TOL_REL
of each pixel's tap range, the bitwise properties the header promises, the edge condition of the CPU test, and the
pipeline's restore_method."""
import pytest
import torch

from tests import upsample_util as U

pytestmark = pytest.mark.gpu


def _dev(t):
    return t.cuda()


def _run(values, guide_lo, guide_hi, r, **kw):
    from rollingdepth_amd import kernels as K

    return K.joint_bilateral_upsample(_dev(values), _dev(guide_lo), _dev(guide_hi), r, U.SIGMA_SPATIAL, U.SIGMA_RANGE,
                                      **kw)


@pytest.mark.parametrize("vdtype", [U.F16, U.F32], ids=["f16", "f32"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8guide", "f32guide"])
@pytest.mark.parametrize("ci", range(len(U.GPU_CASES)))
def test_against_the_f64_restatement(ci, u8, vdtype):
    values, guide_lo, guide_hi = U.gpu_inputs(ci, u8, vdtype)
    ref, rng = U.gpu_reference(ci, u8, vdtype)
    N, h, w, H, W, r, C = U.GPU_CASES[ci]
    out = _run(values, guide_lo, guide_hi, r)
    assert out.shape == (N, C, H, W) and out.dtype == U.F32
    q = ((out.cpu().double() - ref).abs() / rng).max().item()
    print(f"case {U.GPU_CASES[ci]}: worst |device - f64| / range {q:.3e} (TOL_REL {U.TOL_REL:.3e})")
    assert q <= U.TOL_REL, q


def test_bitwise_properties():
    """Two calls agree; a frame alone equals the frame in the batch; channel k of a C = 4 call equals the C = 1 call;
    views at an odd storage offset equal the aligned call; `out` is honoured."""
    ci = 3
    N, h, w, H, W, r, C = U.GPU_CASES[ci]
    for u8, vd in ((True, U.F16), (False, U.F32)):
        values, guide_lo, guide_hi = (_dev(t) for t in U.gpu_inputs(ci, u8, vd))
        a = _run(values, guide_lo, guide_hi, r)
        assert torch.equal(a, _run(values, guide_lo, guide_hi, r))
        for n in range(N):
            one = _run(values[n:n + 1], guide_lo[n:n + 1], guide_hi[n:n + 1], r)
            assert torch.equal(one[0], a[n]), n
        for k in range(C):
            one = _run(values[:, k:k + 1].contiguous(), guide_lo, guide_hi, r)
            assert torch.equal(one[:, 0], a[:, k]), k

        def shifted(t):  # the same elements one element further into a fresh buffer
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() == buf.data_ptr() + t.element_size() and v.is_contiguous()
            return v

        b = _run(shifted(values), shifted(guide_lo), shifted(guide_hi), r)
        assert torch.equal(a, b)
        o = torch.empty_like(a)
        assert _run(values, guide_lo, guide_hi, r, out=o) is o and torch.equal(o, a)
    # f16 values and the same numbers widened to f32 are the same call
    values, guide_lo, guide_hi = U.gpu_inputs(ci, True, U.F16)
    assert torch.equal(_run(values, guide_lo, guide_hi, r), _run(values.float(), guide_lo, guide_hi, r))
    # a planar guide given through strides (a permuted channels-last buffer) is the planar call
    values, guide_lo, guide_hi = U.gpu_inputs(ci, False, U.F32)
    cl = _dev(guide_hi).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(_run(values, guide_lo, guide_hi, r), _run(values, guide_lo, cl.permute(0, 3, 1, 2), r))
    assert torch.equal(_run(values, guide_lo, guide_hi, r), _run(values, guide_lo, cl, r, channels_last=True))


@pytest.mark.parametrize("ci", [0, 3, 4])
def test_constant_plane_within_4_ulp(ci):
    N, h, w, H, W, r, C = U.GPU_CASES[ci]
    values, guide_lo, guide_hi = U.gpu_inputs(ci, True, U.F32)
    for c in (0.37, -1.0, 3.0e-3, 1234.5):
        cf = torch.tensor(c, dtype=U.F32)
        out = _run(torch.full_like(values, c), guide_lo, guide_hi, r).cpu()
        ulp = torch.nextafter(cf.abs(), torch.tensor(float("inf"))) - cf.abs()
        d = ((out - cf).abs().max() / ulp).item()
        print(f"case {U.GPU_CASES[ci]} c = {c}: {d:.1f} ulp")
        assert d <= 4.0, (c, d)


@pytest.mark.parametrize("ei", range(len(U.EDGE_CASES)))
def test_edge_preservation_on_the_device(ei):
    """The CPU test's condition on the device: within 1e-6 of the own side for r = 1, 2, 3, where the bilinear resize
    of the same values has pixels strictly between 0.05 and 0.95 — what the option buys."""
    from rollingdepth_amd import kernels as K

    values, guide_lo, guide_hi, side = U.edge_inputs(ei)
    h, w, H, W, X0 = U.EDGE_CASES[ei]
    for r in (1, 2, 3):
        out = _run(values, guide_lo, guide_hi, r).cpu().double()
        d = (out[0, 0] - side).abs().max().item()
        print(f"edge case {U.EDGE_CASES[ei]} r = {r}: max |out - side| {d:.2e}")
        assert d <= 1e-6, (r, d)
    up = K.resize(_dev(values), (H, W), "BILINEAR").cpu()
    ramp = int(((up > 0.05) & (up < 0.95)).sum())
    print(f"edge case {U.EDGE_CASES[ei]}: the bilinear resize leaves {ramp} pixels in (0.05, 0.95)")
    assert ramp > 0


def test_guided_upsample_matches_the_kernel_call():
    """The public function builds guide_lo with the device's own bilinear resize, takes host or device tensors and
    returns depth's dtype on depth's device; uint8 frames and the same frames as floats in [0, 1] land within the
    tolerance of each other's restatement."""
    import rollingdepth_amd as R
    from rollingdepth_amd import kernels as K

    ci = 2
    N, h, w, H, W, r, C = U.GPU_CASES[ci]
    values, _, frames = U.gpu_inputs(ci, True, U.F16)
    got = R.guided_upsample(values, frames, r, U.SIGMA_SPATIAL, U.SIGMA_RANGE)
    assert got.dtype == U.F16 and got.device == values.device and got.shape == (N, C, H, W)
    guide_lo = K.resize(_dev(frames), (h, w), "BILINEAR", channels_last=True) * (1.0 / 255.0)
    want = _run(values, guide_lo.cpu(), frames, r)
    assert torch.equal(got, want.half().cpu())
    ref = U.restate(values, guide_lo.cpu(), frames, r)
    q = ((want.cpu().double() - ref).abs() / U.tap_range(values, frames, r)).max().item()
    print(f"guided_upsample against the restatement on its own guide_lo: {q:.3e}")
    assert q <= U.TOL_REL
    on_dev = R.guided_upsample(_dev(values), frames, r, U.SIGMA_SPATIAL, U.SIGMA_RANGE)
    assert on_dev.is_cuda and torch.equal(on_dev.cpu(), got)
    with pytest.raises(ValueError, match="only upsamples"):
        R.guided_upsample(values, frames[:, :h - 1], r)


def test_pipeline_restore_method():
    """The tiny synthetic pipeline and frames of test_call_with_decoded_frames_and_restore_res: "resize" is the call
    without the keyword, bitwise; "joint_bilateral" returns depth_pred and depth_uncertainty at 45 × 60, bitwise
    guided_upsample of the un-restored run's outputs, and leaves the other outputs alone."""
    import rollingdepth_amd as R
    from rollingdepth_amd import config as C
    from rollingdepth_amd.pipeline import RollingDepthPipeline
    from tests.test_video_gpu import _frames

    pipe = RollingDepthPipeline.from_synthetic(C.TINY_UNET, C.TINY_VAE, C.RD_SCHEDULER, device="cuda")
    fr = _frames(9, 45, 60)
    kw = dict(dilations=[1, 3], cap_dilation=True, snippet_lengths=[3], init_infer_steps=[1], strides=[1],
              coalign_kwargs={"num_iterations": 50}, refine_step=0, output_uncertainty=True)
    h, w = pipe.vae.latent_hw(24, 32)
    noise = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(3))
    call = lambda **extra: pipe(fr, processing_res=32, init_noise=noise, **dict(kw, **extra))
    names = ("input_rgb", "depth_pred", "depth_coaligned", "depth_uncertainty")

    plain = call(restore_res=True)
    resize = call(restore_res=True, restore_method="resize")
    for name in names:
        assert torch.equal(getattr(plain, name), getattr(resize, name)), name
    for a, b in zip(plain.snippet_ls, resize.snippet_ls):
        assert torch.equal(a, b)

    low = call()
    jb = call(restore_res=True, restore_method="joint_bilateral")
    assert jb.depth_pred.shape == (9, 1, 45, 60) and jb.depth_uncertainty.shape == (9, 1, 45, 60)
    assert jb.depth_pred.dtype == low.depth_pred.dtype and jb.depth_uncertainty.dtype == torch.float32
    assert not jb.depth_pred.is_cuda and not jb.depth_uncertainty.is_cuda
    frames = torch.from_numpy(fr)
    assert torch.equal(jb.depth_pred, R.guided_upsample(low.depth_pred, frames))
    assert torch.equal(jb.depth_uncertainty, R.guided_upsample(low.depth_uncertainty, frames))
    assert torch.equal(jb.input_rgb, plain.input_rgb)
    assert torch.equal(jb.depth_coaligned, low.depth_coaligned)
    for a, b in zip(jb.snippet_ls, low.snippet_ls):
        assert torch.equal(a, b)
    assert not torch.equal(jb.depth_pred, plain.depth_pred)

    wide = call(restore_res=True, restore_method="joint_bilateral", restore_kwargs=dict(radius=3, sigma_range=0.2))
    assert torch.equal(wide.depth_pred, R.guided_upsample(low.depth_pred, frames, radius=3, sigma_range=0.2))
    # a video below the processing resolution is refused right after ingest, before any inference
    with pytest.raises(ValueError, match="only upsamples"):
        pipe(_frames(9, 20, 30), processing_res=32, init_noise=noise, restore_res=True,
             restore_method="joint_bilateral", **kw)
    with pytest.raises(ValueError, match="radius"):
        call(restore_res=True, restore_method="joint_bilateral", restore_kwargs=dict(radius=5))
