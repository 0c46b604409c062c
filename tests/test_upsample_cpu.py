"""CPU side of the edge-aware restore (joint bilateral upsampling): the new library symbol, the argument checks that
run before any device work in the C entry, in guided_upsample and in the pipeline's __call__, the edge-preservation
condition on the f64 restatement (tests/upsample_util.py), and the f32-against-f64 ratio from which
tests/test_upsample_gpu.py takes its tolerance."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests import upsample_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDMI_E_ARG, RDMI_E_UNSUPPORTED = 1001, 1003


def test_new_symbol_declared_bound_and_exported():
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import upsample as UP

    hdr = open(os.path.join(ROOT, "include", "rdmi.h")).read()
    assert "Guided upsampling (since rdmi_version 11)" in hdr
    name = "rdmi_joint_bilateral_upsample"
    assert re.search(rf"\b{name}\s*\(", hdr)
    assert name in N_.EXPORTED and callable(getattr(N_.lib, name))
    assert N_.lib.rdmi_version() >= 11
    assert "#define RDMI_JBU_MAX_RADIUS 3" in hdr
    assert (K.JBU_MAX_RADIUS, UP.MAX_RADIUS, K.JBU_MAX_CHANNELS, UP.MAX_CHANNELS) == (3, 3, 4, 4)
    assert os.path.exists(os.path.join(ROOT, "rollingdepth_amd", "csrc", "upsample.hip"))
    for code, text in ((RDMI_E_ARG, "RDMI_E_ARG"), (RDMI_E_UNSUPPORTED, "RDMI_E_UNSUPPORTED")):
        assert re.search(rf"#define\s+{text}\s+\(?{code}\)?", hdr), text


def _call(**over):
    """One call of the C entry with valid arguments (the pointers are dummies that are never dereferenced: every
    call below is refused before a launch) except for what `over` replaces."""
    from rollingdepth_amd import _native as N_

    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(values=p, values_dtype=N_.RDMI_F32, guide_lo=p, guide_hi=p, guide_dtype=N_.RDMI_U8, sn=1, sc=1, sy=1,
             sx=1, guide_scale=1.0, N=1, C=1, h=2, w=2, H=4, W=4, radius=2, sigma_spatial=1.0, sigma_range=0.1, out=p,
             stream=None)
    a.update(over)
    rc = N_.lib.rdmi_joint_bilateral_upsample(*a.values())
    return rc, N_.lib.rdmi_last_error().decode()


def test_library_checks_run_before_any_launch():
    """Every rejected argument gets one call, on a machine without a GPU: nothing can have been launched."""
    from rollingdepth_amd import _native as N_

    bad = [dict(values=None), dict(guide_lo=None), dict(guide_hi=None), dict(out=None),
           dict(N=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(N=-1),
           dict(C=0), dict(C=5),
           dict(radius=0), dict(radius=4),
           dict(sigma_spatial=0.0), dict(sigma_spatial=-1.0), dict(sigma_spatial=float("nan")),
           dict(sigma_range=0.0), dict(sigma_range=-0.1), dict(sigma_range=float("nan")),
           dict(values_dtype=N_.RDMI_U8), dict(values_dtype=7),
           dict(guide_dtype=N_.RDMI_F16), dict(guide_dtype=9)]
    for kw in bad:
        rc, msg = _call(**kw)
        assert rc == RDMI_E_ARG and "joint_bilateral_upsample" in msg, (kw, rc, msg)
    for kw in (dict(H=1), dict(W=1), dict(h=5, H=4), dict(w=9, W=8)):
        rc, msg = _call(**kw)
        assert rc == RDMI_E_UNSUPPORTED and "upsampler" in msg, (kw, rc, msg)


def test_check_restore_method():
    from rollingdepth_amd.pipeline import RollingDepthPipeline, check_restore_method

    assert check_restore_method("resize") == ("resize", {})
    assert check_restore_method("joint_bilateral", None) == ("joint_bilateral", {})
    assert check_restore_method("joint_bilateral", {"radius": 3, "sigma_range": 0.2}) == (
        "joint_bilateral", {"radius": 3, "sigma_range": 0.2})
    for bad in ("bilinear", "JOINT_BILATERAL", "", None, 1, True, b"resize"):
        with pytest.raises(ValueError, match="restore_method"):
            check_restore_method(bad)
    for bad in ({"sigma": 1.0}, [("radius", 2)], "radius", 2):
        with pytest.raises(ValueError, match="restore_kwargs"):
            check_restore_method("joint_bilateral", bad)
    with pytest.raises(ValueError, match="restore_kwargs"):
        check_restore_method("resize", {"radius": 2})
    p = inspect.signature(RollingDepthPipeline.__call__).parameters
    assert p["restore_method"].default == "resize" and p["restore_kwargs"].default is None


def test_call_refuses_before_any_device_work():
    """self = None and no GPU: the errors below are raised before the pipeline or a device is touched."""
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    fr = torch.zeros((5, 3, 8, 8))
    with pytest.raises(ValueError, match="restore_method"):
        RollingDepthPipeline.__call__(None, fr, restore_method="bicubic")
    with pytest.raises(ValueError, match="restore_method"):
        RollingDepthPipeline.__call__(None, fr, restore_res=True, restore_method=None)
    with pytest.raises(ValueError, match="needs restore_res"):
        RollingDepthPipeline.__call__(None, fr, restore_method="joint_bilateral")
    with pytest.raises(ValueError, match="restore_kwargs"):
        RollingDepthPipeline.__call__(None, fr, restore_res=True, restore_method="joint_bilateral",
                                      restore_kwargs={"sigma": 1})


def test_guided_upsample_checks_come_before_any_device_work():
    import rollingdepth_amd
    from rollingdepth_amd import upsample as UP

    assert rollingdepth_amd.guided_upsample is UP.guided_upsample
    p = inspect.signature(UP.guided_upsample).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("radius", 2), ("sigma_spatial", 1.0), ("sigma_range", 0.1)]
    d = torch.zeros(2, 1, 4, 5)
    u8 = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    fl = torch.zeros(2, 3, 8, 9)
    assert UP.check_upsample_args(d, u8) == (2, 1, 4, 5, 8, 9)
    assert UP.check_upsample_args(d.half().expand(2, 4, 4, 5), fl, 3, 2, 0.5) == (2, 4, 4, 5, 8, 9)
    type_errors = [(dict(depth=d.numpy()), "depth"), (dict(depth=d.double()), "depth"), (dict(depth=d.int()), "depth"),
                   (dict(frames=u8.numpy()), "frames"), (dict(frames=u8.int()), "frames"),
                   (dict(radius=2.0), "radius"), (dict(radius=True), "radius"),
                   (dict(sigma_spatial="1"), "sigma_spatial"), (dict(sigma_range=True), "sigma_range")]
    for kw, word in type_errors:
        with pytest.raises(TypeError, match=word):
            UP.guided_upsample(**dict(dict(depth=d, frames=u8), **kw))
    value_errors = [(dict(depth=d[0]), "depth"), (dict(depth=d.expand(2, 5, 4, 5)), "depth"),
                    (dict(frames=u8[0]), "frames"), (dict(frames=u8.permute(0, 3, 1, 2)), "three channels"),
                    (dict(frames=fl.permute(0, 2, 3, 1)), "three channels"), (dict(frames=u8[:1]), "2 frames"),
                    (dict(frames=u8[:, :3]), "only upsamples"), (dict(frames=fl[..., :4]), "only upsamples"),
                    (dict(depth=d[:, :, :0]), "empty"),
                    (dict(radius=0), "radius"), (dict(radius=4), "radius"),
                    (dict(sigma_spatial=0), "sigma_spatial"), (dict(sigma_spatial=float("nan")), "sigma_spatial"),
                    (dict(sigma_range=-0.1), "sigma_range"), (dict(sigma_range=float("inf")), "sigma_range")]
    for kw, word in value_errors:
        with pytest.raises(ValueError, match=word):
            UP.guided_upsample(**dict(dict(depth=d, frames=u8), **kw))


def test_ingest_keeps_its_two_values_by_default():
    from rollingdepth_amd import video_io as V

    for fn in (V.frames_from_rgb24, V.load_video_frames):
        assert inspect.signature(fn).parameters["return_source"].default is False, fn


@pytest.mark.parametrize("ei", range(len(U.EDGE_CASES)))
def test_edge_preservation_on_the_restatement(ei):
    """A 0 | 1 step in the guide, values 1 where the downsampled guide is above 0.5: with σs = 1, σr = 0.1 every output
    pixel lies within 1e-6 of its own side's value for r = 1, 2, 3 (measured: at most 2e-44), where a plain bilinear
    upsample of the same values leaves 46, 74 and 87 pixels between 0.05 and 0.95."""
    values, guide_lo, guide_hi, side = U.edge_inputs(ei)
    h, w, H, W, X0 = U.EDGE_CASES[ei]
    for r in (1, 2, 3):
        out = U.restate(values, guide_lo, guide_hi, r, 1.0, 0.1)
        d = (out[0, 0] - side).abs().max().item()
        print(f"edge case {U.EDGE_CASES[ei]} r = {r}: max |out - side| {d:.2e}")
        assert d <= 1e-6, (r, d)
    ramp = U.bilinear_ramp_pixels(values, H, W)
    print(f"edge case {U.EDGE_CASES[ei]}: bilinear leaves {ramp} pixels in (0.05, 0.95)")
    assert ramp == (46, 74, 87)[ei]


def test_restatement_basics():
    """A constant plane comes out constant, the weights do not depend on the channel count, and one in-image tap of
    weight 1 exists for a σ as small as 1e-6 (no 0/0)."""
    values, guide_lo, guide_hi = U.gpu_inputs(3, True, U.F32)
    r = U.GPU_CASES[3][5]
    ref = U.gpu_reference(3, True, U.F32)[0]
    one = U.restate(values[:, 2:3], guide_lo, guide_hi, r)
    assert torch.equal(one[:, 0], ref[:, 2])
    c = U.restate(torch.full_like(values, 0.37), guide_lo, guide_hi, r)
    assert (c - values.new_tensor(0.37).double()).abs().max().item() <= 1e-15
    tiny = U.restate(values, guide_lo, guide_hi, r, 1e-6, 1e-6)
    assert torch.isfinite(tiny).all() and tiny.abs().max().item() <= 1.0


def test_f32_ratio_behind_the_gpu_tolerance():
    """U.F32_RATIO is the worst |f32 restatement − f64| / range over all 20 GPU variants; re-measured here on every
    one of them, so that the constant cannot drift from the code.  The upsampling cases alone stay within the
    (2r)²·2⁻²⁴ of the error model."""
    worst, worst_up = 0.0, 0.0
    for ci, u8, vd in U.all_gpu_variants():
        q = U.f32_ratio(ci, u8, vd)
        print(f"case {U.GPU_CASES[ci]} {'u8' if u8 else 'f32'} guide, {vd} values: ratio {q:.3e}")
        worst = max(worst, q)
        if ci > 0:
            r = U.GPU_CASES[ci][5]
            assert q <= (2 * r) ** 2 * 2.0 ** -24, (ci, q)
            worst_up = max(worst_up, q)
    print(f"worst ratio {worst:.3e} (upsampling cases {worst_up:.3e}); F32_RATIO {U.F32_RATIO:.3e}, TOL_REL {U.TOL_REL:.3e}")
    assert 0.5 * U.F32_RATIO <= worst <= U.F32_RATIO
    assert U.TOL_REL == 4 * U.F32_RATIO
