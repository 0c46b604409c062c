"""CPU side of the alignment spaces and of temporal_metrics: the public names, the argument checks that run before
any device work, the pooling of pair sums (mocked sums), librdmi's own checks of the three new calls, which return
before any launch, and the properties of the seeded inputs that tests/test_temporal_gpu.py relies on."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tests import temporal_util as T


def _ok(n=3, h=4, w=5):
    return torch.rand(n, h, w) + 0.5, torch.rand(n, h, w) + 0.5, torch.ones(n, h, w, dtype=torch.bool)


def test_public_names():
    import rollingdepth_amd as R
    from rollingdepth_amd import metrics as M

    assert R.temporal_metrics is M.temporal_metrics and R.TemporalMetrics is M.TemporalMetrics
    names = [f.name for f in dataclasses.fields(M.TemporalMetrics)]
    assert names == ["flicker", "flicker_rmse", "tge", "tge_rmse", "target_change", "change_corr", "n_valid", "scale",
                     "shift", "per_pair", "pairs_skipped"]
    assert M.SPACES == ("depth", "disparity", "log")


def test_library_version_and_space_codes():
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K

    assert N_.lib.rdmi_version() >= 8
    assert (N_.RDMI_SPACE_DEPTH, N_.RDMI_SPACE_DISPARITY, N_.RDMI_SPACE_LOG) == (0, 1, 2)
    assert K.DEPTH_SPACES == {"depth": 0, "disparity": 1, "log": 2}


@pytest.mark.parametrize("fn", ["depth_metrics", "align_scale_shift"])
def test_space_errors_come_before_any_device_work(fn):
    from rollingdepth_amd import metrics as M

    call = getattr(M, fn)
    p, g, m = _ok()
    with pytest.raises(ValueError, match="space"):
        call(p, g, m, space="inverse")
    with pytest.raises(ValueError, match="space"):
        call(p, g, m, space=None)
    with pytest.raises(ValueError, match="does not match"):
        call(p, g[:, :3], space="log")
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p.double(), g, space="disparity", **({"clip": (0.1, 10.0)} if fn == "depth_metrics" else {}))


def test_disparity_space_needs_a_finite_upper_clip():
    from rollingdepth_amd.metrics import depth_metrics, temporal_metrics

    p, g, m = _ok()
    for clip in (None, (0.1, math.inf), (-math.inf, math.inf)):
        with pytest.raises(ValueError, match="finite upper clip"):
            depth_metrics(p, g, m, space="disparity", clip=clip)
        with pytest.raises(ValueError, match="finite upper clip"):
            temporal_metrics(p, g, m, space="disparity", clip=clip)
    with pytest.raises(ValueError, match="clip"):
        depth_metrics(p, g, m, space="disparity", clip=(2.0, 1.0))


def test_temporal_value_and_type_errors_come_before_any_device_work():
    from rollingdepth_amd.metrics import temporal_metrics as call

    p, g, m = _ok()
    flow, pm = torch.zeros(2, 4, 5, 2), torch.ones(2, 4, 5, dtype=torch.bool)
    # the messages and the TypeError / ValueError split of depth_metrics
    with pytest.raises(ValueError, match="does not match"):
        call(p, g[:, :3])
    with pytest.raises(ValueError, match="does not match"):
        call(p, g, m[:1])
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        call(p[0], g[0])
    with pytest.raises(ValueError, match="empty"):
        call(p[:0], g[:0])
    with pytest.raises(ValueError, match="valid_range"):
        call(p, g, valid_range=(1.0, 1.0))
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p.double(), g)
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p, g.to(torch.bfloat16))
    with pytest.raises(TypeError, match="bool or uint8"):
        call(p, g, m.float())
    with pytest.raises(TypeError, match="tensor"):
        call(p.numpy(), g)
    with pytest.raises(ValueError, match="align"):
        call(p, g, m, align="snippet")
    with pytest.raises(ValueError, match="space"):
        call(p, g, m, space="inverse")
    with pytest.raises(ValueError, match="clip"):
        call(p, g, m, clip=(math.nan, 1.0))
    # its own
    for align in ("video", "frame"):
        with pytest.raises(ValueError, match="without a target"):
            call(p, None, m, align=align)
    with pytest.raises(ValueError, match="without a target"):
        call(p)  # the default align is "video"
    for k in (0, -1, 3, 7):
        with pytest.raises(ValueError, match="frame_step"):
            call(p, g, m, frame_step=k)
    with pytest.raises(ValueError, match="frame_step"):
        call(p[:1], g[:1], m[:1])
    with pytest.raises(TypeError, match="frame_step"):
        call(p, g, m, frame_step=1.0)
    with pytest.raises(ValueError, match="flow: shape"):
        call(p, g, m, flow=flow[:1])
    with pytest.raises(ValueError, match="flow: shape"):
        call(p, g, m, flow=flow, frame_step=2)
    with pytest.raises(ValueError, match="flow: shape"):
        call(p, g, m, flow=flow.permute(0, 3, 1, 2))
    with pytest.raises(TypeError, match="flow: float32"):
        call(p, g, m, flow=flow.double())
    with pytest.raises(TypeError, match="flow: float32"):
        call(p, g, m, flow=flow.half())
    with pytest.raises(TypeError, match="flow: a tensor"):
        call(p, g, m, flow=flow.numpy())
    with pytest.raises(ValueError, match="pair_mask: shape"):
        call(p, g, m, pair_mask=m)
    with pytest.raises(ValueError, match="pair_mask: shape"):
        call(p, g, m, pair_mask=pm[:, :3])
    with pytest.raises(TypeError, match="pair_mask: bool or uint8"):
        call(p, g, m, pair_mask=pm.float())
    with pytest.raises(TypeError, match="pair_mask: a tensor"):
        call(p, g, m, pair_mask=[[1]])


def test_pool_adds_pairs_and_divides_by_n():
    from rollingdepth_amd.metrics import _pool_temporal

    # n, Σ|Δa|, ΣΔa², Σ|Δa−Δg|, Σ(Δa−Δg)², Σ|Δg|, ΣΔg², ΣΔa·Δg
    sums = torch.tensor([[4.0, 2.0, 8.0, 1.0, 3.0, 4.0, 8.0, 6.0],
                         [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                         [12.0, 2.0, 56.0, 3.0, 1.0, 4.0, 8.0, 10.0]], dtype=torch.float64)
    scale = torch.tensor([1.5, 2.0, math.nan, 2.0], dtype=torch.float64)
    shift = torch.tensor([0.25, 0.0, 0.5, 0.0], dtype=torch.float64)
    m = _pool_temporal(sums, scale, shift, 1)
    assert (m.n_valid, m.pairs_skipped) == (16, [1, 2])  # pairs (1, 2) and (2, 3) touch frame 2
    assert (m.flicker, m.flicker_rmse, m.tge, m.tge_rmse, m.target_change) == (0.25, 2.0, 0.25, 0.5, 0.5)
    assert m.change_corr == 16.0 / math.sqrt(64.0 * 16.0) == 0.5
    assert m.per_pair is sums and m.scale is scale and m.shift is shift
    assert all(isinstance(getattr(m, k), float) for k in ("flicker", "flicker_rmse", "tge", "tge_rmse", "change_corr"))
    # frame_step 2 on five frames: three pairs, (0, 2), (1, 3), (2, 4)
    five = torch.tensor([1.0, math.nan, 1.0, 1.0, 1.0], dtype=torch.float64)
    assert _pool_temporal(sums, five, torch.zeros(5, dtype=torch.float64), 2).pairs_skipped == [1]
    assert _pool_temporal(sums, five.roll(1), five.roll(1), 2).pairs_skipped == [0, 2]
    # without a target the target-based fields are NaN whatever the sums hold
    m = _pool_temporal(sums, scale, shift, 1, has_target=False)
    assert (m.flicker, m.flicker_rmse, m.n_valid) == (0.25, 2.0, 16)
    assert all(math.isnan(getattr(m, k)) for k in ("tge", "tge_rmse", "target_change", "change_corr"))


def test_pool_of_nothing_is_nan_and_does_not_raise():
    from rollingdepth_amd.metrics import _pool_temporal

    ones = torch.ones(3, dtype=torch.float64)
    m = _pool_temporal(torch.zeros((2, 8), dtype=torch.float64), ones, ones.clone(), 1)
    assert m.n_valid == 0 and m.pairs_skipped == []
    for k in ("flicker", "flicker_rmse", "tge", "tge_rmse", "target_change", "change_corr"):
        assert math.isnan(getattr(m, k)), k
    # a constant prediction or a constant target: no correlation to speak of
    sums = torch.tensor([[4.0, 0.0, 0.0, 2.0, 1.0, 2.0, 1.0, 0.0]], dtype=torch.float64)
    m = _pool_temporal(sums, ones[:2], ones[:2].clone(), 1)
    assert m.flicker == 0.0 and m.tge == 0.5 and math.isnan(m.change_corr)


def test_library_checks_run_before_any_launch():
    """RDMI_E_ARG for every listed bad argument of the three new calls, RDMI_E_UNSUPPORTED for too many pairs — on a
    machine without a GPU, so nothing can have been launched.  The pointers are never dereferenced."""
    from rollingdepth_amd import _native as N_

    lib, inf, nan, x = N_.lib, math.inf, math.nan, 4096  # x: a non-null pointer value
    mom = lambda *a: (lib.rdmi_depth_moments_space(*a, None), lib.rdmi_last_error())  # noqa: E731
    err = lambda *a: (lib.rdmi_depth_errors_space(*a, None), lib.rdmi_last_error())  # noqa: E731

    def tmp(**bad):  # a good call with the named arguments replaced; never without one: the pointers are dummies
        assert bad
        a = dict(pred=x, pred_dtype=1, target=x, target_dtype=1, N=3, H=4, W=5, k=1, lo=1e-3, hi=inf, st=x, space=0,
                 clip_lo=-inf, clip_hi=inf, ws=x, sums=x)
        a.update(bad)
        rc = lib.rdmi_depth_temporal(a["pred"], a["pred_dtype"], a["target"], a["target_dtype"], None, None, None,
                                     a["N"], a["H"], a["W"], a["k"], a["lo"], a["hi"], a["st"], a["space"],
                                     a["clip_lo"], a["clip_hi"], a["ws"], a["sums"], None)
        return rc, lib.rdmi_last_error()

    bad = {
        "moments space": (mom(x, 1, x, 1, None, 2, 9, 1e-3, inf, 3, x), b"space"),
        "moments negative space": (mom(x, 1, x, 1, None, 2, 9, 1e-3, inf, -1, x), b"space"),
        "moments pred null": (mom(None, 1, x, 1, None, 2, 9, 1e-3, inf, 1, x), b"null"),
        "moments workspace null": (mom(x, 1, x, 1, None, 2, 9, 1e-3, inf, 2, None), b"null"),
        "moments N": (mom(x, 1, x, 1, None, 0, 9, 1e-3, inf, 1, x), b"N (0)"),
        "moments dtype": (mom(x, 2, x, 1, None, 2, 9, 1e-3, inf, 1, x), b"dtype"),
        "moments lo >= hi": (mom(x, 0, x, 0, None, 2, 9, 1.0, 1.0, 2, x), b"lo < hi"),
        "errors space": (err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, 7, -inf, inf, x, x), b"space"),
        "errors st null": (err(x, 1, x, 1, None, 2, 9, 1e-3, inf, None, 1, -inf, inf, x, x), b"null"),
        "errors sums null": (err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, 2, -inf, inf, x, None), b"null"),
        "errors P": (err(x, 1, x, 1, None, 2, 0, 1e-3, inf, x, 1, -inf, inf, x, x), b"P (0)"),
        "errors dtype": (err(x, 1, x, 3, None, 2, 9, 1e-3, inf, x, 1, -inf, inf, x, x), b"dtype"),
        "errors lo >= hi": (err(x, 1, x, 1, None, 2, 9, 2.0, 1.0, x, 1, -inf, inf, x, x), b"lo < hi"),
        "errors clip": (err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, 1, 1.0, 0.5, x, x), b"clip"),
        "errors nan clip": (err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, 2, nan, 0.5, x, x), b"clip"),
        "temporal pred null": (tmp(pred=None), b"null"),
        "temporal st null": (tmp(st=None), b"null"),
        "temporal workspace null": (tmp(ws=None), b"null"),
        "temporal sums null": (tmp(sums=None), b"null"),
        "temporal N": (tmp(N=1), b"N (1)"),
        "temporal H": (tmp(H=0), b"H (0)"),
        "temporal W": (tmp(W=-5), b"W (-5)"),
        "temporal k = 0": (tmp(k=0), b"frame_step"),
        "temporal k = N": (tmp(k=3), b"frame_step"),
        "temporal pred dtype": (tmp(pred_dtype=2), b"dtype"),
        "temporal target dtype": (tmp(target_dtype=5), b"dtype"),
        "temporal no target, pred dtype": (tmp(target=None, pred_dtype=-1), b"dtype"),
        "temporal space": (tmp(space=3), b"space"),
        "temporal lo >= hi": (tmp(lo=1.0, hi=1.0), b"lo < hi"),
        "temporal nan range": (tmp(lo=nan, hi=1.0), b"lo < hi"),
        "temporal clip": (tmp(clip_lo=1.0, clip_hi=0.5), b"clip"),
        "temporal nan clip": (tmp(target=None, clip_hi=nan), b"clip"),
    }
    wrong = {k: v for k, (v, word) in bad.items() if v[0] != 1001 or word not in v[1]}
    assert not wrong, wrong
    rc, msg = tmp(N=65537)
    assert rc == 1003 and b"65535 pairs" in msg
    with pytest.raises(N_.RdmiError, match="65535 pairs"):
        N_.check(rc, "rdmi_depth_temporal")


def test_space_inputs_are_fit_for_the_comparison():
    """What tests/test_temporal_gpu.py takes for granted about the disparity- and log-space inputs, for every shape and
    dtype pair: no aligned disparity is <= 0, no ratio lies within the 1e-10 guard of a δ threshold, and δ₁ is
    neither 0 nor 1."""
    for space in ("disparity", "log"):
        for shape, pd, td, mk in T.SPACE_CASES:
            p, gt, m = T.inputs(shape, space)
            pn, gn = T.f64(p.to(pd)), T.f64(gt.to(td))
            v = T.ref_valid(pn, gn, m.numpy() if mk else None, space=space)
            mom, mom_abs = T.ref_moments(pn, gn, v, space)
            for align in ("video", "frame", "none"):
                s, t, cond = T.ref_fit(mom, mom_abs, align)
                sums, dist, dmin = T.ref_errors(pn, gn, v, s, t, space, T.CLIP if space == "disparity" else None)
                assert dmin > 0 and dist > 1e-8 and (cond < 1e3).all(), (space, shape, align, dist, dmin, cond)
                d1 = sums[:, 5].sum() / sums[:, 0].sum()
                if align != "none":
                    assert 0.25 < d1 < 0.45, (space, shape, align, d1)


def test_temporal_inputs_keep_enough_pixels():
    """The reference keeps at least a fifth of the pixels of every pair of every temporal case; its sums are finite."""
    for ci, case in enumerate(T.TEMPORAL_CASES):
        N, H, W, _ = T.SHAPES[case[0]]
        _, _, sums = T.temporal_reference(ci)
        assert sums.shape == (N - case[6], 8) and np.isfinite(sums).all()
        assert (sums[:, 0] >= H * W / 5).all(), (T.TEMPORAL_IDS[ci], sums[:, 0] / (H * W))


def test_reference_on_a_hand_worked_pair():
    """2 × 2 frames.  Flow (½, 0) on the top row: pixel (0, 0) samples the mean of the later frame's top row, pixel
    (0, 1) leaves the frame.  Flow (0, 1) at (1, 0) leaves it too; flow (0, −1) at (1, 1) is the single tap (0, 1)."""
    p = np.array([[1.0, 2.0, 3.0, 4.0], [2.0, 4.0, 8.0, 16.0]])
    g = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 2.0, 1.0, 1.0]])
    flow = np.zeros((1, 2, 2, 2), np.float32)
    flow[0, 0, :, 0] = 0.5
    flow[0, 1, 0, 1] = 1.0
    flow[0, 1, 1, 1] = -1.0  # (1, 1) → (0, 1): a single tap
    sums = T.ref_temporal(p, g, None, flow, None, (np.ones(2), np.zeros(2)), 1, 2, 2)
    # pixel (0, 0): a' = 3, g' = 1.5 → Δa = 2, Δg = 0.5; pixel (1, 1): a' = 4, g' = 2 → Δa = 0, Δg = 1
    assert sums.tolist() == [[2.0, 2.0, 4.0, 2.5, 3.25, 1.5, 1.25, 1.0]]
    # an invalid tap (target outside the valid range) removes the pixel that needs it, and only that one
    g[1, 0] = 0.0
    assert T.ref_temporal(p, g, None, flow, None, (np.ones(2), np.zeros(2)), 1, 2, 2)[0, 0] == 1.0
