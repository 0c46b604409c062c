"""CPU side of rollingdepth_amd.metrics: the argument checks that run before any device work, the result
type, the pooling of frame sums (mocked sums), and librdmi's own checks of the depth-metric calls, which
return before any launch."""
import dataclasses
import math

import pytest
import torch


def _ok(n=2, h=4, w=5):
    return torch.rand(n, h, w) + 0.5, torch.rand(n, h, w) + 0.5, torch.ones(n, h, w, dtype=torch.bool)


def test_public_names():
    import rollingdepth_amd as R
    from rollingdepth_amd import metrics as M

    assert R.depth_metrics is M.depth_metrics and R.align_scale_shift is M.align_scale_shift
    assert R.DepthMetrics is M.DepthMetrics
    names = [f.name for f in dataclasses.fields(M.DepthMetrics)]
    assert names == ["abs_rel", "sq_rel", "mae", "rmse", "delta1", "delta2", "delta3", "n_valid", "scale", "shift",
                     "per_frame", "frames_skipped"]


@pytest.mark.parametrize("fn", ["depth_metrics", "align_scale_shift"])
def test_value_and_type_errors_come_before_any_device_work(fn):
    from rollingdepth_amd import metrics as M

    call = getattr(M, fn)
    p, g, m = _ok()
    with pytest.raises(ValueError, match="does not match"):
        call(p, g[:, :3])
    with pytest.raises(ValueError, match="does not match"):
        call(p, g, m[:1])
    with pytest.raises(ValueError, match="does not match"):
        call(p[:, None], g[:, None], m[:, None, :, :4])
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        call(p[0], g[0])
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        call(p[:, None].expand(-1, 3, -1, -1), g)
    with pytest.raises(ValueError, match="empty"):
        call(p[:0], g[:0])
    with pytest.raises(ValueError, match="valid_range"):
        call(p, g, valid_range=(1.0, 1.0))
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p.double(), g)
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p, g.to(torch.bfloat16))
    with pytest.raises(TypeError, match="float16 or float32"):
        call(p, (g * 10).long())
    with pytest.raises(TypeError, match="bool or uint8"):
        call(p, g, m.float())
    with pytest.raises(TypeError, match="tensor"):
        call(p.numpy(), g)


def test_depth_metrics_rejects_unknown_align_and_bad_clip():
    from rollingdepth_amd.metrics import depth_metrics

    p, g, m = _ok()
    with pytest.raises(ValueError, match="align"):
        depth_metrics(p, g, m, align="snippet")
    with pytest.raises(ValueError, match="align"):
        depth_metrics(p, g, m, align=None)
    with pytest.raises(ValueError, match="clip"):
        depth_metrics(p, g, m, clip=(2.0, 1.0))
    with pytest.raises(ValueError, match="clip"):
        depth_metrics(p, g, m, clip=(math.nan, 1.0))


def test_pool_adds_frames_and_divides_by_n():
    from rollingdepth_amd.metrics import _pool

    sums = torch.tensor([[4.0, 2.0, 1.0, 8.0, 3.0, 4.0, 4.0, 4.0],
                         [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                         [12.0, 2.0, 3.0, 56.0, 5.0, 4.0, 8.0, 12.0]], dtype=torch.float64)
    scale = torch.tensor([1.5, math.nan, 2.0], dtype=torch.float64)
    shift = torch.tensor([0.25, math.nan, 0.0], dtype=torch.float64)
    m = _pool(sums, scale, shift)
    assert (m.n_valid, m.frames_skipped) == (16, [1])
    assert (m.mae, m.abs_rel, m.sq_rel, m.rmse) == (0.25, 0.25, 0.5, 2.0)
    assert (m.delta1, m.delta2, m.delta3) == (0.5, 0.75, 1.0)
    assert m.per_frame is sums and m.scale is scale and m.shift is shift
    assert all(isinstance(getattr(m, k), float) for k in ("abs_rel", "sq_rel", "mae", "rmse", "delta1", "delta3"))


def test_pool_of_nothing_is_nan_and_does_not_raise():
    from rollingdepth_amd.metrics import _pool

    nan = torch.full((2,), math.nan, dtype=torch.float64)
    m = _pool(torch.zeros((2, 8), dtype=torch.float64), nan, nan.clone())
    assert m.n_valid == 0 and m.frames_skipped == [0, 1]
    for k in ("abs_rel", "sq_rel", "mae", "rmse", "delta1", "delta2", "delta3"):
        assert math.isnan(getattr(m, k)), k


def test_workspace_depends_on_n_and_p_only():
    from rollingdepth_amd._native import lib

    w = lib.rdmi_depth_metrics_workspace
    assert w(1, 1) == w(1, 4096) == 8 and w(1, 4097) == 16 and w(7, 4097) == 7 * 16
    assert w(1, 768 * 768) == 144 * 8 and w(1, 1 << 30) == 256 * 8  # capped: larger frames are grid-strided
    assert w(0, 10) == 0 and w(3, 0) == 0


def test_library_checks_run_before_any_launch():
    """RDMI_E_ARG for every bad argument of the three calls — on a machine without a GPU, so nothing can have
    been launched.  The pointers are never dereferenced."""
    from rollingdepth_amd import _native as N_

    lib, inf, x = N_.lib, math.inf, 4096  # x: a non-null pointer value
    mom = lambda *a: lib.rdmi_depth_moments(*a, None)  # noqa: E731
    err = lambda *a: lib.rdmi_depth_errors(*a, None)  # noqa: E731
    fit = lambda *a: lib.rdmi_depth_fit(*a, None)  # noqa: E731
    bad = {
        "moments pred null": mom(None, 1, x, 1, None, 2, 9, 1e-3, inf, x),
        "moments target null": mom(x, 1, None, 1, None, 2, 9, 1e-3, inf, x),
        "moments workspace null": mom(x, 1, x, 1, None, 2, 9, 1e-3, inf, None),
        "moments N": mom(x, 1, x, 1, None, 0, 9, 1e-3, inf, x),
        "moments P": mom(x, 1, x, 1, None, 2, 0, 1e-3, inf, x),
        "moments pred dtype": mom(x, 2, x, 1, None, 2, 9, 1e-3, inf, x),
        "moments target dtype": mom(x, 0, x, -1, None, 2, 9, 1e-3, inf, x),
        "moments lo == hi": mom(x, 0, x, 0, None, 2, 9, 1.0, 1.0, x),
        "moments lo > hi": mom(x, 0, x, 0, x, 2, 9, inf, 1.0, x),
        "moments nan range": mom(x, 0, x, 0, x, 2, 9, math.nan, 1.0, x),
        "fit mode": fit(x, 2, 9, 3, x, x),
        "fit N": fit(x, 0, 9, 1, x, x),
        "fit P": fit(x, 2, -9, 1, x, x),
        "fit st null": fit(x, 2, 9, 1, x, None),
        "fit moments null": fit(x, 2, 9, 2, None, x),
        "fit workspace null": fit(None, 2, 9, 2, x, x),
        "fit none st null": fit(None, 2, 9, 0, None, None),
        "errors pred null": err(None, 1, x, 1, None, 2, 9, 1e-3, inf, x, -inf, inf, x, x),
        "errors st null": err(x, 1, x, 1, None, 2, 9, 1e-3, inf, None, -inf, inf, x, x),
        "errors sums null": err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, -inf, inf, x, None),
        "errors workspace null": err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, -inf, inf, None, x),
        "errors dtype": err(x, 1, x, 3, None, 2, 9, 1e-3, inf, x, -inf, inf, x, x),
        "errors N": err(x, 1, x, 1, None, -2, 9, 1e-3, inf, x, -inf, inf, x, x),
        "errors lo >= hi": err(x, 1, x, 1, None, 2, 9, 2.0, 1.0, x, -inf, inf, x, x),
        "errors clip": err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, 1.0, 0.5, x, x),
        "errors nan clip": err(x, 1, x, 1, None, 2, 9, 1e-3, inf, x, math.nan, 0.5, x, x),
    }
    assert all(rc == 1001 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc != 1001}
    assert b"clip" in lib.rdmi_last_error()
    with pytest.raises(N_.RdmiError, match="clip"):
        N_.check(1001, "rdmi_depth_errors")
    assert lib.rdmi_version() >= 5
