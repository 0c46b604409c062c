"""CPU side of the temporal filter: the new library symbol, the argument checks that run before any device work in
the C entry, in temporal_filter and in the pipeline's __call__, the properties of the restatement
(tests/stabilize_util.py) that the header states, and the f32-against-f64 ratio from which
tests/test_stabilize_gpu.py takes its tolerance."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from tests import stabilize_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDMI_E_ARG, RDMI_E_ALIGN, RDMI_E_UNSUPPORTED = 1001, 1002, 1003
F32, F64 = U.F32, U.F64


def test_new_symbol_declared_bound_and_exported():
    import rollingdepth_amd
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import stabilize as S

    hdr = open(os.path.join(ROOT, "include", "rdmi.h")).read()
    assert "Temporal filter (since rdmi_version 13)" in hdr
    name = "rdmi_temporal_filter"
    assert re.search(rf"\b{name}\s*\(", hdr)
    assert name in N_.EXPORTED and callable(getattr(N_.lib, name))
    assert N_.lib.rdmi_version() >= 13
    assert "#define RDMI_TFILTER_MAX_RADIUS 3" in hdr
    assert (K.TFILTER_MAX_RADIUS, S.MAX_RADIUS) == (3, 3)
    assert os.path.exists(os.path.join(ROOT, "rollingdepth_amd", "csrc", "tfilter.hip"))
    assert rollingdepth_amd.temporal_filter is S.temporal_filter
    # one launch's packed flow (8 B) and mask (1 B) stay within 1 GiB
    assert 9 * S._CHUNK_ELEMS <= 1 << 30


def _call(**over):
    """One call of the C entry with valid arguments (the pointers are dummies that are never dereferenced: every
    call below is refused before a launch) except for what `over` replaces; ("+", b) shifts the pointer by b bytes."""
    from rollingdepth_amd import _native as N_

    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    a = dict(depth=p, depth_dtype=N_.RDMI_F32, N=3, H=4, W=4, f0=0, n=3, radius=1, flow=p, valid=p, sigma_time=1.0,
             sigma_depth=0.05, out=p, stream=None)
    a.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    rc = N_.lib.rdmi_temporal_filter(*a.values())
    return rc, N_.lib.rdmi_last_error().decode()


def test_library_checks_run_before_any_launch():
    """Every rejected argument gets one call, on a machine without a GPU: nothing can have been launched."""
    from rollingdepth_amd import _native as N_

    nan, inf = math.nan, math.inf
    bad = [dict(depth=None), dict(flow=None), dict(out=None),
           dict(N=0), dict(H=0), dict(W=0), dict(n=0), dict(N=-1), dict(n=-2),
           dict(f0=-1), dict(f0=1), dict(f0=3, n=1), dict(n=4),
           dict(radius=0), dict(radius=4), dict(radius=-1),
           dict(depth_dtype=N_.RDMI_U8), dict(depth_dtype=7),
           dict(sigma_time=0.0), dict(sigma_time=-1.0), dict(sigma_time=nan), dict(sigma_time=inf),
           dict(sigma_time=1e-30), dict(sigma_time=1e30),
           dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=nan), dict(sigma_depth=inf),
           dict(sigma_depth=1e-30), dict(sigma_depth=1e30)]
    for kw in bad:
        rc, msg = _call(**kw)
        assert rc == RDMI_E_ARG and "temporal_filter" in msg, (kw, rc, msg)
    for kw, what in ((dict(flow=("+", 4)), "flow"), (dict(flow=("+", 1)), "flow"), (dict(out=("+", 2)), "out"),
                     (dict(out=("+", 1)), "out")):
        rc, msg = _call(**kw)
        assert rc == RDMI_E_ALIGN and f"{what} not" in msg, (kw, rc, msg)
    rc, msg = _call(H=1 << 16, W=(1 << 14) + 1)
    assert rc == RDMI_E_UNSUPPORTED and "2^30" in msg, (rc, msg)
    rc, msg = _call(N=1 << 20, n=1 << 20, H=1 << 15, W=1 << 15)
    assert rc == RDMI_E_UNSUPPORTED and "tiles" in msg, (rc, msg)


def test_check_stabilize_args():
    from rollingdepth_amd import stabilize as S

    d = torch.zeros((4, 6, 8))
    fr = torch.zeros((4, 3, 6, 8))
    u8 = torch.zeros((4, 6, 8, 3), dtype=torch.uint8)
    fl = torch.zeros((4, 4, 6, 8, 2))
    va = torch.ones((4, 4, 6, 8), dtype=torch.uint8)
    assert S.check_stabilize_args(d, fr) == (4, 6, 8)
    assert S.check_stabilize_args(d[:, None].half(), u8, radius=3, flow_kwargs={"radius": 2, "levels": 1}) == (4, 6, 8)
    assert S.check_stabilize_args(d, flow=fl, valid=va) == (4, 6, 8)
    assert S.check_stabilize_args(d, flow=fl[:2], radius=1) == (4, 6, 8)
    assert S.check_stabilize_args(d[:1], fr[:1]) == (1, 6, 8)
    for kw in (dict(depth=None), dict(depth=[1.0]), dict(depth=d.double()), dict(depth=d.long()),
               dict(frames=fr.long()), dict(frames="video.mp4"), dict(frames=None, flow=fl.double()),
               dict(frames=None, flow=fl, valid=va.bool()), dict(radius=True), dict(radius=2.0), dict(radius="2"),
               dict(sigma_time=True), dict(sigma_time="1"), dict(sigma_depth=None), dict(sigma_depth=False),
               dict(flow_kwargs=[("radius", 2)]), dict(flow_kwargs={"radius": 2.5}),
               dict(flow_kwargs={"iterations": True}), dict(flow_kwargs={"fb_tol": 0.5}), dict(return_flow=1)):
        a = dict(dict(depth=d, frames=fr), **kw)
        with pytest.raises(TypeError):
            S.check_stabilize_args(**a)
    for kw in (dict(frames=None), dict(flow=fl), dict(frames=None, valid=va),
               dict(frames=None, flow=fl, flow_kwargs={"radius": 2}),
               dict(radius=0), dict(radius=4), dict(sigma_time=0.0), dict(sigma_time=-1.0), dict(sigma_time=math.nan),
               dict(sigma_depth=0.0), dict(sigma_depth=math.inf), dict(sigma_depth=1e-30), dict(sigma_depth=1e30),
               dict(depth=d[0]), dict(depth=torch.zeros((4, 2, 6, 8))), dict(depth=d[:, :0]),
               dict(frames=fr[:3]), dict(frames=fr[:, :2]), dict(frames=fr[..., :7]), dict(frames=fr[0]),
               dict(frames=torch.zeros((4, 3, 12, 16))), dict(frames=u8[:, :5]), dict(frames=u8.permute(0, 3, 1, 2)),
               dict(frames=None, flow=fl, radius=1), dict(frames=None, flow=fl[:, :3]),
               dict(frames=None, flow=fl, valid=va[:2]), dict(frames=None, flow=fl[..., :1]),
               dict(flow_kwargs={"frame_step": 2}), dict(flow_kwargs={"backward": False}),
               dict(flow_kwargs={"radius": 9}), dict(flow_kwargs={"iterations": 0}),
               dict(flow_kwargs={"damping": -1.0}), dict(flow_kwargs={"fb_tol": (0.1,)})):
        a = dict(dict(depth=d, frames=fr), **kw)
        with pytest.raises(ValueError):
            S.check_stabilize_args(**a)
    # the public function refuses before it touches a device
    with pytest.raises(ValueError, match="exactly one"):
        S.temporal_filter(d)
    with pytest.raises(ValueError, match="exactly one"):
        S.temporal_filter(d, fr, flow=fl)
    with pytest.raises(ValueError, match="resize the frames"):
        S.temporal_filter(d, torch.zeros((4, 3, 12, 16)))
    p = inspect.signature(S.temporal_filter).parameters
    assert [p[k].default for k in ("radius", "sigma_time", "sigma_depth", "flow_kwargs", "return_flow")] == [
        2, 1.0, 0.05, None, False]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("flow", "valid", "radius", "return_flow"))


def test_pipeline_check_stabilize():
    from rollingdepth_amd.pipeline import RollingDepthPipeline, check_stabilize

    assert check_stabilize(False) == (False, {})
    assert check_stabilize(True, None) == (True, {})
    kw = {"radius": 3, "sigma_depth": 0.1, "flow_kwargs": {"radius": 3}}
    assert check_stabilize(True, kw) == (True, kw)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(TypeError, match="stabilize"):
            check_stabilize(bad)
    for bad in ({"sigma": 1.0}, {"frames": None}, {"return_flow": True}, [("radius", 2)], "radius", 2):
        with pytest.raises(ValueError, match="stabilize_kwargs"):
            check_stabilize(True, bad)
    with pytest.raises(ValueError, match="stabilize_kwargs"):
        check_stabilize(False, {"radius": 2})
    with pytest.raises(ValueError, match="radius"):
        check_stabilize(True, {"radius": 4})
    with pytest.raises(TypeError, match="sigma_time"):
        check_stabilize(True, {"sigma_time": True})
    with pytest.raises(ValueError, match="flow_kwargs"):
        check_stabilize(True, {"flow_kwargs": {"window": 3}})
    p = inspect.signature(RollingDepthPipeline.__call__).parameters
    assert p["stabilize"].default is False and p["stabilize_kwargs"].default is None
    # self = None and no GPU: raised before the pipeline or a device is touched
    fr = torch.zeros((5, 3, 8, 8))
    with pytest.raises(TypeError, match="stabilize"):
        RollingDepthPipeline.__call__(None, fr, stabilize=1)
    with pytest.raises(ValueError, match="stabilize_kwargs"):
        RollingDepthPipeline.__call__(None, fr, stabilize=True, stabilize_kwargs={"sigma": 1})
    with pytest.raises(ValueError, match="sigma_depth"):
        RollingDepthPipeline.__call__(None, fr, stabilize=True, stabilize_kwargs={"sigma_depth": 0.0})


def _random_flow(R, N, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((2 * R, N, H, W, 2), generator=g, dtype=F64) * 2 - 1) * amp).to(F32)


def test_constant_video_is_exact_in_f32():
    """The lerp form gives equal taps back exactly whatever wx and wy are, δ is then 0 and the quotient +0: a
    constant video comes out bit for bit, in f32 as in f64, for flows that land anywhere."""
    R, N, H, W = 2, 5, 9, 11
    flow = _random_flow(R, N, H, W, 1)
    for c in (0.7319, -3.0e5, 1.0e-12):
        d = torch.full((N, H, W), c, dtype=F32)
        for dt in (F32, F64):
            assert torch.equal(U.restate(d, flow, None, R, dt=dt), d.to(dt))
    h = torch.full((N, H, W), 0.1234, dtype=U.F16)
    assert torch.equal(U.restate(h, flow, None, R, dt=F32), h.float())


def test_identities():
    """N = 1, all-invalid neighbours and flows that all leave the frame return the input, bitwise."""
    R, N, H, W = 2, 4, 7, 9
    g = torch.Generator().manual_seed(2)
    d = torch.randn((N, H, W), generator=g, dtype=F64).to(F32)
    flow = _random_flow(R, N, H, W, 3)
    for dt in (F32, F64):
        assert torch.equal(U.restate(d[:1], flow[:, :1], None, R, dt=dt), d[:1].to(dt))
        assert torch.equal(U.restate(d, flow, torch.zeros((2 * R, N, H, W), dtype=torch.uint8), R, dt=dt), d.to(dt))
        assert torch.equal(U.restate(d, flow + 100.0, None, R, dt=dt), d.to(dt))
        assert torch.equal(U.restate(d, torch.full_like(flow, math.nan), None, R, dt=dt), d.to(dt))
        assert not torch.equal(U.restate(d, flow, None, R, dt=dt), d.to(dt))


def _scene(N, H, W, d, noise=0.0, seed=0):
    """A smooth scene that moves by the integer d = (dx, dy) per frame, f32 [N, H, W], and its packed true flow
    (slot k: k·d) for radius R = 2."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    f = lambda X, Y: 2.0 + 0.5 * torch.sin(0.21 * X + 0.3) * torch.cos(0.17 * Y) + 0.2 * torch.sin(0.11 * (X + Y))
    D = torch.stack([f(xs - i * d[0], ys - i * d[1]) for i in range(N)])
    if noise:
        D = D + noise * torch.randn(D.shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
    R = 2
    flow = torch.zeros((2 * R, N, H, W, 2), dtype=F32)
    for s in range(2 * R):
        k = U.slot_offset(s, R)
        flow[s, ..., 0], flow[s, ..., 1] = k * d[0], k * d[1]
    return D.to(F32), flow


def test_noise_free_scene_under_integer_flow_is_reproduced():
    """With the true integer flow every tap is the pixel's own value in the neighbouring frame: δ = 0 exactly, so
    the interior (R·|d| pixels from the border) comes out unchanged; zero flow on a still scene likewise, at
    every pixel."""
    N, H, W, R = 6, 24, 28, 2
    for d in ((0, 0), (2, 1), (-1, 3)):
        D, flow = _scene(N, H, W, d)
        m = R * max(abs(d[0]), abs(d[1]))
        for dt in (F32, F64):
            out = U.restate(D, flow, None, R, dt=dt)
            err = (out - D.to(dt)).abs()[:, m:H - m, m:W - m].max().item()
            print(f"d = {d}, {dt}: largest interior change {err}")
            assert err == 0.0


def test_noise_variance_falls_as_the_weights_say():
    """sigma_depth huge switches the range term off: on i.i.d. noise the interior frames' error variance falls to
    (1 + Σ g²) / (1 + Σ g)², 0.287 at R = 2, σt = 1.  20 480 samples: the estimator's relative standard deviation is
    about 1 %, the 5 % allowed about five of them."""
    N, H, W, R = 9, 64, 64, 2
    want = U.variance_ratio(R, 1.0)
    assert abs(want - 0.287) < 5e-4
    D, flow = _scene(N, H, W, (0, 0), noise=0.01, seed=11)
    truth, _ = _scene(N, H, W, (0, 0))
    out = U.restate(D, flow, None, R, 1.0, 1e3)
    before = (D.double() - truth.double())[R:N - R]
    after = (out - truth.double())[R:N - R]
    got = (after.pow(2).mean() / before.pow(2).mean()).item()
    print(f"variance ratio {got:.4f}, expected {want:.4f}")
    assert abs(got / want - 1.0) <= 0.05


def test_range_term_keeps_a_moving_depth_step():
    """One frame's step is displaced by two pixels under zero flow.  With sigma_depth = 0.05 the unit jump weighs
    exp(−200): every frame passes unchanged to 1e-6.  With sigma_depth = 1e3 the displaced pixels are pulled by
    Σg / (1 + Σg) = 0.597 towards their neighbours: this is what the range term buys."""
    N, H, W, R = 5, 6, 16, 2
    D = torch.zeros((N, H, W), dtype=F32)
    D[..., 8:] = 1.0
    D[2, :, 8:10] = 0.0  # frame 2: the step at column 10
    flow = torch.zeros((2 * R, N, H, W, 2), dtype=F32)
    for dt in (F32, F64):
        keep = U.restate(D, flow, None, R, 1.0, 0.05, dt=dt)
        assert (keep - D.to(dt)).abs().max().item() < 1e-6
        smear = U.restate(D, flow, None, R, 1.0, 1e3, dt=dt)
        moved = (smear - D.to(dt))[2, :, 8:10]
        print(f"{dt}: the displaced pixels move by {moved.min().item():.4f} … {moved.max().item():.4f}")
        assert moved.min().item() > 0.5


def test_restatement_honours_chunks_and_non_finite_pixels():
    """Rows f0 … f0 + n − 1 of the whole-video result equal the chunk's, and the planted NaN pixel stays NaN while its
    reader skips it."""
    ci = 2
    N, H, W, R = U.GPU_CASES[ci]
    depth, flow, valid = U.gpu_inputs(ci, F32)
    ref, rng = U.gpu_reference(ci, F32)
    part = U.restate(depth, flow[:, 1:4].contiguous(), valid[:, 1:4].contiguous(), R, f0=1, n=3)
    assert torch.equal(part.isnan(), ref[1:4].isnan()) and torch.equal(part.nan_to_num(), ref[1:4].nan_to_num())
    fn, yn, xn = U.nan_pixel(ci)
    assert torch.isnan(ref[fn, yn, xn]) and int(torch.isnan(ref).sum()) == 1
    assert torch.isfinite(ref[0, yn, xn]) and (rng[torch.isfinite(ref)] > 0).all()


def test_f32_ratio_behind_the_gpu_tolerance():
    """U.F32_RATIO is the worst |f32 restatement − f64| / tap_range over all 10 GPU variants; re-measured here on every
    one of them, so that the constant cannot drift from the code."""
    worst = 0.0
    for ci, dt in U.all_gpu_variants():
        depth, flow, valid = U.gpu_inputs(ci, dt)
        ref, rng = U.gpu_reference(ci, dt)
        got = U.restate(depth, flow, valid, U.GPU_CASES[ci][3], dt=F32)
        q = U.ratio(got, ref, rng)
        fin = torch.isfinite(ref)
        med = ((got.double() - ref).abs()[fin] / rng[fin]).median().item()
        print(f"case {U.GPU_CASES[ci]} {dt}: worst ratio {q:.3e}, median {med:.3e}")
        assert q == U.f32_ratio(ci, dt)
        worst = max(worst, q)
    print(f"worst ratio {worst:.3e}; F32_RATIO {U.F32_RATIO:.3e}, TOL_REL {U.TOL_REL:.3e}")
    assert 0.5 * U.F32_RATIO <= worst <= U.F32_RATIO
    assert U.TOL_REL == 4 * U.F32_RATIO
