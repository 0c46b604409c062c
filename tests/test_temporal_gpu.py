"""The alignment spaces and the temporal pass of rollingdepth_amd.metrics on the device against the numpy f64
reference of tests/temporal_util.py.

Bounds.  n and every count are compared exactly; error and temporal sums to relative 1e-10, the project's bound
for sums of up to 2e4 terms whose aligned values differ by one rounding (fma on the device, s * p + t in numpy).

Moments in the disparity and log spaces.  In depth space the six terms are exact in f64 and the only error is the
summation's, |Δ| ≤ n · 2⁻⁵² · Σ|terms| (tests/test_metrics_gpu.py).  φ = 1 / g and φ = ln g are full f64 values, which
adds two ingredients: (i) p·φ and φ·φ are rounded in numpy (a product, then the sum) and not on the device (fma):
2⁻⁵³ relative per term; (ii) the device's and numpy's `log` are each within 1 ulp = 2⁻⁵² of ln g, so they differ by at
most c · 2⁻⁵³ with c = 4, which reaches φ and p·φ once and φ·φ twice (the IEEE division of the disparity space is
the same on both sides: c = 0).  Together
    |Δ| ≤ (2n + 1 + 2c) · 2⁻⁵³ · Σ|terms|  =: ε · Σ|terms|.
Fit.  s = (n·Σpφ − Σp·Σφ) / det, t = (Σp²·Σφ − Σp·Σpφ) / det, det = n·Σp² − (Σp)².  With every moment off by at most
ε of its Σ|terms|, a numerator is off by ε·(n·Σ|pφ| + 2·Σ|p|·Σ|φ|) resp. ε·(Σp²·Σ|φ| + 2·Σ|p|·Σ|pφ|) and det by
ε·(n·Σp² + 2·(Σ|p|)²); dividing each by the quantity itself gives the conditioning κ that temporal_util.ref_solve
returns (numerator's + determinant's).  The relative error of s and t is then ε·κ to first order; the test allows
2·ε·κ + 8·2⁻⁵³, the factor 2 for the second-order terms and the 8 roundings of the solve itself.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import temporal_util as T

pytestmark = pytest.mark.gpu
F16, F32 = T.F16, T.F32
LOG_ULPS = {"depth": 0, "disparity": 0, "log": 4}
POOLED = ("flicker", "flicker_rmse", "tge", "tge_rmse", "target_change", "change_corr")


def cuda(t):
    return None if t is None else t.cuda()


def rel_err(got, ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ref == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / np.abs(ref))


def assert_pooled(out, ref, tol=1e-10):
    for k in POOLED:
        x, y = getattr(out, k), ref[k]
        assert (math.isnan(x) and math.isnan(y)) or math.isclose(x, y, rel_tol=tol, abs_tol=tol), (k, x, y)


# ----------------------------------------------------------------------------- 1. disparity and log spaces
@functools.lru_cache(maxsize=None)
def space_reference(space, ci):
    shape, pd, td, mk = T.SPACE_CASES[ci]
    p, gt, m = T.inputs(shape, space)
    pn, gn = T.f64(p.to(pd)), T.f64(gt.to(td))
    v = T.ref_valid(pn, gn, m.numpy() if mk else None, space=space)
    mom, mom_abs = T.ref_moments(pn, gn, v, space)
    ref = {"mom": mom, "mom_abs": mom_abs}
    for align in ("video", "frame", "none"):
        s, t, cond = T.ref_fit(mom, mom_abs, align)
        sums, dist, dmin = T.ref_errors(pn, gn, v, s, t, space, T.CLIP if space == "disparity" else None)
        assert dist > 1e-10, f"a test input lies {dist:.1e} from a δ threshold: counts are not comparable"
        assert space != "disparity" or dmin > 0, "an aligned disparity <= 0 in the comparison inputs"
        ref[align] = (s, t, cond, sums)
    return ref


@pytest.mark.parametrize("ci", range(len(T.SPACE_CASES)), ids=T.SPACE_IDS)
@pytest.mark.parametrize("space", ["disparity", "log"])
def test_space_moments_fit_and_errors(space, ci):
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.metrics import align_scale_shift, depth_metrics

    shape, pd, td, mk = T.SPACE_CASES[ci]
    p, gt, m = T.inputs(shape, space)
    p, g, m = p.to(pd).cuda(), gt.to(td).cuda(), (m.cuda() if mk else None)
    N, P = p.shape[0], p.shape[1] * p.shape[2]
    ref = space_reference(space, ci)
    n = ref["mom"][:, 0]
    c = LOG_ULPS[space]
    # moments
    mu8 = None if m is None else m.view(torch.uint8).view(N, P)
    ws = K.depth_moments(p.view(N, P), g.view(N, P), mu8, T.LO, math.inf, space=K.DEPTH_SPACES[space])
    mom = K.depth_fit(ws, N, P, K.DEPTH_FIT_MODES["frame"])[0].cpu().numpy()
    err, bound = np.abs(mom - ref["mom"]), ((2 * n + 1 + 2 * c) * T.U)[:, None] * ref["mom_abs"]
    print("moments: max |Δ| / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(mom[:, 0], n)
    assert (err <= bound).all(), (err, bound)
    # fit
    for per_frame in (False, True):
        s, t, _ = align_scale_shift(p, g, m, per_frame=per_frame, space=space)
        rs, rt, cond, _ = ref["frame" if per_frame else "video"]
        nn = n if per_frame else np.full(N, n.sum())
        tol = 2 * (2 * nn + 1 + 2 * c) * T.U * cond + 8 * T.U
        es, et = np.abs(s.numpy() - rs) / np.abs(rs), np.abs(t.numpy() - rt) / np.abs(rt)
        print("fit: max rel err / tol", (es / tol).max(), (et / tol).max(), "tol", tol.max())
        assert (es <= tol).all() and (et <= tol).all(), (es, et, tol)
    # errors
    for align in ("video", "frame", "none"):
        out = depth_metrics(p, g, m, align=align, space=space, clip=T.CLIP if space == "disparity" else None)
        sums = ref[align][3]
        got = out.per_frame.numpy()
        assert np.array_equal(got[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]]), (got, sums)
        assert 0 < sums[:, 5].sum() < sums[:, 0].sum()  # the counts are not trivially 0 or n
        rel = rel_err(got[:, 1:5], sums[:, 1:5])
        print("errors: max rel Δ of the sums", rel.max())
        assert (rel <= 1e-10).all(), rel
        want = T.ref_metrics(sums)
        for k, y in want.items():
            assert math.isclose(getattr(out, k), y, rel_tol=1e-10, abs_tol=1e-10), (k, getattr(out, k), y)


# ----------------------------------------------------------------------------- 2. space="depth" is the old call
@pytest.mark.parametrize("ci", [3, 7, 12, 17], ids=lambda ci: T.SPACE_IDS[ci])
def test_depth_space_through_the_new_entry_points_gives_the_old_bits(ci):
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K

    shape, pd, td, mk = T.SPACE_CASES[ci]
    p, gt, m = T.inputs(shape)
    N, P = p.shape[0], p.shape[1] * p.shape[2]
    p, g = p.to(pd).cuda().view(N, P), gt.to(td).cuda().view(N, P)
    m = m.cuda().view(torch.uint8).view(N, P) if mk else None
    lib, code, dev = N_.lib, {F16: N_.RDMI_F16, F32: N_.RDMI_F32}, p.device
    mp = None if m is None else m.data_ptr()
    for mode in ("video", "frame"):
        ws_old = K.depth_moments(p, g, m, T.LO, math.inf, torch.full_like(K.depth_metrics_workspace(N, P, dev), -7.0))
        ws_new = torch.full_like(ws_old, -7.0)
        N_.check(lib.rdmi_depth_moments_space(p.data_ptr(), code[pd], g.data_ptr(), code[td], mp, N, P, T.LO, math.inf,
                                              N_.RDMI_SPACE_DEPTH, ws_new.data_ptr(), None))
        assert T.same_bits(ws_old, ws_new)
        mom_old, st_old = K.depth_fit(ws_old, N, P, K.DEPTH_FIT_MODES[mode])
        mom_new, st_new = K.depth_fit(ws_new, N, P, K.DEPTH_FIT_MODES[mode])
        assert T.same_bits(mom_old, mom_new) and T.same_bits(st_old, st_new)
        for clip in ((-math.inf, math.inf), (0.75, 1.5)):
            sums_old = K.depth_errors(p, g, m, st_old, T.LO, math.inf, *clip, ws_old)
            sums_new = torch.empty_like(sums_old)
            N_.check(lib.rdmi_depth_errors_space(p.data_ptr(), code[pd], g.data_ptr(), code[td], mp, N, P, T.LO,
                                                 math.inf, st_new.data_ptr(), N_.RDMI_SPACE_DEPTH, *clip,
                                                 ws_new.data_ptr(), sums_new.data_ptr(), None))
            assert T.same_bits(sums_old, sums_new) and T.same_bits(ws_old, ws_new)
            assert sums_old[:, 0].sum() > 0


# ----------------------------------------------------------------------------- 3. non-positive aligned disparity
def test_non_positive_aligned_disparity():
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.metrics import depth_metrics

    shape = T.SHAPES[1]
    p, gt, m = T.inputs(shape, "disparity")
    N, P = p.shape[0], p.shape[1] * p.shape[2]
    gt = gt.float()
    pn, gn = T.f64(p), T.f64(gt)
    v = T.ref_valid(pn, gn, m.numpy(), space="disparity")
    s, t = np.full(N, -1.0), np.full(N, 0.5)  # d = 0.5 − p, exact on both sides: d <= 0 wherever p >= 0.5
    bad = v & (pn >= 0.5)
    assert bad.sum() > P // 4 and (v & ~bad).sum() > P // 4
    st = torch.tensor(np.stack([s, t], 1), device="cuda")
    dp, dg, dm = p.cuda().view(N, P), gt.cuda().view(N, P), m.cuda().view(torch.uint8).view(N, P)
    sp = K.DEPTH_SPACES["disparity"]
    # with a clip the pixels sit at the cap: counted, above every δ threshold, finite sums
    sums, dist, dmin = T.ref_errors(pn, gn, v, s, t, "disparity", T.CLIP)
    assert dist > 1e-10 and dmin <= 0
    only_bad, _, _ = T.ref_errors(pn, gn, bad, s, t, "disparity", T.CLIP)
    assert (only_bad[:, 0] == bad.sum(1)).all() and (only_bad[:, 5:] == 0).all()  # a = 10 passes no δ test
    got = K.depth_errors(dp, dg, dm, st, T.LO, math.inf, *T.CLIP, space=sp).cpu().numpy()
    assert np.array_equal(got[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]]) and (got[:, 0] == v.sum(1)).all()
    assert (rel_err(got[:, 1:5], sums[:, 1:5]) <= 1e-10).all()
    # without one they are +inf: still counted, still above every threshold, and the sums say so
    sums, dist, _ = T.ref_errors(pn, gn, v, s, t, "disparity", None)
    assert dist > 1e-10 and np.isinf(sums[:, 1:5]).all()
    got = K.depth_errors(dp, dg, dm, st, T.LO, math.inf, space=sp).cpu().numpy()
    assert np.array_equal(got[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]])
    assert np.isinf(got[:, 1:5]).all() and (got[:, 1:5] > 0).all()
    # which is why the Python layer asks for the cap
    for clip in (None, (0.1, math.inf)):
        with pytest.raises(ValueError, match="finite upper clip"):
            depth_metrics(p.cuda(), gt.cuda(), m.cuda(), space="disparity", clip=clip)


# ----------------------------------------------------------------------------- 4. temporal pass against numpy
def run_case(ci, **over):
    from rollingdepth_amd.metrics import temporal_metrics

    p, g, m, flow, pm, kw = T.temporal_case(ci)
    kw = {**kw, **over}
    return temporal_metrics(cuda(p), cuda(g), cuda(m), flow=cuda(flow), pair_mask=cuda(pm), **kw)


def assert_sums_match(got, sums, has_target, P, tol=1e-10):
    assert got.shape == sums.shape
    assert (sums[:, 0] >= P / 5).all(), sums[:, 0]  # the reference keeps pixels: dropping everything cannot pass
    assert np.array_equal(got[:, 0], sums[:, 0]), (got[:, 0], sums[:, 0])
    rel = rel_err(got[:, 1:], sums[:, 1:])
    print("temporal: max rel Δ of the sums", rel.max())
    assert (rel <= tol).all(), rel
    if not has_target:
        assert (got[:, 3:] == 0).all()
    else:
        assert (np.abs(sums[:, 1:7]) > 0).all()


@pytest.mark.parametrize("ci", range(len(T.TEMPORAL_CASES)), ids=T.TEMPORAL_IDS)
def test_temporal_against_numpy(ci):
    case = T.TEMPORAL_CASES[ci]
    N, H, W, _ = T.SHAPES[case[0]]
    out = run_case(ci)
    s, t, sums = T.temporal_reference(ci)
    assert out.per_pair.shape == (N - case[6], 8) and not out.per_pair.is_cuda and out.pairs_skipped == []
    assert np.allclose(out.scale.numpy(), s, rtol=1e-9, atol=0)
    assert np.allclose(out.shift.numpy(), t, rtol=1e-9, atol=1e-300)
    assert_sums_match(out.per_pair.numpy(), sums, case[2] is not None, H * W)
    assert out.n_valid == int(sums[:, 0].sum())
    assert_pooled(out, T.ref_temporal_metrics(sums, case[2] is not None))
    if case[2] is None:
        assert all(math.isnan(getattr(out, k)) for k in POOLED[2:])


# ----------------------------------------------------------------------------- 5. exact invariants
@pytest.mark.parametrize("ci", [2, 7, 18, 23], ids=lambda ci: T.TEMPORAL_IDS[ci])
def test_zero_flow_is_no_flow(ci):
    from rollingdepth_amd.metrics import temporal_metrics

    p, g, m, flow, pm, kw = T.temporal_case(ci)
    a = temporal_metrics(cuda(p), cuda(g), cuda(m), flow=None, pair_mask=cuda(pm), **kw)
    b = temporal_metrics(cuda(p), cuda(g), cuda(m), flow=torch.zeros_like(flow).cuda(), pair_mask=cuda(pm), **kw)
    c = temporal_metrics(cuda(p), cuda(g), cuda(m), flow=(-torch.zeros_like(flow)).cuda(), pair_mask=cuda(pm), **kw)
    assert a.n_valid > 0 and T.same_bits(a.per_pair, b.per_pair) and T.same_bits(a.per_pair, c.per_pair)


def test_identical_frames_do_not_flicker():
    from rollingdepth_amd.metrics import temporal_metrics

    p, gt, m = T.inputs(T.SHAPES[1])
    p, gt, m = (t[:1].expand(3, -1, -1).contiguous().cuda() for t in (p, gt.float(), m))
    for align in ("video", "frame", "none"):
        out = temporal_metrics(p, gt, m, align=align, frame_step=2 if align == "frame" else 1)
        assert out.n_valid > 0 and (out.per_pair[:, 1:] == 0).all()
        assert out.flicker == 0.0 and out.flicker_rmse == 0.0 and out.tge == 0.0 and math.isnan(out.change_corr)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_pred_equal_to_target_has_no_gradient_error(dtype):
    from rollingdepth_amd.metrics import temporal_metrics

    shape = T.SHAPES[2]
    _, gt, _ = T.inputs(shape)
    flow, m, pm = T.temporal_inputs(shape, 1)
    x = gt.to(dtype).cuda()
    for fl in (None, flow.cuda()):
        out = temporal_metrics(x, x, m.cuda(), flow=fl, pair_mask=pm.cuda(), align="none")
        pp = out.per_pair
        assert (pp[:, 0] > 0).all() and (pp[:, 1] > 0).all()
        assert (pp[:, 3] == 0).all() and (pp[:, 4] == 0).all() and out.tge == 0.0 and out.tge_rmse == 0.0
        assert T.same_bits(pp[:, 1], pp[:, 5]) and T.same_bits(pp[:, 2], pp[:, 6]) and T.same_bits(pp[:, 2], pp[:, 7])
        assert math.isclose(out.change_corr, 1.0, rel_tol=1e-15)


@pytest.mark.parametrize("shape", T.SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_integer_flow_is_a_shift(shape):
    """flow = (1, 0): frame f at (y, x) against frame f + 1 at (y, x + 1), a single tap of weight 1.  With
    align="none" every Δ is exact in f64 on both sides (p on the 2⁻¹⁰ grid, targets f32 of one binade range; only
    (Δa − Δg)² and Δa·Δg are rounded, once, 2⁻⁵³), so the sums differ by their order of addition alone: the tighter
    of the two routes to a bound, |Δ| ≤ n · 2⁻⁵² · Σ|terms|, stands in for the relative 1e-10."""
    from rollingdepth_amd.metrics import temporal_metrics

    N, H, W, _ = shape
    p, gt, m = T.inputs(shape)
    gt = gt.float()
    flow = torch.zeros((N - 1, H, W, 2))
    flow[..., 0] = 1.0
    out = temporal_metrics(p.cuda(), gt.cuda(), m.cuda(), flow=flow.cuda(), align="none")
    pn, gn, mn = (T.f64(t).reshape(N, H, W) for t in (p, gt, m))
    v = T.ref_valid(pn, gn, mn).reshape(N, H, W)
    for i in range(N - 1):
        ok = v[i, :, :-1] & v[i + 1, :, 1:]
        da = (pn[i + 1, :, 1:] - pn[i, :, :-1])[ok]
        dg = (gn[i + 1, :, 1:] - gn[i, :, :-1])[ok]
        r = da - dg
        terms = np.stack([np.ones_like(da), np.abs(da), da * da, np.abs(r), r * r, np.abs(dg), dg * dg, da * dg])
        want, bound = terms.sum(1), da.size * 2.0 ** -52 * np.abs(terms).sum(1)
        got = out.per_pair[i].numpy()
        assert got[0] == da.size >= H * W / 5
        assert (np.abs(got - want) <= bound).all() and bound[1] / want[1] < 1e-10, (got, want, bound)
    # and through the bilinear route of the reference
    sums = T.ref_temporal(pn.reshape(N, -1), gn.reshape(N, -1), mn.reshape(N, -1), flow.numpy(), None,
                          (np.ones(N), np.zeros(N)), 1, H, W)
    assert np.array_equal(out.per_pair.numpy()[:, 0], sums[:, 0])
    assert (rel_err(out.per_pair.numpy()[:, 1:], sums[:, 1:]) <= 1e-10).all()


# ----------------------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("kind", ["outside", "inf", "-inf", "nan"])
def test_a_flow_that_leaves_the_frame_leaves_nothing(kind):
    from rollingdepth_amd.metrics import temporal_metrics

    N, H, W, _ = shape = T.SHAPES[1]
    p, gt, m = T.inputs(shape)
    flow = torch.zeros((N - 1, H, W, 2))
    value = {"outside": float(W), "inf": math.inf, "-inf": -math.inf, "nan": math.nan}[kind]
    flow[..., 0 if kind != "nan" else 1] = value
    for target, align in ((gt.float().cuda(), "video"), (None, "none")):
        out = temporal_metrics(p.cuda(), target, m.cuda(), flow=flow.cuda(), align=align)
        assert (out.per_pair == 0).all() and out.n_valid == 0 and out.pairs_skipped == []
        assert all(math.isnan(getattr(out, k)) for k in POOLED)
    # dx = W − 1: column 0 lands on the last column, every other pixel outside
    flow[..., 0], flow[..., 1] = float(W - 1), 0.0
    out = temporal_metrics(p.cuda(), None, None, flow=flow.cuda(), align="none")
    assert out.per_pair[:, 0].tolist() == [float(H)] * (N - 1)


@pytest.mark.parametrize("k", [1, 2])
def test_a_frame_without_a_fit_zeroes_its_pairs(k):
    from rollingdepth_amd.metrics import temporal_metrics

    shape = T.SHAPES[2]
    p, gt, _ = T.inputs(shape)
    flow, m, pm = T.temporal_inputs(shape, k)
    args = dict(flow=flow.cuda(), pair_mask=pm.cuda(), frame_step=k, align="frame")
    base = temporal_metrics(p.cuda(), gt.float().cuda(), m.cuda(), **args)
    m = m.clone()
    m[2] = False  # frame 2 has no valid pixel: no fit, NaN scale and shift
    out = temporal_metrics(p.cuda(), gt.float().cuda(), m.cuda(), **args)
    touched = [i for i in range(shape[0] - k) if 2 in (i, i + k)]
    assert math.isnan(out.scale[2]) and out.pairs_skipped == touched and base.pairs_skipped == []
    for i in range(shape[0] - k):
        if i in touched:
            assert (out.per_pair[i] == 0).all()
        else:
            assert T.same_bits(out.per_pair[i], base.per_pair[i]) and out.per_pair[i, 0] > 0
    assert out.n_valid == int(sum(base.per_pair[i, 0] for i in range(shape[0] - k) if i not in touched))
    assert math.isfinite(out.flicker) and math.isfinite(out.tge)


def test_the_largest_frame_step_gives_one_pair():
    from rollingdepth_amd.metrics import temporal_metrics

    N, H, W, _ = shape = T.SHAPES[2]
    p, gt, m = T.inputs(shape)
    gt = gt.float()
    out = temporal_metrics(p.cuda(), gt.cuda(), m.cuda(), frame_step=N - 1, align="none")
    sums = T.ref_temporal(T.f64(p), T.f64(gt), m.numpy().reshape(N, -1), None, None, (np.ones(N), np.zeros(N)), N - 1,
                          H, W)
    assert out.per_pair.shape == (1, 8)
    assert_sums_match(out.per_pair.numpy(), sums, True, H * W)


# ----------------------------------------------------------------------------- 7. reproducibility
@pytest.mark.parametrize("ci", [3, 7, 15, 19], ids=lambda ci: T.TEMPORAL_IDS[ci])
def test_repeated_offset_and_lone_pairs_give_the_same_bits(ci):
    from rollingdepth_amd.metrics import temporal_metrics

    p, g, m, flow, pm, kw = T.temporal_case(ci)
    k = kw["frame_step"]
    kw = {**kw, "align": "frame"}  # a frame's own fit does not depend on the other frames: pairs can be cut out
    m8 = m.to(torch.uint8)
    a = temporal_metrics(cuda(p), cuda(g), cuda(m8), flow=cuda(flow), pair_mask=cuda(pm), **kw)
    b = temporal_metrics(cuda(p), cuda(g), cuda(m8), flow=cuda(flow), pair_mask=cuda(pm), **kw)
    assert a.n_valid > 0 and T.same_bits(a.per_pair, b.per_pair) and T.same_bits(a.scale, b.scale)

    def shifted(t):  # one element past a 16-byte boundary
        if t is None:
            return None
        buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v

    pm8 = None if pm is None else pm.to(torch.uint8)
    c = temporal_metrics(shifted(p), shifted(g), shifted(m8), flow=shifted(flow), pair_mask=shifted(pm8), **kw)
    assert T.same_bits(a.per_pair, c.per_pair) and T.same_bits(a.scale, c.scale) and T.same_bits(a.shift, c.shift)
    for i in range(p.shape[0] - k):
        two = [i, i + k]
        d = temporal_metrics(cuda(p[two]), cuda(g[two]), cuda(m8[two]), flow=cuda(flow[i:i + 1]),
                             pair_mask=None if pm is None else cuda(pm[i:i + 1]), **{**kw, "frame_step": 1})
        assert d.per_pair.shape == (1, 8) and T.same_bits(d.per_pair[0], a.per_pair[i])


# ----------------------------------------------------------------------------- 8. grid-stride loop
def test_a_frame_larger_than_the_grid():
    """H·W = 4096·256 + 8·256 + 3: 256 workgroups stride twice and a little over the octets, the last of which is short.
    align="none" keeps every term exact (see test_integer_flow_is_a_shift), so the bound is the summation's,
    n · 2⁻⁵² · Σ|terms| — n ≈ 8e5 is beyond what the relative 1e-10 was derived for."""
    from rollingdepth_amd.metrics import temporal_metrics

    W = 4096 * 256 + 8 * 256 + 3
    g = torch.Generator().manual_seed(7)
    p = torch.randint(128, 1024, (2, 1, W), generator=g) / 1024
    gt = torch.randint(256, 4096, (2, 1, W), generator=g) / 1024
    m = torch.randint(0, 8, (2, 1, W), generator=g) > 0
    out = temporal_metrics(p.cuda(), gt.cuda(), m.cuda(), align="none")
    pn, gn, mn = T.f64(p), T.f64(gt), m.numpy().reshape(2, -1)
    ok = T.ref_valid(pn, gn, mn).all(0)
    da, dg = (pn[1] - pn[0])[ok], (gn[1] - gn[0])[ok]
    r = da - dg
    terms = np.stack([np.ones_like(da), np.abs(da), da * da, np.abs(r), r * r, np.abs(dg), dg * dg, da * dg])
    want, bound = terms.sum(1), da.size * 2.0 ** -52 * np.abs(terms).sum(1)
    got = out.per_pair[0].numpy()
    assert ok[-3:].any() and got[0] == da.size > W / 2
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    sums = T.ref_temporal(pn, gn, mn, None, None, (np.ones(2), np.zeros(2)), 1, 1, W)  # the shared reference agrees
    assert sums[0, 0] == want[0] and (rel_err(sums[0], want) < 1e-12).all()
