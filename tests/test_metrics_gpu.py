"""rollingdepth_amd.metrics on the device against a numpy f64 reference written here.

Inputs lie on a 2⁻¹⁰ grid, so f32 holds them exactly (f16 operands are rounded once, and the reference reads
the rounded values).  Bounds:
  moments   |Δ| ≤ n · 2⁻⁵² · Σ|terms|                       (f64 summation, either order; n exact)
  fit       relative 16 · n · 2⁻⁵³ · (n·Σp² / det)           (moment error × conditioning, both computed here)
  errors    n and the δ counts equal, sums relative 1e-10   (2⁻⁵³ on each a, n·2⁻⁵² on a sum, n ≤ 2e4);
            the reference asserts that no ratio lies within 1e-10 of a δ threshold before counts are compared.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7, 9, 0), (2, 33, 31, 1), (5, 64, 48, 2), (2, 96, 96, 4)]
F16, F32 = torch.float16, torch.float32
# every dtype / mask combination on the first two shapes, one on the rest
CASES = [(s, pd, td, mk) for s in SHAPES[:2] for pd in (F16, F32) for td in (F16, F32) for mk in (False, True)]
CASES += [(s, F32, F32, True) for s in SHAPES[2:]]
_DT = {F16: "f16", F32: "f32"}
CASE_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{_DT[pd]}-{_DT[td]}-{'mask' if mk else 'nomask'}" for s, pd, td, mk in CASES]
THR = (1.25, 1.25 ** 2, 1.25 ** 3)
LO = 1e-3


@functools.lru_cache(maxsize=None)
def inputs(shape):
    N, H, W, seed = shape
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(128, 1024, (N, H, W), generator=g) / 1024
    r = torch.randint(512, 2048, (N, H, W), generator=g) / 1024
    gt = ((1.5 * p + 0.25) * r).float()
    m = torch.randint(0, 4, (N, H, W), generator=g) > 0
    return p, gt, m


def f64(t):
    return t.detach().cpu().double().numpy().reshape(t.shape[0], -1)


# ----------------------------------------------------------------------------- the numpy f64 reference
def ref_valid(p, g, m, lo=LO, hi=math.inf):
    v = np.isfinite(p) & np.isfinite(g) & (g > float(np.float32(lo))) & (g < float(np.float32(hi)))
    return v if m is None else v & (m.reshape(v.shape) != 0)


def ref_moments(p, g, v):
    """[N, 6] sums and [N, 6] sums of |terms| (the scale of the summation bound)."""
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.stack([np.ones_like(p), p, g, p * p, p * g, g * g], -1)
    terms = np.where(v[..., None], terms, 0.0)
    return terms.sum(1), np.abs(terms).sum(1)


def ref_solve(mom):
    n, sp, sg, spp, spg = mom[..., 0], mom[..., 1], mom[..., 2], mom[..., 3], mom[..., 4]
    det = n * spp - sp * sp
    ok = (n >= 2) & (det > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(ok, (n * spg - sp * sg) / det, np.nan)
        t = np.where(ok, (spp * sg - sp * spg) / det, np.nan)
        cond = np.where(ok, n * spp / det, np.nan)
    return s, t, cond


def ref_fit(mom, align):
    """(s [N], t [N], conditioning [N]) of the numpy moments."""
    N = mom.shape[0]
    if align == "none":
        return np.ones(N), np.zeros(N), np.ones(N)
    if align == "video":
        s, t, c = ref_solve(mom.sum(0))
        return np.full(N, s), np.full(N, t), np.full(N, c)
    return ref_solve(mom)


def ref_errors(p, g, v, s, t, clip=None):
    """[N, 8] sums and the smallest distance of a ratio max(a/g, g/a) to a δ threshold."""
    out = np.zeros((p.shape[0], 8))
    dist = math.inf
    for f in range(p.shape[0]):
        if math.isnan(s[f]) or math.isnan(t[f]):
            continue
        pf, gf = p[f][v[f]], g[f][v[f]]
        a = s[f] * pf + t[f]
        if clip is not None:
            a = np.clip(a, clip[0], clip[1])
        d = np.abs(a - gf)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(a > 0, np.maximum(a / gf, gf / a), np.inf)
        out[f, :5] = [pf.size, d.sum(), (d / gf).sum(), (d * d).sum(), (d * d / gf).sum()]
        for k, c in enumerate(THR):
            out[f, 5 + k] = (ratio < c).sum()
            if ratio.size:
                dist = min(dist, np.abs(ratio - c).min())
    return out, dist


def ref_metrics(sums):
    tot = sums.sum(0)
    n = tot[0]
    return {"mae": tot[1] / n, "abs_rel": tot[2] / n, "rmse": math.sqrt(tot[3] / n), "sq_rel": tot[4] / n,
            "delta1": tot[5] / n, "delta2": tot[6] / n, "delta3": tot[7] / n}


@functools.lru_cache(maxsize=None)
def reference(case_idx):
    """Computed once per case and shared: operands as f64, validity, moments, and per align mode the fit
    and the error sums."""
    shape, pd, td, mk = CASES[case_idx]
    p, gt, m = inputs(shape)
    pn, gn = f64(p.to(pd)), f64(gt.to(td))
    v = ref_valid(pn, gn, m.numpy() if mk else None)
    mom, scale = ref_moments(pn, gn, v)
    ref = {"mom": mom, "mom_abs": scale}
    for align in ("video", "frame", "none"):
        s, t, cond = ref_fit(mom, align)
        sums, dist = ref_errors(pn, gn, v, s, t)
        assert dist > 1e-10, f"a test input lies {dist:.1e} from a δ threshold: counts are not comparable"
        ref[align] = (s, t, cond, sums)
    return ref


def device_case(case_idx):
    shape, pd, td, mk = CASES[case_idx]
    p, gt, m = inputs(shape)
    return p.to(pd).cuda(), gt.to(td).cuda(), (m.cuda() if mk else None)


def assert_metrics_close(a, b, tol=1e-10):
    for k in ("abs_rel", "sq_rel", "mae", "rmse", "delta1", "delta2", "delta3"):
        x, y = (a[k] if isinstance(a, dict) else getattr(a, k)), (b[k] if isinstance(b, dict) else getattr(b, k))
        assert math.isclose(x, y, rel_tol=tol, abs_tol=tol), (k, x, y)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ----------------------------------------------------------------------------- 1. moments
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_moments(ci):
    from rollingdepth_amd import kernels as K

    p, g, m = device_case(ci)
    N, P = p.shape[0], p.shape[1] * p.shape[2]
    mu8 = None if m is None else m.view(torch.uint8).view(N, P)
    ws = K.depth_moments(p.view(N, P), g.view(N, P), mu8, LO, math.inf)
    assert ws.numel() == K.lib.rdmi_depth_metrics_workspace(N, P)
    mom, _ = K.depth_fit(ws, N, P, K.DEPTH_FIT_MODES["frame"])
    mom = mom.cpu().numpy()
    ref = reference(ci)
    n = ref["mom"][:, 0]
    err, bound = np.abs(mom - ref["mom"]), n[:, None] * 2.0 ** -52 * ref["mom_abs"]
    print("moments: max |Δ| / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(mom[:, 0], n)
    assert (err <= bound).all(), (err, bound)


# ----------------------------------------------------------------------------- 2. fit
@pytest.mark.parametrize("per_frame", [False, True], ids=["video", "frame"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_fit(ci, per_frame):
    from rollingdepth_amd.metrics import align_scale_shift

    p, g, m = device_case(ci)
    s, t, mom = align_scale_shift(p, g, m, per_frame=per_frame)
    assert s.dtype == t.dtype == mom.dtype == torch.float64 and s.shape == t.shape == (p.shape[0],)
    ref = reference(ci)
    rs, rt, cond, _ = ref["frame" if per_frame else "video"]
    assert (cond > 1).all() and (cond < 100).all(), cond  # well conditioned inputs (4.7 … 6.5 measured in f32)
    n = ref["mom"][:, 0] if per_frame else np.full(p.shape[0], ref["mom"][:, 0].sum())
    tol = 16 * n * 2.0 ** -53 * cond
    es, et = np.abs(s.numpy() - rs) / np.abs(rs), np.abs(t.numpy() - rt) / np.abs(rt)
    print("fit: max rel err / tol", (es / tol).max(), (et / tol).max())
    assert (es <= tol).all() and (et <= tol).all(), (es, et, tol)


# ----------------------------------------------------------------------------- 3. errors
@pytest.mark.parametrize("align", ["video", "frame", "none"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_errors(ci, align):
    from rollingdepth_amd.metrics import depth_metrics

    p, g, m = device_case(ci)
    out = depth_metrics(p, g, m, align=align)
    _, _, _, sums = reference(ci)[align]
    got = out.per_frame.numpy()
    assert got.shape == (p.shape[0], 8) and not out.per_frame.is_cuda
    assert np.array_equal(got[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]]), (got, sums)
    rel = np.abs(got[:, 1:5] - sums[:, 1:5]) / np.abs(sums[:, 1:5])
    print("errors: max rel Δ of the sums", rel.max())
    assert (rel <= 1e-10).all(), rel
    assert out.n_valid == int(sums[:, 0].sum()) and out.frames_skipped == []
    assert_metrics_close(out, ref_metrics(sums))


# ----------------------------------------------------------------------------- 4. planted transform
@pytest.mark.parametrize("align", ["video", "frame"])
def test_planted_transform(align):
    from rollingdepth_amd.metrics import depth_metrics

    p, _, m = inputs(SHAPES[1])
    out = depth_metrics(p, 1.5 * p + 0.25, m, align=align)  # host tensors: moved to the device inside
    assert (out.scale - 1.5).abs().max() < 1e-12 and (out.shift - 0.25).abs().max() < 1e-12
    assert out.abs_rel < 1e-12 and out.delta1 == 1.0 and out.n_valid == int(m.sum())


# ----------------------------------------------------------------------------- 5. affine invariance
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_affine_invariance(shape):
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = (t.cuda() for t in inputs(shape))
    q = 2 * p + 0.5  # exact in f32
    for align in ("video", "frame"):
        a, b = depth_metrics(p, gt, m, align=align), depth_metrics(q, gt, m, align=align)
        assert_metrics_close(a, b)
        assert torch.equal(a.per_frame[:, [0, 5, 6, 7]], b.per_frame[:, [0, 5, 6, 7]])
        assert torch.allclose(a.scale, 2 * b.scale, rtol=1e-10, atol=0)
    a, b = depth_metrics(p, gt, m, align="none"), depth_metrics(q, gt, m, align="none")
    assert abs(a.abs_rel - b.abs_rel) > 1e-2 and abs(a.mae - b.mae) > 1e-2


# ----------------------------------------------------------------------------- 6. edges
def _rows_same(a, b, frames):
    return all(same_bits(a.per_frame[f], b.per_frame[f]) and same_bits(a.scale[f:f + 1], b.scale[f:f + 1])
               and same_bits(a.shift[f:f + 1], b.shift[f:f + 1]) for f in frames)


@pytest.mark.parametrize("kind", ["masked", "constant_pred"])
def test_frame_without_a_fit(kind):
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = (t.clone() for t in inputs(SHAPES[0]))
    base = depth_metrics(p, gt, m, align="frame")
    if kind == "masked":
        m[1] = False
    else:
        p[1] = 0.5  # det = n·n/4 − (n/2)² = 0 exactly
    out = depth_metrics(p, gt, m, align="frame")
    assert math.isnan(out.scale[1]) and math.isnan(out.shift[1]) and out.frames_skipped == [1]
    assert (out.per_frame[1] == 0).all() and _rows_same(out, base, (0, 2))
    assert out.n_valid == int(base.per_frame[[0, 2], 0].sum()) and math.isfinite(out.abs_rel)
    # video mode does not care: a masked frame adds exact zeros, a constant frame is fitted with the rest
    vid = depth_metrics(p, gt, m, align="video")
    assert vid.frames_skipped == [] and torch.isfinite(vid.scale).all()
    if kind == "masked":
        two = depth_metrics(p[[0, 2]], gt[[0, 2]], m[[0, 2]], align="video")
        assert same_bits(vid.per_frame[[0, 2]], two.per_frame) and same_bits(vid.scale[:2], two.scale)
        assert (vid.per_frame[1] == 0).all() and vid.abs_rel == two.abs_rel
    else:
        pn, gn = f64(p), f64(gt)
        v = ref_valid(pn, gn, m.numpy())
        s, t, _ = ref_fit(ref_moments(pn, gn, v)[0], "video")
        sums, dist = ref_errors(pn, gn, v, s, t)
        assert dist > 1e-10
        assert np.array_equal(vid.per_frame.numpy()[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]])
        assert_metrics_close(vid, ref_metrics(sums))


def test_all_frames_without_a_fit_gives_nan_metrics():
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = inputs(SHAPES[0])
    out = depth_metrics(p, gt, torch.zeros_like(m))
    assert out.n_valid == 0 and out.frames_skipped == [0, 1, 2]
    assert all(math.isnan(getattr(out, k)) for k in ("abs_rel", "sq_rel", "mae", "rmse", "delta1", "delta2", "delta3"))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_poison_is_excluded_behind_and_in_front_of_the_mask(dtype):
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = (t.clone() for t in inputs(SHAPES[1]))
    p, gt = p.to(dtype), gt.to(dtype)
    m[:, 0, :8] = True
    clean = m.clone()
    clean[:, 0, :8] = False  # the reference run: those pixels masked out, values untouched
    base = {a: depth_metrics(p, gt, clean, align=a) for a in ("video", "frame", "none")}
    nan, inf = math.nan, math.inf
    for k, (tensor, val, visible) in enumerate([(p, nan, False), (p, inf, True), (gt, nan, True), (gt, inf, False),
                                                (p, -inf, False), (gt, -inf, True), (p, nan, True), (gt, inf, True)]):
        tensor[:, 0, k] = val
        m[:, 0, k] = visible
    for a in ("video", "frame", "none"):
        out = depth_metrics(p, gt, m, align=a)
        assert same_bits(out.per_frame, base[a].per_frame) and same_bits(out.scale, base[a].scale)
        assert same_bits(out.shift, base[a].shift) and math.isfinite(out.abs_rel) and out.frames_skipped == []
    # without a mask the poisoned pixels are still excluded, all of them
    out = depth_metrics(p, gt, None)
    assert out.n_valid == p.numel() - 8 * p.shape[0] and math.isfinite(out.rmse)


def test_valid_range_and_clip():
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = inputs(SHAPES[1])
    pn, gn = f64(p), f64(gt)
    v = ref_valid(pn, gn, m.numpy(), 0.5, 2.0)
    assert 0 < v.sum() < ref_valid(pn, gn, m.numpy()).sum()  # the range does exclude targets
    for align in ("video", "frame"):
        s, t, _ = ref_fit(ref_moments(pn, gn, v)[0], align)
        for clip in (None, (0.75, 1.5)):
            sums, dist = ref_errors(pn, gn, v, s, t, clip)
            assert dist > 1e-10
            out = depth_metrics(p, gt, m, align=align, valid_range=(0.5, 2.0), clip=clip)
            assert np.array_equal(out.per_frame.numpy()[:, [0, 5, 6, 7]], sums[:, [0, 5, 6, 7]])
            assert_metrics_close(out, ref_metrics(sums))
    # the clip changed something, and it is applied to a only: targets beyond it still count in full
    assert gn[v].max() > 1.5 and gn[v].min() < 0.75
    a = depth_metrics(p, gt, m, valid_range=(0.5, 2.0))
    b = depth_metrics(p, gt, m, valid_range=(0.5, 2.0), clip=(0.75, 1.5))
    assert a.n_valid == b.n_valid and a.mae != b.mae


def test_two_valid_pixels_fit_exactly():
    from rollingdepth_amd.metrics import depth_metrics

    p = torch.tensor([[[0.25, 0.75, 0.5]]])
    gt = torch.tensor([[[1.0, 2.0, 9.0]]])
    m = torch.tensor([[[True, True, False]]])
    for align in ("video", "frame"):
        out = depth_metrics(p, gt, m, align=align)
        assert out.scale.tolist() == [2.0] and out.shift.tolist() == [0.5] and out.n_valid == 2
        assert out.mae == 0.0 and out.abs_rel == 0.0 and out.rmse == 0.0 and out.delta1 == 1.0
    one = depth_metrics(p, gt, torch.tensor([[[True, False, False]]]))
    assert one.frames_skipped == [0] and one.n_valid == 0 and math.isnan(one.abs_rel)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["odd_P", "P_multiple_of_8"])
def test_views_at_an_odd_element_offset_give_the_same_bits(shape):
    """f16 pred at 2-byte, f32 target at 4-byte and the mask at 1-byte alignment: the scalar-load path adds
    in the order of the 16-byte-load path."""
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = inputs(shape)
    p, mu8 = p.half(), m.to(torch.uint8)

    def shifted(t):
        buf = torch.zeros(t.numel() + 9, dtype=t.dtype, device="cuda")
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v

    for align in ("video", "frame", "none"):
        a = depth_metrics(p.cuda(), gt.cuda(), mu8.cuda(), align=align)
        b = depth_metrics(shifted(p), shifted(gt), shifted(mu8), align=align)
        assert same_bits(a.per_frame, b.per_frame) and same_bits(a.scale, b.scale) and same_bits(a.shift, b.shift)
        c = depth_metrics(shifted(p), gt.cuda(), None, align=align)
        d = depth_metrics(p.cuda(), shifted(gt), None, align=align)
        assert same_bits(c.per_frame, d.per_frame) and same_bits(c.scale, d.scale)


# ----------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["odd_P", "three_blocks"])
def test_determinism(shape):
    from rollingdepth_amd.metrics import align_scale_shift, depth_metrics

    p, gt, m = (t.cuda() for t in inputs(shape))
    for align in ("video", "frame"):
        a, b = depth_metrics(p, gt, m, align=align), depth_metrics(p, gt, m, align=align)
        assert same_bits(a.per_frame, b.per_frame) and same_bits(a.scale, b.scale) and same_bits(a.shift, b.shift)
    two, one = depth_metrics(p, gt, m, align="frame"), depth_metrics(p[:1], gt[:1], m[:1], align="frame")
    assert same_bits(two.per_frame[0], one.per_frame[0])
    assert same_bits(two.scale[:1], one.scale) and same_bits(two.shift[:1], one.shift)
    m2, m1 = align_scale_shift(p, gt, m, per_frame=True)[2], align_scale_shift(p[:1], gt[:1], m[:1], per_frame=True)[2]
    assert same_bits(m2[0], m1[0])


def test_shapes_and_mask_kinds_agree():
    """[N, 1, H, W] and [N, H, W], bool and uint8 masks, host and device operands: one result."""
    from rollingdepth_amd.metrics import depth_metrics

    p, gt, m = inputs(SHAPES[0])
    a = depth_metrics(p, gt, m)
    b = depth_metrics(p[:, None].cuda(), gt[:, None].cuda(), (m[:, None].to(torch.uint8) * 7).cuda())
    assert same_bits(a.per_frame, b.per_frame) and same_bits(a.scale, b.scale) and a.abs_rel == b.abs_rel


# ----------------------------------------------------------------------------- 8. arguments
def test_bad_arguments_come_back_as_the_library_error():
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K

    p, gt, m = inputs(SHAPES[0])
    p, gt, m = p.cuda().view(3, 63), gt.cuda().view(3, 63), m.cuda().view(torch.uint8).view(3, 63)
    ws = K.depth_metrics_workspace(3, 63, p.device)
    ws.fill_(-7.0)
    st = torch.ones((3, 2), dtype=torch.float64, device=p.device)
    inf = math.inf
    with pytest.raises(N_.RdmiError, match="lo < hi"):
        K.depth_moments(p, gt, m, 1.0, 1.0, ws)
    with pytest.raises(N_.RdmiError, match="lo < hi"):
        K.depth_moments(p, gt, m, math.nan, 1.0, ws)
    with pytest.raises(N_.RdmiError, match="lo < hi"):
        K.depth_errors(p, gt, m, st, 2.0, 1.0, ws=ws)
    with pytest.raises(N_.RdmiError, match="clip"):
        K.depth_errors(p, gt, m, st, LO, inf, 1.0, 0.5, ws)
    with pytest.raises(N_.RdmiError, match="mode"):
        K.depth_fit(ws, 3, 63, 3)
    with pytest.raises(N_.RdmiError, match="must be >= 1"):
        K.depth_fit(ws, 0, 63, K.DEPTH_FIT_MODES["video"])
    with pytest.raises(N_.RdmiError, match="must be >= 1"):
        K.depth_fit(ws, 3, 0, K.DEPTH_FIT_MODES["video"])
    with pytest.raises(N_.RdmiError, match="null"):
        K.depth_fit(None, 3, 63, K.DEPTH_FIT_MODES["video"], device=p.device)
    with pytest.raises(N_.RdmiError):  # N = 0
        K.depth_moments(p[:0], gt[:0], None, LO, inf, ws)
    lib, ptr = N_.lib, (p.data_ptr(), gt.data_ptr(), m.data_ptr(), ws.data_ptr(), st.data_ptr())
    sums = torch.full((3, 8), -7.0, dtype=torch.float64, device=p.device)
    sp = sums.data_ptr()
    bad = [
        lib.rdmi_depth_moments(None, 1, ptr[1], 1, ptr[2], 3, 63, LO, inf, ptr[3], None),
        lib.rdmi_depth_moments(ptr[0], 1, None, 1, ptr[2], 3, 63, LO, inf, ptr[3], None),
        lib.rdmi_depth_moments(ptr[0], 1, ptr[1], 1, ptr[2], 3, 63, LO, inf, None, None),
        lib.rdmi_depth_moments(ptr[0], 2, ptr[1], 1, ptr[2], 3, 63, LO, inf, ptr[3], None),   # u8 pred
        lib.rdmi_depth_moments(ptr[0], 1, ptr[1], 7, ptr[2], 3, 63, LO, inf, ptr[3], None),   # unknown dtype
        lib.rdmi_depth_moments(ptr[0], 1, ptr[1], 1, ptr[2], 3, 0, LO, inf, ptr[3], None),
        lib.rdmi_depth_errors(ptr[0], 1, ptr[1], 1, ptr[2], 3, 63, LO, inf, None, -inf, inf, ptr[3], sp, None),
        lib.rdmi_depth_errors(ptr[0], 1, ptr[1], 1, ptr[2], 3, 63, LO, inf, ptr[4], -inf, inf, ptr[3], None, None),
        lib.rdmi_depth_errors(ptr[0], 1, ptr[1], 4, ptr[2], 3, 63, LO, inf, ptr[4], -inf, inf, ptr[3], sp, None),
        lib.rdmi_depth_errors(ptr[0], 1, ptr[1], 1, ptr[2], -1, 63, LO, inf, ptr[4], -inf, inf, ptr[3], sp, None),
        lib.rdmi_depth_fit(ptr[3], 3, 63, 2, None, ptr[4], None),
        lib.rdmi_depth_fit(ptr[3], 3, 63, 2, sp, None, None),
    ]
    assert bad == [1001] * len(bad), bad
    with pytest.raises(N_.RdmiError):
        N_.check(bad[0], "rdmi_depth_moments")
    assert lib.rdmi_depth_metrics_workspace(0, 63) == 0 and lib.rdmi_depth_metrics_workspace(3, 0) == 0
    # nothing was launched: no output buffer was touched
    torch.cuda.synchronize()
    assert (ws == -7.0).all() and (sums == -7.0).all() and (st == 1.0).all()
    # and the wrapper's own checks
    with pytest.raises(ValueError):
        K.depth_moments(p, gt[:, :62], None, LO, inf)
    with pytest.raises(ValueError):
        K.depth_moments(p.cpu(), gt, None, LO, inf)
    with pytest.raises(TypeError):
        K.depth_moments(p, gt, m.bool(), LO, inf)
    with pytest.raises(TypeError):
        K.depth_moments(p.double(), gt, None, LO, inf)
    with pytest.raises(ValueError):
        K.depth_moments(p, gt, None, LO, inf, ws[:1])
