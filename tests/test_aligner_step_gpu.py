"""One DepthAligner iteration on the device, stage by stage, against tests/aligner_util.py.

The three-launch loop (RDMI_ALIGNER_FUSED=0) leaves every intermediate of its last iteration in the workspace
kernels.aligner_optimize returns (csrc/aligner_ws.h): T, Td, the chunk partials of frame_stats and
snippet_grad, Adam's moments and the bias corrections.  Each stage is compared given the device's own
previous stage, so no sign or clip decision can differ between the two sides, at pixel counts where a
workgroup's loops take every path (tests/test_aligner_step_cpu.py::test_cases_cover_what_they_claim), for
three weight sets, from a random state, at Adam steps 1 (zero moments) and 2 (the state read after step 1).
The restatement itself is tied to the loss's definition on the CPU (tests/test_aligner_step_cpu.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import aligner_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = pytest.mark.parametrize("geometry,wname", U.CASES)
STEPS = pytest.mark.parametrize("step", [1, 2])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _runs(geometry, wname):
    """The device results of a case, computed once: iters = 1 and iters = 2 from the same start state, in the
    three-launch loop (fused False: intermediates readable) and in the default two-launch loop."""
    from rollingdepth_amd import kernels as K

    case, w = U.get_case(geometry), dict(U.DEFAULT_WEIGHTS, **U.WEIGHT_SETS[wname])
    xs = [torch.from_numpy(x).to(DEV) for x in case.xs]
    ss = case.start_steps if max(case.start_steps) > 1 else None
    out = {}
    for iters in (1, 2):
        for fused in (False, True):
            s = [torch.from_numpy(v.copy()).to(DEV) for v in case.s]
            t = [torch.from_numpy(v.copy()).to(DEV) for v in case.t]
            hist = torch.zeros((iters, 3), dtype=torch.float32, device=DEV)
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("RDMI_ALIGNER_FUSED", "1" if fused else "0")
                ws = K.aligner_optimize(xs, s, t, case.dilations, case.N, w["lr"], w["betas"], w["eps"], w["lmda2"],
                                        w["lmda3"], w["depth_w"], w["loss_scale"], iters, hist, start_steps=ss)
                torch.cuda.synchronize()
            out[iters, fused] = SimpleNamespace(
                w=U.read_workspace(ws.cpu().numpy(), case.N, case.P, case.ntot, iters, True),
                s=[v.cpu().numpy() for v in s], t=[v.cpu().numpy() for v in t], hist=hist.cpu().numpy())
    return out


def _state(geometry, wname, step):
    """(s, t, m, v) before iteration `step`: the start state, or what the iters = 1 call left."""
    case = U.get_case(geometry)
    if step == 1:
        return (case.s, case.t) + U.zero_moments(case)
    r = _runs(geometry, wname)[1, False]
    return r.s, r.t, r.w.m, r.w.v


def _restate(geometry, wname, step, dt=np.float32, fused=True, **given):
    """The restatement from the state before `step`; in f32 with the kernels' two fused multiply-adds unless
    fused=False (mul then add, the oracle's arithmetic)."""
    case = U.get_case(geometry)
    s, t, m, v = _state(geometry, wname, step)
    return U.one_iteration(case.xs, case.idx, case.N, s, t, m, v, step, U.WEIGHT_SETS[wname], dt,
                           fused=dt is np.float32 and fused, **given)


@CASES
@STEPS
def test_frame_means(geometry, wname, step):
    """T and Td are bitwise the f32 restatement's: A = fma(x, s, t) — the optimiser rounds x·s + t once
    (aligner.hip, mulrn) —, max, 1/·, the running sums in row order and the division by (float)count are single
    IEEE operations on both sides.  Against mul then add (the reference's and the oracle's two roundings) each A is
    within the product's rounding plus 1 ulp of A (tests/test_aligner_step_cpu.py::test_single_rounding_of_a); for
    T and Td that gives aligner_util.single_rounding_bounds, asserted here.  It is not 1 ulp of T or Td: sums of
    terms that cancel and 1/max(A, 1e-3) do not keep an ulp (the exact-fma restatement itself lies up to 8 and 220
    ulp from the two-rounding one over these cases).

    Against the f64 reference of the same state, with u = 2⁻²⁴ and every rounding at most u times the magnitude
    of its own result: T carries at most c + 3 roundings per pixel (the fma — one rounding, relative to |a| —, c
    running-sum adds, the division: c + 2), every rounded quantity at most Σ_i|a_i| over the c covering slots, so
    |ΔT| ≤ (c + 3)·u·Σ_i|a_i|/c on every pixel.  Td = Σ 1/max(a_i, 1e-3) / c:
    |Δ(1/ac)| ≤ (1/ac)·(u·(|x·s| + |a|)/ac + u), the sum and the division add (c + 1)·u·Σ 1/ac_i, all ÷ c
    (aligner_util.rounding_bounds; ×1.05 for second-order terms)."""
    case = U.get_case(geometry)
    dev = _runs(geometry, wname)[step, False].w
    r32 = _restate(geometry, wname, step)
    assert np.array_equal(_bits(dev.T), _bits(r32.T_own)), int((_bits(dev.T) != _bits(r32.T_own)).sum())
    assert np.array_equal(_bits(dev.Td), _bits(r32.Td_own)), int((_bits(dev.Td) != _bits(r32.Td_own)).sum())
    r2 = _restate(geometry, wname, step, fused=False)
    b2 = U.single_rounding_bounds(case.xs, case.idx, case.N, _state(geometry, wname, step)[0], r2)
    e2T, e2Td = np.abs(dev.T.astype(np.float64) - r2.T_own), np.abs(dev.Td.astype(np.float64) - r2.Td_own)
    assert np.all(e2T <= b2.T) and np.all(e2Td <= b2.Td)
    r64 = _restate(geometry, wname, step, np.float64)
    s, t, _, _ = _state(geometry, wname, step)
    b = U.rounding_bounds(case.xs, case.idx, case.N, s, t, U.WEIGHT_SETS[wname], r64)
    eT, eTd = np.abs(dev.T - r64.T), np.abs(dev.Td - r64.Td)
    print(f"max |ΔT|/bound {np.max(eT / b.T_tight):.3f}, |ΔTd|/bound {np.max(eTd / b.Td):.3f}")
    assert np.all(eT <= b.T_tight) and np.all(eTd <= b.Td)


@CASES
@STEPS
def test_fpart(geometry, wname, step):
    """frame_stats' chunk partials against numpy on the device's own T, Td over [P·c//8, P·(c + 1)//8): the f64
    sums of |T|, |Td| within n·2⁻⁵²·Σ|·| (n pixels, any order of n f64 additions of exact f32 values), min and
    max exact; an empty chunk (P = 7) gives 0, 0, +inf, −inf."""
    case = U.get_case(geometry)
    dev = _runs(geometry, wname)[step, False].w
    ref = U.fpart_of(dev.T, dev.Td)
    n = np.maximum(np.diff(U.chunk_bounds(case.P)), 1)[None, :]
    for k in (0, 1):
        assert np.all(np.abs(dev.fpart[..., k] - ref[..., k]) <= n * 2.0 ** -52 * ref[..., k])
    assert np.array_equal(dev.fpart[..., 2:], ref[..., 2:])
    if case.P == 7:
        assert np.array_equal(dev.fpart[:, 0], np.tile([0.0, 0.0, np.inf, -np.inf], (case.N, 1)))


@CASES
@STEPS
def test_partials(geometry, wname, step):
    """snippet_grad's gs, gt, l1, l2 per (snippet, chunk) against the f32 restatement evaluated on the device's
    T, Td and on scales rebuilt from the device's fpart in chunk order: every sign and the clip mask are decided
    on identical numbers, the terms are f64 products and sums of identical f32 values.  Tolerance 4·2⁻²⁴·Σ|terms|
    of the chunk; a single missing or doubled pixel is ≥ 1/(3·1 300) of Σ|terms|, three orders larger."""
    dev = _runs(geometry, wname)[step, False].w
    r = _restate(geometry, wname, step, T=dev.T, Td=dev.Td, fpart=dev.fpart)
    worst = 0.0
    for k in ("gs", "gt", "l1", "l2"):
        err = np.abs(getattr(dev, k) - r.partials_own[k])
        tol = 4 * U.U32 * r.abs_partials[k]
        worst = max(worst, float(np.max(err / np.maximum(r.abs_partials[k], 1e-300))))
        assert np.all(err <= tol), k
    print(f"largest |Δpartial| / Σ|terms|: {worst:.2e} (allowed {4 * U.U32:.2e})")


@CASES
@STEPS
def test_adam(geometry, wname, step):
    """From the device's partials and the device's bias corrections the f32 restatement of adam_param gives m, v,
    s, t bitwise — at step 1 from zero moments and at step 2 from the moments step 1 left, with both branches of
    the lerp over the weight sets (the weight < 0.5 branch m + lw·(g − m) is one fma in the kernel and in the
    restatement; everything else is one IEEE operation per operator).  The bias corrections are 1 − βⁱ within 4 ulp of f64 (pow is not correctly
    rounded on either side)."""
    case = U.get_case(geometry)
    run = _runs(geometry, wname)[step, False]
    dev = run.w
    for i in range(step + 1):
        ref = np.array(U.bias_corrections(U.WEIGHT_SETS[wname], i))
        assert np.all(np.abs(dev.bct[i] - ref) <= 4 * np.spacing(np.maximum(ref, 2.0 ** -1022))), (i, dev.bct[i], ref)
    r = _restate(geometry, wname, step, T=dev.T, Td=dev.Td, fpart=dev.fpart, partials=(dev.gs, dev.gt, dev.l1, dev.l2),
                 bct=dev.bct[step])
    assert np.array_equal(_bits(dev.m), _bits(r.m)) and np.array_equal(_bits(dev.v), _bits(r.v))
    for d in range(len(case.xs)):
        assert np.array_equal(_bits(run.s[d]), _bits(r.s[d])), d
        assert np.array_equal(_bits(run.t[d]), _bits(r.t[d])), d
    lw = np.float32(1) - np.float32(dict(U.DEFAULT_WEIGHTS, **U.WEIGHT_SETS[wname])["betas"][0])
    assert (lw < 0.5) == (wname == "other")


@CASES
@STEPS
def test_history_row(geometry, wname, step):
    """Column 0 is within 1 ulp of f32 of loss_scale·(Σl1 + depth_w·Σl2)/numel + the soft terms, evaluated in f64
    on the device's partials and the parameters before the update; columns 1 and 2 are the min and max of the
    device's T exactly.  The iters = 2 call's first row is the iters = 1 call's."""
    runs = _runs(geometry, wname)
    run = runs[step, False]
    dev = run.w
    r = _restate(geometry, wname, step, T=dev.T, Td=dev.Td, fpart=dev.fpart, partials=(dev.gs, dev.gt, dev.l1, dev.l2))
    row = run.hist[step - 1]
    assert abs(float(row[0]) - float(r.loss)) <= np.spacing(np.float32(r.loss))
    assert row[1] == dev.T.min() and row[2] == dev.T.max()
    assert np.array_equal(_bits(runs[2, False].hist[0]), _bits(runs[1, False].hist[0]))


@CASES
def test_whole_iteration_vs_f64(geometry, wname):
    """The first iteration against pure f64 from the inputs alone: with zero initial moments m = (1 − β1)·g, so
    the device's gradient is m / (1 − β1); it and the loss lie within the rounding count of
    aligner_util.rounding_bounds (per term the relative error of its factors; an undecidable term — sign(z),
    sign(zd) or the clip mask within the two sides' rounding of a tie — counted as flipped), and at most 0.1 % of
    the case's terms are undecidable."""
    case, weights = U.get_case(geometry), U.WEIGHT_SETS[wname]
    run = _runs(geometry, wname)[1, False]
    r64 = _restate(geometry, wname, 1, np.float64)
    b = U.rounding_bounds(case.xs, case.idx, case.N, case.s, case.t, weights, r64)
    assert b.undecidable <= 1e-3
    lw = float(np.float32(1) - U._w32(weights).b1)
    g = run.w.m.astype(np.float64) / lw
    eg = np.abs(g - r64.grad)
    el = abs(float(run.hist[0, 0]) - float(r64.loss))
    print(f"undecidable {b.undecidable:.2e}, max |Δgrad|/bound {np.max(eg / b.grad):.3f}, |Δloss|/bound {el / b.loss:.3f}")
    assert np.all(eg <= b.grad)
    assert el <= b.loss


@CASES
def test_two_launch_loop_bitwise(geometry, wname):
    """The default two-launch loop gives s, t, history, m and v bitwise the three-launch loop's, after one and
    after two iterations."""
    runs = _runs(geometry, wname)
    for iters in (1, 2):
        a, b = runs[iters, True], runs[iters, False]
        for x, y in zip(a.s + a.t + [a.hist, a.w.m, a.w.v], b.s + b.t + [b.hist, b.w.m, b.w.v]):
            assert np.array_equal(_bits(x), _bits(y)), iters


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("shape,border,factor", [
    ((2, 3, 37, 41), 2, 10),    # 33 and 37 are no multiples of 10: the last sample is the rounded-up one
    ((2, 2, 9, 7), 0, 1),       # every pixel
    ((3, 3, 500, 500), 0, 1),   # 2 250 000 outputs > 8 192·256: the grid-stride cap
])
def test_aligner_prepare(dtype, shape, border, factor):
    """aligner_prepare is exactly numpy's crop and strided slice of x − shift: one f32 subtraction for f32
    snippets; for f16 snippets (f16)((f32)x − shift), rounded once, widened to f32."""
    from rollingdepth_amd import kernels as K

    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, shape).astype(dtype)
    shift = np.float32(-0.37)
    H, W = shape[2:]
    sub = x[:, :, border:H - border, border:W - border][..., ::factor, ::factor].astype(np.float32) - shift
    ref = sub if dtype is np.float32 else sub.astype(np.float16).astype(np.float32)
    out = K.aligner_prepare(torch.from_numpy(x).to(DEV), torch.tensor([shift], dtype=torch.float32, device=DEV),
                            border, factor)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (shape[0], shape[1], ref.shape[2] * ref.shape[3])
    assert np.array_equal(_bits(out.cpu().numpy().reshape(ref.shape)), _bits(ref))
