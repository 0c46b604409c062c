"""CPU anchors of tests/aligner_util.py: the workspace-layout mirror against csrc/aligner_ws.h, and the
one-iteration restatement against the loss's definition (torch.autograd in f64) and against the oracle —
so that tests/test_aligner_step_gpu.py compares the kernels with something tied to the definition, not to
the kernels."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import rd_oracle as O
from tests import aligner_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUPLES = [(7, 7, 8, 1, 1), (7, 9001, 8, 2, 1), (11, 5929, 8, 2, 0), (14, 9, 20, 20, 1), (100, 5929, 148, 2000, 1),
          (40, 10404, 1024, 129, 1), (3, 1, 1, 0, 0), (7, 2500, 10, 128, 1)]


def test_layout_mirror_total_vs_library():
    """ws_layout's total is rdmi_aligner_workspace's (host-only, no device needed)."""
    from rollingdepth_amd import _native

    hist_buf = (C.c_float * 4)()
    for N, P, ntot, iters, hist in TUPLES:
        a = _native.AlignerArgs()
        split = [ntot - ntot // 2, ntot // 2] if ntot > 1 else [ntot]
        a.n_dil, a.seq_len, a.P, a.iters = len(split), N, P, iters
        for d, n in enumerate(split):
            a.n[d], a.stride[d], a.w[d] = n, 1 + d, 3
        a.history = C.addressof(hist_buf) if hist else None
        assert _native.lib.rdmi_aligner_workspace(C.byref(a)) == U.ws_layout(N, P, ntot, iters, bool(hist))["total"]


def test_layout_mirror_offsets_vs_header(tmp_path):
    """Every offset of the mirror equals what a stand-alone program including csrc/aligner_ws.h prints (built
    with AddressSanitizer + UBSan, runtimes linked statically, like aligner_ws_check.cpp)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/aligner_ws_print.cpp"
    exe = str(tmp_path / "aligner_ws_print")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "aligner_ws_print.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + [str(v) for tup in TUPLES for v in tup], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(TUPLES)
    for tup, line in zip(TUPLES, lines):
        head, vals = line.split(":")
        assert tuple(int(v) for v in head.split()) == tup
        L = U.ws_layout(*tup[:4], bool(tup[4]))
        assert [int(v) for v in vals.split()] == [L[k] for k in U.LAYOUT_FIELDS], tup


def _torch_loss(case, s, t, weights):
    """The loss from its definition in torch f64: dilation d's slot j is scattered into row d·w_d + j of
    [Σw, N, P] tensors M, M_d = 1/clamp(A, 1e-3) and B (an assignment: a later dilation overwrites), T = ΣM/ΣB
    per frame, detached like its L1 scales mean|T|; loss_scale·(mean|M − T·B|/sc + depth_w·mean|M_d − T_d·B|/sc_d)
    over the full tensors + Σ_d λ2·mean(relu(1 − s_d)²) + λ3·mean(t_d²)."""
    W = U._w32(weights)
    R, N, P = sum(case.lengths), case.N, case.P
    M = torch.zeros(R, N, P, dtype=torch.float64)
    Md = torch.zeros(R, N, P, dtype=torch.float64)
    B = torch.zeros(R, N, 1, dtype=torch.float64)
    for d, (x, ix) in enumerate(zip(case.xs, case.idx)):
        A = torch.from_numpy(x.astype(np.float64)) * s[d][:, None, None] + t[d][:, None, None]
        Ad = 1.0 / torch.clamp(A, min=float(U.CLIP))
        for j in range(ix.shape[1]):
            r = d * ix.shape[1] + j
            f = torch.from_numpy(ix[:, j])
            M[r, f] = A[:, j]
            Md[r, f] = Ad[:, j]
            B[r, f] = 1.0
    with torch.no_grad():
        T = M.sum(0) / B.sum(0)
        Td = Md.sum(0) / B.sum(0)
        sc = T.abs().mean(-1, keepdim=True)
        scd = Td.abs().mean(-1, keepdim=True)
    loss = float(W.ls) * (((M - T * B) / sc).abs().mean() + float(W.dw) * ((Md - Td * B) / scd).abs().mean())
    for d in range(len(s)):
        loss = loss + float(W.l2) * (torch.relu(1.0 - s[d]) ** 2).mean() + float(W.l3) * (t[d] ** 2).mean()
    return loss


@pytest.mark.parametrize("geometry,wname", U.CASES)
def test_f64_gradient_equals_autograd(geometry, wname):
    """The f64 restatement's loss and full gradient against torch.autograd of the loss written from its
    definition, at the case's random state.  Both are f64 sums of the same ≤ 3·P·n terms in different orders:
    the gradients agree within n·2⁻⁵³ ≤ 3e-12 (n ≤ 27 003 terms per parameter) of Σ|terms|·loss_scale/numel +
    |soft term| per parameter (observed ≤ 4e-16; one term of wrong sign would be 2/n ≈ 7e-5 of it), the loss
    within 1e-12 relative."""
    case, weights = U.get_case(geometry), U.WEIGHT_SETS[wname]
    s = [torch.from_numpy(v.astype(np.float64)).requires_grad_() for v in case.s]
    t = [torch.from_numpy(v.astype(np.float64)).requires_grad_() for v in case.t]
    loss = _torch_loss(case, s, t, weights)
    loss.backward()
    ref = np.concatenate([v.grad.numpy() for v in s + t])
    m, v = U.zero_moments(case)
    r = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, weights, np.float64)
    W = U._w32(weights)
    mag = np.concatenate([r.abs_partials["gs"].sum(-1), r.abs_partials["gt"].sum(-1)]) * float(W.ls) / r.denom
    err = np.abs(r.grad - ref)
    print(f"{geometry}/{wname}: max |Δgrad| / magnitude {np.max(err / (mag + np.abs(r.grad_soft))):.2e}, "
          f"loss {float(r.loss):.6f} vs {float(loss.detach()):.6f}")
    assert np.all(err <= 3e-12 * (mag + np.abs(r.grad_soft)))
    assert abs(float(r.loss) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))


CHAIN3 = ["P36", "mixed2500", "strided5929"]


@pytest.mark.parametrize("geometry", list(U.GEOMETRIES))
def test_f32_mode_reproduces_oracle(geometry):
    """From s = 1, t = 0 with the default weights the f32 mode is the oracle's first iteration (every geometry),
    and chained with its own m, v its first three (CHAIN3).  T (history columns 1, 2) is the same arithmetic:
    exact.  The oracle sums its gradients and scales in f32 (numpy's pairwise sums) where the restatement, like
    the kernels, sums in f64: its gradient is off by at most δ = 24·2⁻²⁴·(Σ|terms|·loss_scale/numel + |soft term|)
    (elementwise f32 products, ≤ 15 levels of pairwise sums of ≤ 27 003 terms, scales an ulp apart).  m̂ is a
    convex combination of gradients and √v̂ a weighted 2-norm of them, so both move by ≤ δ, and the step
    lr·m̂/√v̂ by ≤ lr·δ/√v̂·(1 + |m̂|/√v̂); the update's own roundings add an ulp of the parameter.  Per parameter
    the tolerance is the sum of both over the iterations — for t ≈ ±1e-3 it is 4e-9 … 1.5e-7 over these cases
    (largest where a gradient nearly cancels), not an ulp of 1; the observed differences use ≤ 5 % of it.  The loss (f64 from f32 terms on both sides, scales 1 ulp apart) within 1e-6 relative.

    That argument needs every branch decided alike on both sides.  The first step from t = 0 moves every t to
    ±lr = ±1e-3 up to its last bit, and the min-shifted data holds one pixel x = 0, whose A = t then sits ON the
    clip threshold 1e-3: a last-bit difference of t switches that pixel's −1/clip² = −1e6 term.  P2056 does so
    (its second step differs from the oracle's by 1.7e-5 in that one t, every other parameter by ≤ 5e-9), which is
    why the chain is asserted on CHAIN3 only."""
    case = U.get_case(geometry)
    s = [np.ones_like(v) for v in case.s]
    t = [np.zeros_like(v) for v in case.t]
    m, v = U.zero_moments(case)
    for iters in (1, 3) if geometry in CHAIN3 else (1,):
        rs, rt, rh = O.aligner_optimize(case.xs, case.idx, case.N, iters=iters)
        cs, ct, cm, cv, hist = s, t, m, v, []
        tol, delta = np.zeros(2 * case.ntot), np.zeros(2 * case.ntot)
        for step in range(1, iters + 1):
            r = U.one_iteration(case.xs, case.idx, case.N, cs, ct, cm, cv, step, U.DEFAULT_WEIGHTS, np.float32)
            cs, ct, cm, cv = r.s, r.t, r.m, r.v
            hist.append(r.hist)
            mag = np.concatenate([r.abs_partials["gs"].sum(-1), r.abs_partials["gt"].sum(-1)]) / r.denom
            delta = np.maximum(delta, 24 * U.U32 * (mag + np.abs(r.grad_soft)))
            bc1, bc2 = U.bias_corrections(U.DEFAULT_WEIGHTS, step)
            mh, vh = np.abs(r.m.astype(np.float64)) / bc1, np.sqrt(r.v.astype(np.float64) / bc2)
            pn = np.concatenate(cs + ct)
            tol += 2 * np.spacing(np.abs(pn)).astype(np.float64) + 1e-3 * delta / vh * (1 + mh / vh)
        err = np.abs(np.concatenate(cs + ct).astype(np.float64) - np.concatenate(list(rs) + list(rt)))
        print(f"{geometry} iters {iters}: max |Δp|/tolerance {np.max(err / tol):.3f}, tolerance of t up to "
              f"{tol[case.ntot:].max():.1e}")
        assert np.all(err <= tol)
        h, rh = np.array(hist, np.float64), np.array(rh, np.float64)
        np.testing.assert_allclose(h[:, 0], rh[:, 0], rtol=1e-6)
        assert np.array_equal(h[0, 1:], rh[0, 1:])
        np.testing.assert_allclose(h[:, 1:], rh[:, 1:], rtol=0, atol=2.4e-7 * iters)


@pytest.mark.parametrize("geometry", list(U.GEOMETRIES))
def test_cases_cover_what_they_claim(geometry):
    """Each case's start state has both signs of 1 − s, between 1 % and 50 % of the values A below the clip,
    and a frame covered by at least 4 slots.  A frame covered by exactly one slot exists in the start-step
    geometry (frame 1: only snippet 0 of dilation 1); with dilations (1, 2), length 3 and N = 7 every frame
    has at least two, so over the set of cases the cover counts 1, 2, 3, ≥ 4 all occur.  The pixel counts put
    pixels on every path of the loops: an empty chunk at P = 7, one pixel in unroll lane 1 at 2056 (chunks of 257),
    two full lanes and a partial one at 5929 (741), a second round with a tail at 9001 (1125 / 1126)."""
    case = U.get_case(geometry)
    sflat = np.concatenate(case.s)
    assert (sflat < 1).any() and (sflat > 1).any()
    m, v = U.zero_moments(case)
    r = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, U.DEFAULT_WEIGHTS, np.float32)
    below = np.concatenate([(a[al] < U.CLIP).ravel() for a, al in zip(r.A, r.alive)])
    assert 0.01 <= below.mean() <= 0.5, below.mean()
    assert r.cnt.max() >= 4 and r.cnt.min() >= 1
    if geometry == "strided5929":
        assert r.cnt[1] == 1 and [ix.shape[0] for ix in case.idx] == [5, 3]
    if geometry == "mixed2500":
        assert not r.alive[0].all() and r.alive[1].all()  # the overwrite rule is in play
    assert case.N <= 11 and case.ntot <= 10
    sizes = np.diff(U.chunk_bounds(case.P))
    expect = {"P7": 0, "P8": 1, "P2056": 257, "P5929": 741, "P9001": 1125}
    if geometry in expect:
        assert sizes.min() == expect[geometry]
    if geometry == "P9001":
        assert sizes.max() == 1126


def test_cover_count_one_occurs():
    assert any((U.cover_count(U.get_case(g).idx, U.get_case(g).N) == 1).any() for g in U.GEOMETRIES)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("geometry,wname", U.CASES)
def test_f32_restatement_within_rounding_bounds_of_f64(geometry, wname, fused):
    """The bounds the GPU test holds the kernels to (aligner_util.rounding_bounds) hold for the f32
    restatement itself: T, Td per pixel, the gradient per parameter and the loss against the f64 run of the
    same inputs; at most 0.1 % of a case's terms are undecidable.  fused: the kernels' arithmetic (A as one fma),
    held on every pixel to (c + 3)·2⁻²⁴·Σ|a|/c; mul then add to the wider Σ(|x·s| + |t|) form, and to the tight
    one where no covering t is negative."""
    case, weights = U.get_case(geometry), U.WEIGHT_SETS[wname]
    m, v = U.zero_moments(case)
    r64 = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, weights, np.float64)
    r32 = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, weights, np.float32, fused=fused)
    b = U.rounding_bounds(case.xs, case.idx, case.N, case.s, case.t, weights, r64)
    assert b.undecidable <= 1e-3, b.undecidable
    eT = np.abs(r32.T.astype(np.float64) - r64.T)
    eTd = np.abs(r32.Td.astype(np.float64) - r64.Td)
    assert np.all(eT <= b.T) and np.all(eTd <= b.Td)
    if fused:
        assert np.all(eT <= b.T_tight)
    assert np.all(eT[b.T_nocancel] <= b.T_tight[b.T_nocancel])
    eg = np.abs(r32.grad.astype(np.float64) - r64.grad)
    print(f"{geometry}/{wname}: undecidable {b.undecidable:.2e}, max |ΔT|/bound {np.max(eT / (b.T_tight if fused else b.T)):.3f}, "
          f"|ΔTd|/bound {np.max(eTd / b.Td):.3f}, |Δgrad|/bound {np.max(eg / b.grad):.3f}, "
          f"|Δloss|/bound {abs(float(r32.hist[0]) - float(r64.loss)) / b.loss:.3f}")
    assert np.all(eg <= b.grad)
    assert abs(float(r32.hist[0]) - float(r64.loss)) <= b.loss


def test_fma32_is_the_correctly_rounded_fma():
    """aligner_util.fma32 against exact rational arithmetic: for every triple the result is the f32 nearest to
    a·b + c (half of the triples with c ≈ −a·b, where the product's low bits decide), and it is not what mul
    then add gives on all of them."""
    from fractions import Fraction

    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    c[:2048] = -(a * b)[:2048] + np.float32(1e-6) * c[:2048]
    f = U.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(f[i], np.float32(-np.inf)), np.nextafter(f[i], np.float32(np.inf))
        d = abs(Fraction(float(f[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i
    assert (f != a * b + c).any()


@pytest.mark.parametrize("geometry", list(U.GEOMETRIES))
def test_single_rounding_of_a(geometry):
    """The kernels form A = x·s + t as one fma (aligner.hip, mulrn); the restatement's fused=True models that
    with an exact fma.  Against mul then add (the oracle's arithmetic) every A is within the product's rounding
    plus 1 ulp of A, and T, Td within aligner_util.single_rounding_bounds — not within 1 ulp of T or Td: over these
    cases T differs by up to 8 ulp and Td by up to 220 ulp (terms that cancel; 1/max(A, 1e-3) near the clip), in
    18 – 29 % of the pixels.  With
    the weight set whose lerp weight is < 0.5, Adam's m differs in a few parameters (m + lw·diff as one fma)."""
    case = U.get_case(geometry)
    m, v = U.zero_moments(case)
    r2 = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, U.WEIGHT_SETS["other"], np.float32)
    rf = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, U.WEIGHT_SETS["other"], np.float32,
                         fused=True)
    b = U.single_rounding_bounds(case.xs, case.idx, case.N, case.s, r2)
    for x, y, dl in zip(rf.A, r2.A, b.delta):
        assert np.all(np.abs(x.astype(np.float64) - y) <= dl)
    eT, eTd = np.abs(rf.T.astype(np.float64) - r2.T), np.abs(rf.Td.astype(np.float64) - r2.Td)
    print(f"{geometry}: T differs in {np.mean(rf.T != r2.T):.1%} of the pixels, by up to "
          f"{np.max(eT / np.spacing(np.abs(r2.T))):.0f} ulp; Td by up to {np.max(eTd / np.spacing(np.abs(r2.Td))):.0f} ulp")
    assert np.all(eT <= b.T) and np.all(eTd <= b.Td)


def _owned(P, c, mutant=None):
    """The pixels one workgroup of frame_stats / snippet_grad visits for chunk c, in the kernels' loop
    structure (256 threads, UP = 4 lanes 256 apart, rounds of 1024), with one deliberate off-by-one:
    'lane_le': the lane guard px < p1 as px <= p1; 'loop_le': the round guard pb < p1 as pb <= p1;
    'lo_plus': chunk_lo one pixel high for 0 < c < PS.  Out-of-frame pixels are dropped."""
    def lo(c):
        return P * c // U.PS + (1 if mutant == "lo_plus" and 0 < c < U.PS else 0)

    p0, p1 = lo(c), lo(c + 1)
    out = []
    for tid in range(256):
        pb = p0 + tid
        while pb < p1 or (mutant == "loop_le" and pb == p1):
            for u in range(4):
                px = pb + 256 * u
                ok = px <= p1 if mutant == "lane_le" and u > 0 else (px < p1 or u == 0)
                if ok and px < P:
                    out.append(px)
            pb += 1024
    return out


def test_off_by_one_would_be_caught_beyond_36_pixels():
    """By reasoning on the loop structure, nothing run on a device: the unmutated loops visit every pixel of
    a frame exactly once at every case's P.  An off-by-one in a guard makes a workgroup visit pixel p1 of the
    next chunk as well — |T[p1]| more in that chunk's Σ|T| and one term more in its gs / gt / l1 / l2
    partials; `caught` computes both sums over the mutated pixel sets from the case's restatement and applies
    the tolerances of test_fpart (n·2⁻⁵²) and test_partials (4·2⁻²⁴) of the GPU file.  Where each mutation shows: the lane guard (lanes u ≥ 1 only, lane 0 is under the
    round guard) only where a chunk ends inside a lane u ≥ 1 — 2056 (257 = 256 + 1) and 5929 (741), not 36 or
    below, and not 9001, whose chunks (1125 = 1024 + 101) end in lane 0 of the second round; the round guard
    where a chunk ends in lane 0 — 9001, and 36 — not at 2056 or 5929; chunk_lo itself at every P, 36 included.
    So the lane guard is invisible to every comparison at P ≤ 36 and each P ≥ 2056 sees one of the guards."""
    for g in U.GEOMETRIES.values():
        P = g["P"]
        seen = sorted(px for c in range(U.PS) for px in _owned(P, c))
        assert seen == list(range(P))

    def caught(geometry, mutant):
        """Whether test_fpart's and test_partials' tolerances reject what the mutated workgroups would sum:
        frame 0's Σ|T| per chunk against n·2⁻⁵²·Σ|T|, snippet 0 slot 0's gs terms per chunk against
        4·2⁻²⁴·Σ|terms|, both from the case's restatement."""
        case = U.get_case(geometry)
        m, v = U.zero_moments(case)
        r = U.one_iteration(case.xs, case.idx, case.N, case.s, case.t, m, v, 1, U.DEFAULT_WEIGHTS, np.float32, fused=True)
        aT = np.abs(r.T[0].astype(np.float64))
        gs = r.terms[0]["gs"][0, 0]
        b = U.chunk_bounds(case.P)
        fp = pt = False
        for c in range(U.PS):
            own = np.array(_owned(case.P, c, mutant), np.int64)
            n = max(b[c + 1] - b[c], 1)
            ref = aT[b[c]:b[c + 1]].sum()
            fp |= bool(abs(aT[own].sum() - ref) > n * 2.0 ** -52 * ref)
            pt |= bool(abs(gs[own].sum() - gs[b[c]:b[c + 1]].sum()) > 4 * U.U32 * np.abs(gs[b[c]:b[c + 1]]).sum())
        return fp, pt

    geos = ("P7", "P8", "P36", "P2056", "P5929", "P9001")
    for g in geos:
        assert caught(g, None) == (False, False)
    assert [caught(g, "lane_le") for g in geos] == [(x, x) for x in (False, False, False, True, True, False)]
    assert [caught(g, "loop_le") for g in geos[2:]] == [(x, x) for x in (True, False, False, True)]
    assert all(caught(g, "lo_plus") == (True, True) for g in ("P36", "P2056", "P9001"))
