"""The bounds of tests/norm_util.py, checked without a GPU: a plain model of a right kernel (exact
statistics rounded once to f32, f32 fma apply; the two-pass f32 LayerNorm) stays inside them, and wrong
ones — f32 one-pass moments at |mean|/σ ≥ 8, another group's or image's statistics — fall outside."""
import pytest
import torch

from tests import norm_util as NO

GN_SMALL = [(40, 8, 77), (320, 32, 576), (128, 32, 7), (2560, 32, 64)]
LN_SHAPES = [(1, 40), (5, 320), (16389, 40), (70, 520), (70, 1280), (9, 2048)]


def test_ulp16():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 1000.0, 2.0 ** -14, 2.0 ** -15, 0.0, -3.0], dtype=torch.float64)
    want = torch.tensor([-10, -10, -9, -11, -1, -24, -24, -24, -9], dtype=torch.float64)
    assert torch.equal(NO.ulp16(v), torch.exp2(want))
    # agrees with the spacing of torch's own f16
    h = torch.tensor([1.0, 1000.0, 0.75, 3.0], dtype=torch.float16)
    nxt = (h.view(torch.int16) + 1).view(torch.float16)
    assert torch.equal(NO.ulp16(h.double()), (nxt.double() - h.double()))


@pytest.mark.parametrize("rho", [0, 8, 32, 64])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("C,G,HW", GN_SMALL)
def test_ideal_groupnorm_inside_bounds(C, G, HW, f16, rho):
    cs = NO.gn_case(C, G, HW, rho, f16)
    mr, y = NO.gn_emulate(cs)
    em, er = NO.stats_excess(mr, cs["m64"], cs["s64"], cs["r64"])
    ref, R = NO.gn_ref(cs)
    ey = NO.excess(y, ref, NO.gn_out_bound(ref, R, f16))
    print(f"ideal gn C={C} HW={HW} rho={rho}: mean {em:.3f} rstd {er:.3f} out {ey:.3f} of the bounds")
    assert em <= 1.0 and er <= 1.0 and ey <= 1.0


@pytest.mark.parametrize("rho", [8, 32, 64])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_f32_one_pass_moments_outside_bound(f16, rho):
    """Sequential f32 Σx, Σx² per 64-row strip, f64 only from there on: the rstd bound rejects it from
    |mean|/σ = 8 upwards, and the f32 output bound from 32."""
    cs = NO.gn_case(320, 32, 576, rho, f16)
    mr, y = NO.gn_emulate(cs, "f32")
    _, er = NO.stats_excess(mr, cs["m64"], cs["s64"], cs["r64"])
    ref, R = NO.gn_ref(cs)
    ey = NO.excess(y, ref, NO.gn_out_bound(ref, R, f16))
    print(f"f32 one-pass rho={rho}: rstd {er:.1f} out {ey:.2f} of the bounds")
    assert er > 1.0
    if rho >= 32 and not f16:
        assert ey > 1.0


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_wrong_index_outside_bounds(f16):
    """Statistics of the neighbouring group, or of the next image, are far outside every bound, at ρ = 0 too."""
    cs = NO.gn_case(40, 8, 77, 0, f16)
    ref, R = NO.gn_ref(cs)
    bound = NO.gn_out_bound(ref, R, f16)
    for dim in (0, 1):
        wrong = dict(cs, m64=torch.roll(cs["m64"], 1, dim), r64=torch.roll(cs["r64"], 1, dim))
        mr, y = NO.gn_emulate(wrong)
        em, er = NO.stats_excess(mr, cs["m64"], cs["s64"], cs["r64"])
        assert min(em, er) > 100 and NO.excess(y, ref, bound) > 100


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("M,C", LN_SHAPES)
def test_layernorm_model_inside_bound(M, C, f16):
    cs = NO.ln_case(M, C, f16)
    ex = NO.excess(NO.ln_emulate(cs), cs["ref"], cs["bound"])
    print(f"layernorm model M={M} C={C}: {ex:.3f} of the bound")
    assert ex <= 1.0


def test_head_reference_matches_torch():
    """The hand-written f64 head reference is torch's group_norm → silu → conv2d."""
    import torch.nn.functional as F

    cs = NO.head_case(2, 9, 11, 24, 8, True)
    x = cs["x"].double().permute(0, 3, 1, 2)
    n = F.group_norm(x, cs["G"], cs["gamma"].double(), cs["beta"].double(), cs["eps"])
    w = cs["w9"].double().view(3, 3, 24).permute(2, 0, 1)[None]
    for silu in (False, True):
        ref = F.conv2d(F.silu(n) if silu else n, w, padding=1) + cs["bias"]
        assert torch.allclose(ref.permute(0, 2, 3, 1), cs["refs"][silu], rtol=1e-12, atol=1e-12)
