"""The derived GEMM / conv tolerance of tests/numerics_util.py, checked without a GPU: a plain f32
emulation of every GEMM case stays inside the bound (it is loose enough for a right kernel), and
three deliberately wrong emulations fall outside it (it is tight enough to catch a wrong one)."""
import pytest
import torch

from tests import numerics_util as NU


@pytest.mark.parametrize("name", sorted(NU.GEMM_CASES))
def test_emulation_inside_bound(name):
    ref, bound = NU.gemm_ref(name)
    y = NU.gemm_emulate(name)
    assert y.dtype == (torch.float32 if NU.GEMM_CASES[name]["out_f32"] else torch.float16)
    ex = NU.excess(y, ref, bound)
    print(f"{name}: max |y - ref| / bound = {ex:.3f}")
    assert ex <= 1.0


def _cases(pred):
    return [n for n in sorted(NU.GEMM_CASES) if pred(NU.GEMM_CASES[n])]


@pytest.mark.parametrize("name", _cases(lambda c: c["bias"]))
def test_dropped_bias_column_outside_bound(name):
    ref, bound = NU.gemm_ref(name)
    col = NU.GEMM_CASES[name]["N"] // 2
    d = (NU.gemm_emulate(name, "bias").double() - ref).abs() / bound
    assert d[..., col].max().item() > 1.0
    d[..., col] = 0
    assert d.max().item() <= 1.0  # only that column is wrong


@pytest.mark.parametrize("name", _cases(lambda c: c["silu"]))
def test_omitted_silu_outside_bound(name):
    ref, bound = NU.gemm_ref(name)
    assert NU.excess(NU.gemm_emulate(name, "silu"), ref, bound) > 1.0


@pytest.mark.parametrize("name", _cases(lambda c: c["residual"] and c["M"] > 1))
def test_shifted_residual_outside_bound(name):
    ref, bound = NU.gemm_ref(name)
    d = (NU.gemm_emulate(name, "residual").double() - ref).abs() / bound
    assert (d.amax(dim=-1) > 1.0).all()  # every row reads the wrong residual row


def test_bound_scales_with_the_operands():
    """The f16 term follows |ref|, the accumulation term S and K; NaN / inf never pass."""
    ref = torch.tensor([0.0, 1.0, -1024.0], dtype=torch.float64)
    S = torch.tensor([0.0, 2.0, 2048.0], dtype=torch.float64)
    b16 = NU.epilogue_bound(ref, S, 56, False)
    assert torch.allclose(b16, 2.0 ** -10 * ref.abs() + 64 * 2.0 ** -24 * S + 2.0 ** -24, rtol=0, atol=0)
    b32 = NU.epilogue_bound(ref, S, 56, True)
    assert torch.allclose(b32, 64 * 2.0 ** -24 * S + 2.0 ** -24 * ref.abs(), rtol=0, atol=0)
    bs = NU.epilogue_bound(ref, S, 56, False, silu=True)
    assert torch.allclose(bs - b16, 0.1 * 64 * 2.0 ** -24 * S, rtol=1e-12, atol=0)
    assert NU.excess(torch.tensor([0.0, float("nan"), -1024.0]), ref, b16 + 1) == float("inf")
