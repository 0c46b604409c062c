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


# ----------------------------------------------------------------------------- f32 engines
NPS = [1, 2, 3]
F32_NAMES = sorted(NU.GEMM_F32_CASES)


def _cases32(pred):
    return [n for n in F32_NAMES if pred(NU.GEMM_F32_CASES[n])]


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("name", F32_NAMES)
def test_f32_emulation_inside_bound(name, np_):
    ref, bound = NU.gemm_f32_ref(name, np_)
    y = NU.gemm_emulate_f32(name, np_)
    assert y.dtype == torch.float32 and y.shape == ref.shape
    ex = NU.excess(y, ref, bound)
    print(f"{name} np={np_}: max |y - ref| / bound = {ex:.3f}")
    assert ex <= 1.0


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("name", _cases32(lambda c: c["bias"] and not c["geglu"]))
def test_f32_dropped_bias_column_outside_bound(name, np_):
    ref, bound = NU.gemm_f32_ref(name, np_)
    col = NU.GEMM_F32_CASES[name]["N"] // 2
    d = (NU.gemm_emulate_f32(name, np_, "bias").double() - ref).abs() / bound
    assert d[..., col].max().item() > 1.0
    d[..., col] = 0
    assert d.max().item() <= 1.0  # only that column is wrong


@pytest.mark.parametrize("np_", NPS)
def test_f32_geglu_dropped_bias_column_outside_bound(np_):
    """The dropped bias is that of the first gate column: output column 0 leaves the bound, no other does."""
    ref, bound = NU.gemm_f32_ref("geglu_70x512x64", np_)
    d = (NU.gemm_emulate_f32("geglu_70x512x64", np_, "bias").double() - ref).abs() / bound
    assert d[:, 0].max().item() > 1.0
    d[:, 0] = 0
    assert d.max().item() <= 1.0


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("name", _cases32(lambda c: c["silu"]))
def test_f32_omitted_silu_outside_bound(name, np_):
    ref, bound = NU.gemm_f32_ref(name, np_)
    assert NU.excess(NU.gemm_emulate_f32(name, np_, "silu"), ref, bound) > 1.0


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("name", _cases32(lambda c: c["residual"] and c["M"] > 1))
def test_f32_shifted_residual_outside_bound(name, np_):
    ref, bound = NU.gemm_f32_ref(name, np_)
    d = (NU.gemm_emulate_f32(name, np_, "residual").double() - ref).abs() / bound
    assert (d.amax(dim=-1) > 1.0).all()  # every row reads the wrong residual row


@pytest.mark.parametrize("np_", NPS)
@pytest.mark.parametrize("name", F32_NAMES)
def test_f32_leaked_k_tail_outside_bound(name, np_):
    ref, bound = NU.gemm_f32_ref(name, np_)
    assert NU.excess(NU.gemm_emulate_f32(name, np_, "ktail"), ref, bound) == float("inf")


@pytest.mark.parametrize("part", ["part1", "part2"])
@pytest.mark.parametrize("name,np_", [(n, np_) for np_, kmax in ((2, 320), (3, 72))
                                      for n in _cases32(lambda c: c["K"] <= kmax)])
def test_f32_dropped_large_product_outside_bound(name, np_, part):
    """x3 without its hi·lo or lo·hi product (every case: K ≤ 320), x6 without hi·mid or mid·hi (the cases of
    K ≤ 72; beyond, the accumulation term has grown past the product): outside the elementwise bound.  (The
    x6 small products are below it at any K: the RMS criterion holds those.)"""
    ref, bound = NU.gemm_f32_ref(name, np_)
    assert NU.excess(NU.gemm_emulate_f32(name, np_, part), ref, bound) > 1.0


@pytest.mark.parametrize("name", NU.RMS_CASES)
def test_f32_rms_criterion(name):
    """exact and x6 emulations within 3·e_seq, x6 with any small product dropped outside; x3 emulation
    within its own limit, without its hi·lo product outside."""
    ref = NU.gemm_f32_ref(name, 1)[0]
    es = NU.e_seq(name)
    e1, e3 = (NU.rel_rms(NU.gemm_emulate_f32(name, n), ref) for n in (1, 3))
    print(f"{name}: e_seq {es:.2e}, exact {e1:.2e} ({e1 / es:.2f}), x6 {e3:.2e} ({e3 / es:.2f})")
    assert e1 <= NU.rms_limit(name, 1) and e3 <= NU.rms_limit(name, 3) == NU.RMS_FACTOR * es
    for part in ("part3", "part4", "part5"):
        ed = NU.rel_rms(NU.gemm_emulate_f32(name, 3, part), ref)
        print(f"{name}: x6 without {part} {ed:.2e} ({ed / es:.2f} e_seq)")
        assert ed > NU.rms_limit(name, 3)
    e2 = NU.rel_rms(NU.gemm_emulate_f32(name, 2), ref)
    ed = NU.rel_rms(NU.gemm_emulate_f32(name, 2, "part1"), ref)
    print(f"{name}: x3 {e2:.2e}, without part1 {ed:.2e}")
    assert e2 <= NU.rms_limit(name, 2) < ed


def test_f32_bound_terms():
    """c_np·P + (m_np·K + 8)·u·S·(1.1 if silu) + u·|ref| for each engine."""
    ref = torch.tensor([0.0, 1.0, -1024.0], dtype=torch.float64)
    P = torch.tensor([0.0, 1.5, 2000.0], dtype=torch.float64)
    S = torch.tensor([0.0, 2.0, 2048.0], dtype=torch.float64)
    u = 2.0 ** -24
    for np_, c, m in ((1, 0.0, 1), (2, 2.0 ** -16, 3), (3, u, 6)):
        want = c * P + (m * 56 + 8) * u * S + u * ref.abs()
        assert torch.equal(NU.f32_bound(ref, P, S, 56, np_), want)
        assert torch.allclose(NU.f32_bound(ref, P, S, 56, np_, silu=True) - want, 0.1 * (m * 56 + 8) * u * S,
                              rtol=1e-9, atol=0)


def test_f32_conv_case_matches_conv2d():
    """conv_case_f32's padding arithmetic: symmetric, the VAE's bottom/right-only pad and the ×2 upsample
    against F.conv2d of the explicitly prepared input."""
    import torch.nn.functional as F
    for kw, prep, cv in ((dict(stride=2, pad=1), lambda x: x, dict(stride=2, padding=1)),
                         (dict(stride=2, pad=0, pad_tl=0, out_hw=(6, 5)), lambda x: F.pad(x, (0, 1, 0, 1)),
                          dict(stride=2)),
                         (dict(stride=1, pad=1, upsample=True),
                          lambda x: F.interpolate(x, scale_factor=2.0, mode="nearest"), dict(padding=1))):
        cs = NU.conv_case_f32(1, 12, 10, 8, 24, 3, seed=9, **kw)
        want = F.conv2d(prep(cs["x"].double().permute(0, 3, 1, 2)), cs["w"].double(), **cv).permute(0, 2, 3, 1)
        got = cs["ref"] - cs["bias"].double() - cs["residual"].double()
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-12, atol=1e-12)
