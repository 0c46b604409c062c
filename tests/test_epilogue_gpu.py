"""The f16 GEMM / conv engines' scalar epilogue (p.vec == false: row lengths or pointers that are not
4-element aligned), their SiLU epilogue, operand strides (lda > K, ldc / ldr > N, non-dense batch
strides, channel-slice conv outputs), f32 output with bias / row bias, K-tail masking against NaN
poison, and conv2d's f16 batch split — each element against an f64 reference of the same f16-rounded
inputs within the derived bound of tests/numerics_util.py (the split: bitwise the unsplit call)."""
import pytest
import torch

from tests import numerics_util as NU
from tests.test_kernels_gpu import engine, h32  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _k():
    from rollingdepth_amd import kernels as K
    return K


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(y, ref, bound, what):
    ex = NU.excess(y, ref, bound)
    print(f"{what}: max |y - ref| / bound = {ex:.3f}")
    assert ex <= 1.0, what


def _pack(K_, w):
    """pack_linear per batch (a 3-D weight stays 3-D: [B, N, Kp])."""
    if w.dim() == 2:
        return K_.pack_linear(w.float(), DEV)
    return torch.stack([K_.pack_linear(wi.float(), DEV) for wi in w])


def _run_plain(name, **kw):
    """The case on fresh dense operands."""
    K_ = _k()
    c, t = NU.GEMM_CASES[name], NU.gemm_inputs(name)
    return K_.gemm(_dev(t["a"]), _pack(K_, t["w"]), c["K"], bias=_dev(t["bias"]), residual=_dev(t["residual"]),
                   rowbias=_dev(t["rowbias"]), rows_per_group=c["rpg"], silu=c["silu"], out_f32=c["out_f32"], **kw)


@pytest.mark.parametrize("name", ["silu_3x1280x320", "silu_130x320x1280", "silu_257x200x40", "silu_257x202x40"])
def test_gemm_silu(name, engine):
    """RDMI_EPI_SILU on every f16 engine: whole vector tiles, the `n + 3 < N` remainder (N = 200) and the
    per-element branch (N = 202) against silu(a @ wᵀ + b) in f64."""
    y = _run_plain(name)
    assert y.dtype == torch.float16
    _check(y, *NU.gemm_ref(name), name)


@pytest.mark.parametrize("name", ["scalar_70x130x64_f16", "scalar_70x130x64_f32", "scalar_70x67x64_f16",
                                  "scalar_70x67x64_f32"])
def test_gemm_scalar_epilogue_by_shape(name, engine):
    """ldc = ldr = rowbias_ld = N with N % 4 != 0: bias + row bias (two groups of 35 rows) + f16 residual
    through the per-element branch, f16 and f32 output."""
    y = _run_plain(name)
    assert y.dtype == (torch.float32 if NU.GEMM_CASES[name]["out_f32"] else torch.float16)
    _check(y, *NU.gemm_ref(name), name)


def test_gemm_scalar_epilogue_by_pointer(engine):
    """N = 128 with every epilogue operand one element off its vector alignment: bias = buf[1:129],
    residual and output columns 1..128 of [130, 131] tensors.  The untouched columns stay NaN."""
    K_ = _k()
    name = "ptr_130x128x64"
    c, t = NU.GEMM_CASES[name], NU.gemm_inputs(name)
    buf = torch.zeros(130, device=DEV)
    buf[1:129] = _dev(t["bias"])
    rbig = torch.full((130, 131), NAN, dtype=torch.float16, device=DEV)
    rbig[:, 1:129] = _dev(t["residual"])
    big = torch.full((130, 131), NAN, dtype=torch.float16, device=DEV)
    K_.gemm(_dev(t["a"]), _pack(K_, t["w"]), c["K"], out=big[:, 1:129], bias=buf[1:129], residual=rbig[:, 1:129])
    _check(big[:, 1:129], *NU.gemm_ref(name), name)
    assert torch.isnan(big[:, 0]).all() and torch.isnan(big[:, 129:]).all()


def test_gemm_vector_epilogue_strided(engine):
    """lda > K (a = columns 320..639 of [300, 960]), ldc / ldr > N (columns 64..383 of [300, 448]) on the
    vector path; the border of the output buffer stays NaN."""
    K_ = _k()
    name = "strided_300x320x320"
    c, t = NU.GEMM_CASES[name], NU.gemm_inputs(name)
    abig = torch.randn(300, 960, device=DEV).half()
    abig[:, 320:640] = _dev(t["a"])
    rbig = torch.full((300, 448), NAN, dtype=torch.float16, device=DEV)
    rbig[:, 64:384] = _dev(t["residual"])
    big = torch.full((300, 448), NAN, dtype=torch.float16, device=DEV)
    K_.gemm(abig[:, 320:640], _pack(K_, t["w"]), c["K"], out=big[:, 64:384], residual=rbig[:, 64:384])
    _check(big[:, 64:384], *NU.gemm_ref(name), name)
    assert torch.isnan(big[:, :64]).all() and torch.isnan(big[:, 384:]).all()


def test_gemm_batched_nondense_strides(engine):
    """B = 3 with a, out and residual the first 200 rows of [3, 207, ·] tensors (batch stride ≠ M·ld) and
    a 3-D weight; rows 200..206 of the output buffer stay NaN."""
    K_ = _k()
    name = "batched_3x200x256x96"
    c, t = NU.GEMM_CASES[name], NU.gemm_inputs(name)
    abig = torch.randn(3, 207, 96, device=DEV).half()
    abig[:, :200] = _dev(t["a"])
    rbig = torch.full((3, 207, 256), NAN, dtype=torch.float16, device=DEV)
    rbig[:, :200] = _dev(t["residual"])
    big = torch.full((3, 207, 256), NAN, dtype=torch.float16, device=DEV)
    w = _pack(K_, t["w"])
    assert w.dim() == 3
    K_.gemm(abig[:, :200], w, c["K"], out=big[:, :200], residual=rbig[:, :200])
    _check(big[:, :200], *NU.gemm_ref(name), name)
    assert torch.isnan(big[:, 200:]).all()


@pytest.mark.parametrize("name", ["f32_2x960x1280", "f32_400x256x96"])
def test_gemm_f32_output_bias_rowbias(name, engine):
    """out_f32 with a bias (the time-embedding projection: M = 2) or a row bias (four groups of 100)."""
    y = _run_plain(name)
    assert y.dtype == torch.float32
    _check(y, *NU.gemm_ref(name), name)


@pytest.mark.parametrize("name", ["rows_1x320x64", "rows_129x320x64", "rows_257x320x64"])
def test_gemm_row_edges(name, engine):
    """M = 1 and one row past a 128- / 256-row tile, with a residual (rows past M must not be read)."""
    _check(_run_plain(name), *NU.gemm_ref(name), name)


@pytest.mark.parametrize("name", ["ktail_70x128x8", "ktail_70x128x24", "ktail_70x128x72"])
def test_gemm_k_tail_poison(name, engine):
    """K not a multiple of the 64-wide K-tile, with NaN right behind the valid K in every row of A
    (a = abig[:, :K] of [70, 96]): a missing K mask turns the output NaN."""
    K_ = _k()
    c, t = NU.GEMM_CASES[name], NU.gemm_inputs(name)
    abig = torch.full((70, 96), NAN, dtype=torch.float16, device=DEV)
    abig[:, :c["K"]] = _dev(t["a"])
    y = K_.gemm(abig[:, :c["K"]], _pack(K_, t["w"]), c["K"])
    assert torch.isfinite(y).all()
    _check(y, *NU.gemm_ref(name), name)


def test_gemm_gn_without_moments(engine):
    """gn=True at N = 130: no moments can be emitted (they need vector rows), so none are attached —
    the values are those of the plain call."""
    K_ = _k()
    name = "gn_64x130x64"
    y = _run_plain(name, gn=True)
    assert getattr(y, K_._GN_ATTR) is None
    _check(y, *NU.gemm_ref(name), name)


# ----------------------------------------------------------------------------- conv epilogues
ALPHA = 0.18215
CONV_SHAPES = [(1, 16, 16, 64, 128, 1), (1, 12, 10, 64, 64, 1), (2, 12, 12, 128, 128, 2)]  # halo-eligible; not; stride 2


@pytest.mark.parametrize("c0", [64, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", CONV_SHAPES)
def test_conv3x3_channel_slice_output(B, H, W, Cin, Cout, stride, c0, engine, h32):
    """3×3 conv writing channels c0 .. c0+Cout of an NHWC buffer 128 channels wider (y_ld > Cout), the
    residual a like slice (res_ld > Cout), alpha and bias.  c0 = 1: output and residual pointers 2 B off
    the vector alignment — the scalar epilogue, on the halo engines with the 16-B channel permutation
    off.  The other channels of the buffer stay NaN."""
    K_ = _k()
    cs = NU.conv_case(B, H, W, Cin, Cout, 3, stride, 1, ALPHA)
    Ho, Wo = cs["ref"].shape[1:3]
    rbig = torch.full((B, Ho, Wo, Cout + 128), NAN, dtype=torch.float16, device=DEV)
    rbig[..., c0:c0 + Cout] = _dev(cs["residual"])
    big = torch.full((B, Ho, Wo, Cout + 128), NAN, dtype=torch.float16, device=DEV)
    K_.conv2d(_dev(cs["x"]), K_.pack_conv(cs["w"], DEV), Cout, 3, stride=stride, pad=1, bias=_dev(cs["bias"]),
              residual=rbig[..., c0:c0 + Cout], out=big[..., c0:c0 + Cout], alpha=ALPHA)
    _check(big[..., c0:c0 + Cout], cs["ref"], cs["bound"], f"conv {B}x{H}x{W} {Cin}->{Cout} s{stride} c0={c0}")
    assert torch.isnan(big[..., :c0]).all() and torch.isnan(big[..., c0 + Cout:]).all()


@pytest.mark.parametrize("k", [3, 1])
def test_conv_cout_not_multiple_of_4(k, engine, h32):
    """Cout = 6 (ldc = ldr = 6: the scalar epilogue), Cin = 40, 12×10, bias and residual."""
    K_ = _k()
    cs = NU.conv_case(1, 12, 10, 40, 6, k, 1, k // 2, 1.0, seed=1)
    y = K_.conv2d(_dev(cs["x"]), K_.pack_conv(cs["w"], DEV), 6, k, pad=k // 2, bias=_dev(cs["bias"]),
                  residual=_dev(cs["residual"]))
    assert y.shape == (1, 12, 10, 6)
    _check(y, cs["ref"], cs["bound"], f"conv{k} 40->6")


@pytest.mark.parametrize("rowbias", [2, 1], ids=["rowbias_per_image", "rowbias_1d"])
def test_conv2d_batch_split_f16(rowbias, engine, h32, monkeypatch):
    """conv2d's recursive batch split on f16: five 16×16×64 → 128 images with the threshold lowered to two
    images (5 → 2 + 3 → 1 + 1, 1 + 2 → 1 + 1), with bias, row bias, residual, GroupNorm moments of the
    output (carved slots) and — on the halo engines — a fused input GroupNorm + SiLU (sliced statistics).
    Output and moments are bitwise those of the unsplit call; the values are inside the bound."""
    K_ = _k()
    B, H, W, Cin, Cout = 5, 16, 16, 64, 128
    cs = NU.conv_case(B, H, W, Cin, Cout, 3, 1, 1, 1.0, rowbias=rowbias, seed=2)
    g = torch.Generator().manual_seed(77)
    gm = (1 + 0.2 * torch.randn(Cin, generator=g)).to(DEV)
    bt = (0.2 * torch.randn(Cin, generator=g)).to(DEV)
    w, bias, rb, res = K_.pack_conv(cs["w"], DEV), _dev(cs["bias"]), _dev(cs["rowbias"]), _dev(cs["residual"])
    # per-image scale and offset: a wrong image's statistics or row bias would show
    sc = torch.arange(1, B + 1, device=DEV).view(B, 1, 1, 1) * 0.6
    x = (_dev(cs["x"]).float() * sc + sc).half()
    fused = engine not in ("classic", "pingpong")  # input GroupNorm runs on the halo engines only
    if fused:
        kw = dict(in_gn=(K_.groupnorm_stats(x, 32, 1e-6), gm, bt, 32, True))
    else:
        x = K_.groupnorm(x, gm, bt, 32, 1e-6, True)
        kw = {}

    def run():
        y = K_.conv2d(x, w, Cout, 3, bias=bias, rowbias=rb, residual=res, gn=True, **kw)
        assert getattr(y, K_._GN_ATTR) is not None
        return y, K_.groupnorm_stats(y, 32, 1e-6)

    calls = []
    real = K_.lib.rdmi_conv2d
    monkeypatch.setattr(K_.lib, "rdmi_conv2d", lambda a, s: (calls.append(a._obj.B), real(a, s))[1])
    y0, mr0 = run()
    assert calls == [B]
    monkeypatch.setitem(K_._SPLIT_ELEMS, torch.float16, 2 * H * W * Cin)
    y1, mr1 = run()
    assert calls[1:] == [1] * B  # every image its own launch
    assert torch.equal(y1, y0) and torch.equal(mr1, mr0)
    # the moments the split wrote are those of the output it wrote
    assert torch.allclose(mr1, K_.groupnorm_stats(y1.clone(), 32, 1e-6), rtol=1e-5, atol=1e-6)
    # values: the conv of the normalised input the kernel saw (f16, as the unfused pair feeds it)
    h = (K_.groupnorm(x, gm, bt, 32, 1e-6, True) if fused else x).cpu()
    hd, wd = h.double().permute(0, 3, 1, 2), cs["w"].double()
    rbd = cs["rowbias"].double() if rowbias == 1 else cs["rowbias"].double()[:, None, None, :]
    conv = torch.nn.functional.conv2d
    ref = conv(hd, wd, padding=1).permute(0, 2, 3, 1) + cs["bias"].double() + rbd + cs["residual"].double()
    S = conv(hd.abs(), wd.abs(), padding=1).permute(0, 2, 3, 1) + cs["bias"].double().abs() + rbd.abs() + \
        cs["residual"].double().abs()
    _check(y1, ref, NU.epilogue_bound(ref, S, 9 * Cin, False), f"split conv {engine}")
