"""The f32 GEMM / conv engines (gemm_f32.hip: exact f32-input MFMA, x3 and x6 bf16 splits) and the f32
attention kernels (attention_f32.hip) at their edges: the scalar epilogue (row lengths or pointers that are
not 4-element aligned) with bias / row bias / residual / SiLU, the ragged vector tail, operand strides
(lda > K, ldc / ldr > N, non-dense batch strides with a 3-D split weight, channel-slice conv outputs), GEGLU
with a residual and a strided output, row edges, K-tail masking against NaN poison, the general per-lane
im2col addressing at stride 2 / asymmetric padding / ×2 upsample, conv2d's f32 batch split,
RDMI_F32_SLOTS=3, and attention with Sq ≠ Sk, an explicit scale, a slice output and poisoned key tails.

GEMM and conv: each element against an f64 reference of the same f32 inputs within the derived bound of
tests/numerics_util.py (its f32 branch); f32-equivalence of exact and x6 by the relative-RMS criterion
there.  Attention: the absolute tolerances of tests/test_f32_gpu.py.  All NaN poison sits inside tensors the
tests allocate (the padding of a wider buffer)."""
import pytest
import torch

from tests import numerics_util as NU

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
F32 = torch.float32
X3_ENV = {"exact": "0", "x3": "1", "x6": "6"}
ATT_TOL = {"exact": 1e-5, "x3": 1e-4, "x6": 1e-5}  # test_f32_gpu.py: 1e-5 absolute, ATT_X3 for the bf16x3 form
CONV_ALPHA = 0.18215


def _k():
    from rollingdepth_amd import kernels as K
    return K


@pytest.fixture(params=["exact", "x3", "x6"])
def f32_engine(request, monkeypatch):
    """The product engine of Linear, conv and attention alike: RDMI_F32_X3 = 0 (exact f32-input MFMA), 1 (two-way
    bf16 split, three products) or 6 (three-way split, six products), set before any weight is packed."""
    monkeypatch.setenv("RDMI_F32_X3", X3_ENV[request.param])
    return request.param


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(y, ref, bound, what, eng):
    ex = NU.excess(y, ref, bound)
    print(f"f32-excess {eng} {what}: max |y - ref| / bound = {ex:.3f}")
    assert ex <= 1.0, what


def _pack(K_, w, eng):
    """pack_linear per batch (a 3-D weight stays 3-D: [B, N, Kp] f32, or the split layout in bf16)."""
    if w.dim() == 2:
        wp = K_.pack_linear(w, DEV, F32)
    else:
        wp = torch.stack([K_.pack_linear(wi, DEV, F32) for wi in w])
    assert wp.dtype == (F32 if eng == "exact" else torch.bfloat16)
    return wp


def _run_plain(name, eng, **kw):
    """The case on fresh dense operands."""
    K_ = _k()
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    y = K_.gemm(_dev(t["a"]), _pack(K_, t["w"], eng), c["K"], bias=_dev(t["bias"]), residual=_dev(t["residual"]),
                rowbias=_dev(t["rowbias"]), rows_per_group=c["rpg"], silu=c["silu"], **kw)
    assert y.dtype == F32
    return y


def _check_case(y, name, eng):
    _check(y, *NU.gemm_f32_ref(name, NU.F32_NP[eng]), name, eng)


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("name", ["scalar_70x130x64", "scalar_70x67x64"])
def test_f32_gemm_scalar_epilogue_by_shape(name, f32_engine):
    """ldc = ldr = rowbias_ld = N with N % 4 != 0: bias + row bias (two groups of 35 rows) + residual through
    store_tile_f32's per-element branch."""
    _check_case(_run_plain(name, f32_engine), name, f32_engine)


@pytest.mark.parametrize("name", ["silu_257x202x40", "silu_257x200x40"])
def test_f32_gemm_silu_scalar_and_ragged_vector_tail(name, f32_engine):
    """SiLU on the per-element branch (N = 202) and, at N = 200, on vector rows whose last 16-column fragment
    ends at the `n + 3 < N` test."""
    _check_case(_run_plain(name, f32_engine), name, f32_engine)


def test_f32_gemm_scalar_epilogue_by_pointer(f32_engine):
    """N = 128 with every epilogue operand one element off its vector alignment: bias = buf[1:129], residual
    and output columns 1..128 of [130, 131] tensors.  The untouched columns stay NaN."""
    K_ = _k()
    name = "ptr_130x128x64"
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    buf = torch.zeros(130, device=DEV)
    buf[1:129] = _dev(t["bias"])
    rbig = torch.full((130, 131), NAN, device=DEV)
    rbig[:, 1:129] = _dev(t["residual"])
    big = torch.full((130, 131), NAN, device=DEV)
    K_.gemm(_dev(t["a"]), _pack(K_, t["w"], f32_engine), c["K"], out=big[:, 1:129], bias=buf[1:129],
            residual=rbig[:, 1:129])
    _check_case(big[:, 1:129], name, f32_engine)
    assert torch.isnan(big[:, 0]).all() and torch.isnan(big[:, 129:]).all()


def test_f32_gemm_vector_epilogue_strided(f32_engine):
    """lda > K (a = columns 320..639 of [300, 960]), ldc / ldr > N (columns 64..383 of [300, 448]) on the
    vector path; the border of the output buffer stays NaN."""
    K_ = _k()
    name = "strided_300x320x320"
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    abig = torch.randn(300, 960, device=DEV)
    abig[:, 320:640] = _dev(t["a"])
    rbig = torch.full((300, 448), NAN, device=DEV)
    rbig[:, 64:384] = _dev(t["residual"])
    big = torch.full((300, 448), NAN, device=DEV)
    K_.gemm(abig[:, 320:640], _pack(K_, t["w"], f32_engine), c["K"], out=big[:, 64:384], residual=rbig[:, 64:384])
    _check_case(big[:, 64:384], name, f32_engine)
    assert torch.isnan(big[:, :64]).all() and torch.isnan(big[:, 384:]).all()


def test_f32_gemm_batched_nondense_strides(f32_engine):
    """B = 3 with a, out and residual the first 200 rows of [3, 207, ·] tensors (batch stride ≠ M·ld) and a
    3-D weight — on x3 / x6 the split layout, whose batch stride counts bf16 elements; rows 200..206 of the
    output buffer stay NaN."""
    K_ = _k()
    name = "batched_3x200x256x96"
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    abig = torch.randn(3, 207, 96, device=DEV)
    abig[:, :200] = _dev(t["a"])
    rbig = torch.full((3, 207, 256), NAN, device=DEV)
    rbig[:, :200] = _dev(t["residual"])
    big = torch.full((3, 207, 256), NAN, device=DEV)
    w = _pack(K_, t["w"], f32_engine)
    assert w.dim() == 3 and w.shape[-1] == 96 * {"exact": 1, "x3": 2, "x6": 4}[f32_engine]
    K_.gemm(abig[:, :200], w, c["K"], out=big[:, :200], residual=rbig[:, :200])
    _check_case(big[:, :200], name, f32_engine)
    assert torch.isnan(big[:, 200:]).all()


@pytest.mark.parametrize("name", ["rows_1x320x64", "rows_65x320x64", "rows_129x320x64", "rows_257x320x64"])
def test_f32_gemm_row_edges(name, f32_engine):
    """M = 1 and one row past a 64-row (x6) / 128-row tile, with a residual (rows past M must not be read)."""
    _check_case(_run_plain(name, f32_engine), name, f32_engine)


@pytest.mark.parametrize("name", ["ktail_70x128x8", "ktail_70x128x24", "ktail_70x128x40", "ktail_70x128x72"])
def test_f32_gemm_k_tail_poison(name, f32_engine):
    """K not a multiple of the 32-wide K-tile, with NaN right behind the valid K in every row of A
    (a = abig[:, :K] of [70, 96]) and, on the exact engine (whose weight rows end at K), of W too
    (w = wbig[:, :K] of [128, 96], ldw > K): a missing K mask turns the output NaN."""
    K_ = _k()
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    abig = torch.full((70, 96), NAN, device=DEV)
    abig[:, :c["K"]] = _dev(t["a"])
    if f32_engine == "exact":
        wbig = torch.full((128, 96), NAN, device=DEV)
        wbig[:, :c["K"]] = _dev(t["w"])
        w = wbig[:, :c["K"]]
    else:
        w = _pack(K_, t["w"], f32_engine)
    y = K_.gemm(abig[:, :c["K"]], w, c["K"])
    assert torch.isfinite(y).all()
    _check_case(y, name, f32_engine)


@pytest.mark.parametrize("strided_out", [False, True], ids=["dense", "slice_output"])
def test_f32_gemm_geglu_residual(strided_out, f32_engine):
    """GEGLU (M = 70, C = 64: N = 512 value | gate rows → 256 outputs) with a residual (the epilogue's scalar
    p.R read), into a fresh tensor and into columns 64..319 of a NaN-filled [70, 384] buffer (ldc > N / 2)."""
    K_ = _k()
    name = "geglu_70x512x64"
    c, t = NU.GEMM_F32_CASES[name], NU.gemm_f32_inputs(name)
    wq, bq = K_.geglu_permute(t["w"], t["bias"])
    big = torch.full((70, 384), NAN, device=DEV)
    out = big[:, 64:320] if strided_out else None
    y = K_.gemm(_dev(t["a"]), _pack(K_, wq, f32_engine), c["K"], out=out, bias=_dev(bq), residual=_dev(t["residual"]),
                geglu=True)
    assert y.shape == (70, 256)
    _check_case(y, name, f32_engine)
    if strided_out:
        assert torch.isnan(big[:, :64]).all() and torch.isnan(big[:, 320:]).all()


@pytest.mark.parametrize("eng", ["exact", "x3"])
def test_f32_slots3_bitwise(eng, monkeypatch):
    """RDMI_F32_SLOTS=3 (one workgroup per CU, 3-slot LDS ring) is bitwise the default 2-slot form: a dense
    GEMM with bias + residual and a 64 → 128 conv with the full epilogue.  (x6 has no 3-slot form.)"""
    K_ = _k()
    monkeypatch.setenv("RDMI_F32_X3", X3_ENV[eng])
    monkeypatch.delenv("RDMI_F32_SLOTS", raising=False)
    name = "slots_300x320x320"
    cs = NU.conv_case_f32(2, 12, 10, 64, 128, 3, 1, 1, CONV_ALPHA, rowbias=2, seed=1, image_scale=True)
    wc = K_.pack_conv(cs["w"], DEV, 64, F32)

    def run():
        return _run_plain(name, eng), K_.conv2d(_dev(cs["x"]), wc, 128, 3, bias=_dev(cs["bias"]),
                                                rowbias=_dev(cs["rowbias"]), residual=_dev(cs["residual"]),
                                                alpha=CONV_ALPHA)

    y2, c2 = run()
    monkeypatch.setenv("RDMI_F32_SLOTS", "3")
    y3, c3 = run()
    _check_case(y2, name, eng)
    _check(c2, cs["ref"], NU.conv_f32_bound(cs, NU.F32_NP[eng]), "conv 64->128 (slots)", eng)
    assert torch.equal(y3, y2) and torch.equal(c3, c2)


@pytest.mark.parametrize("name", NU.RMS_CASES)
def test_f32_gemm_rms_criterion(name, f32_engine):
    """f32-equivalence, statistically (numerics_util): the relative RMS error of a pure product at K = 64 and
    320 is ≤ 3·e_seq (the sequential f32 chain's) on exact and x6 — an x6 engine without one of its three
    small products sits 7–18 × e_seq — and ≤ 2 × the x3 emulation's on x3."""
    ref = NU.gemm_f32_ref(name, 1)[0]
    e = NU.rel_rms(_run_plain(name, f32_engine), ref)
    lim = NU.rms_limit(name, NU.F32_NP[f32_engine])
    print(f"f32-rms {f32_engine} {name}: e {e:.3e} = {e / NU.e_seq(name):.3f} e_seq, limit {lim:.3e}")
    assert e <= lim


# ----------------------------------------------------------------------------- conv
GENERAL = {  # B, H, W, stride, conv2d / conv_case_f32 keywords
    "s1_7x9": (1, 7, 9, 1, {}),                                           # M = 63: less than a tile
    "s2_13x11": (2, 13, 11, 2, {}),
    "vae_down_12x10": (2, 12, 10, 2, dict(pad_tl=0, out_hw=(6, 5))),      # F.pad(0, 1, 0, 1) + 3×3 s2
    "up_7x5": (2, 7, 5, 1, dict(upsample=True)),
}


@pytest.mark.parametrize("Cin", [8, 40])
@pytest.mark.parametrize("variant", sorted(GENERAL))
def test_f32_conv_general_addressing(variant, Cin, f32_engine):
    """Cin % 32 != 0: the per-lane (tap, channel chunk) im2col addressing of issue() at stride 1 and 2, with
    the VAE downsample's bottom/right-only padding and through the ×2 upsample (MODE 2); Cout = 24."""
    K_ = _k()
    B, H, W, stride, kw = GENERAL[variant]
    pad = 0 if "pad_tl" in kw else 1
    cs = NU.conv_case_f32(B, H, W, Cin, 24, 3, stride, pad, seed=10 + Cin, **kw)
    y = K_.conv2d(_dev(cs["x"]), K_.pack_conv(cs["w"], DEV, Cin, F32), 24, 3, stride=stride, pad=pad,
                  bias=_dev(cs["bias"]), residual=_dev(cs["residual"]), **kw)
    assert y.dtype == F32 and y.shape == cs["ref"].shape
    _check(y, cs["ref"], NU.conv_f32_bound(cs, NU.F32_NP[f32_engine]), f"conv {variant} {Cin}->24", f32_engine)


@pytest.mark.parametrize("c0", [64, 1], ids=["aligned", "misaligned"])
def test_f32_conv_epilogue_channel_slice(c0, f32_engine):
    """Fast addressing (Cin = 64), 64 → 128 at 12×10, B = 2, each image scaled differently: alpha, bias, a
    per-image row bias [B, Cout] and a residual, written into channels c0 .. c0+Cout of an NHWC buffer 128
    channels wider (the residual a like slice).  c0 = 1: the scalar epilogue.  The other channels stay NaN."""
    K_ = _k()
    B, H, W, Cin, Cout = 2, 12, 10, 64, 128
    cs = NU.conv_case_f32(B, H, W, Cin, Cout, 3, 1, 1, CONV_ALPHA, rowbias=2, seed=1, image_scale=True)
    rbig = torch.full((B, H, W, Cout + 128), NAN, device=DEV)
    rbig[..., c0:c0 + Cout] = _dev(cs["residual"])
    big = torch.full((B, H, W, Cout + 128), NAN, device=DEV)
    K_.conv2d(_dev(cs["x"]), K_.pack_conv(cs["w"], DEV, Cin, F32), Cout, 3, bias=_dev(cs["bias"]),
              rowbias=_dev(cs["rowbias"]), residual=rbig[..., c0:c0 + Cout], out=big[..., c0:c0 + Cout],
              alpha=CONV_ALPHA)
    _check(big[..., c0:c0 + Cout], cs["ref"], NU.conv_f32_bound(cs, NU.F32_NP[f32_engine]),
           f"conv 64->128 c0={c0}", f32_engine)
    assert torch.isnan(big[..., :c0]).all() and torch.isnan(big[..., c0 + Cout:]).all()


@pytest.mark.parametrize("k", [3, 1])
def test_f32_conv_cout_not_multiple_of_4(k, f32_engine):
    """Cout = 6 (ldc = ldr = 6: the scalar epilogue), Cin = 40, 12×10, bias and residual; k = 1 is the dense
    (MODE 0) form."""
    K_ = _k()
    cs = NU.conv_case_f32(1, 12, 10, 40, 6, k, 1, k // 2, seed=2)
    y = K_.conv2d(_dev(cs["x"]), K_.pack_conv(cs["w"], DEV, 40, F32), 6, k, pad=k // 2, bias=_dev(cs["bias"]),
                  residual=_dev(cs["residual"]))
    assert y.shape == (1, 12, 10, 6)
    _check(y, cs["ref"], NU.conv_f32_bound(cs, NU.F32_NP[f32_engine]), f"conv{k} 40->6", f32_engine)


def test_f32_conv_batch_split(f32_engine, monkeypatch):
    """conv2d's recursive batch split on f32: five 16×16×64 → 128 images with the threshold lowered to two
    images (5 → 2 + 3 → 1 + 1, 1 + 2 → 1 + 1), with bias, a per-image row bias and a residual.  The output is
    bitwise that of the unsplit call and inside the bound."""
    K_ = _k()
    B, H, W, Cin, Cout = 5, 16, 16, 64, 128
    cs = NU.conv_case_f32(B, H, W, Cin, Cout, 3, 1, 1, rowbias=2, seed=3, image_scale=True)
    x, w = _dev(cs["x"]), K_.pack_conv(cs["w"], DEV, Cin, F32)
    bias, rb, res = _dev(cs["bias"]), _dev(cs["rowbias"]), _dev(cs["residual"])
    calls = []
    real = K_.lib.rdmi_conv2d
    monkeypatch.setattr(K_.lib, "rdmi_conv2d", lambda a, s: (calls.append(a._obj.B), real(a, s))[1])
    y0 = K_.conv2d(x, w, Cout, 3, bias=bias, rowbias=rb, residual=res)
    assert calls == [B]
    monkeypatch.setitem(K_._SPLIT_ELEMS, F32, 2 * H * W * Cin)
    y1 = K_.conv2d(x, w, Cout, 3, bias=bias, rowbias=rb, residual=res)
    assert calls[1:] == [1] * B  # every image its own launch
    assert torch.equal(y1, y0)
    _check(y1, cs["ref"], NU.conv_f32_bound(cs, NU.F32_NP[f32_engine]), "split conv", f32_engine)


# ----------------------------------------------------------------------------- attention
def _sdpa64(q, k, v, heads, scale):
    B, Sq, HD = q.shape
    D = HD // heads
    qh = q.double().view(B, Sq, heads, D).transpose(1, 2)
    kh = k.double().view(B, -1, heads, D).transpose(1, 2)
    vh = v.double().view(B, -1, heads, D).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return (p @ vh).transpose(1, 2).reshape(B, Sq, HD)


ATT = dict(B=2, H=3, Sq=100, Sk=333, scale=0.2)
_att_cache = {}


def _att_case():
    """Seeded CPU q [B, Sq, C], k / v [B, Sk, C] and the f64 softmax(scale·q·kᵀ)·v, computed once."""
    if not _att_cache:
        g = torch.Generator().manual_seed(5000)
        C = ATT["H"] * 64
        q = torch.randn(ATT["B"], ATT["Sq"], C, generator=g)
        k = torch.randn(ATT["B"], ATT["Sk"], C, generator=g)
        v = torch.randn(ATT["B"], ATT["Sk"], C, generator=g)
        _att_cache.update(q=q, k=k, v=v, ref=_sdpa64(q, k, v, ATT["H"], ATT["scale"]))
    return _att_cache


@pytest.mark.parametrize("poison", [False, True], ids=["dense_kv", "nan_behind_keys"])
def test_f32_attention_cross_lengths_slice_output(poison, f32_engine):
    """Sq = 100 against Sk = 333 (five full 64-key tiles and a ragged one of 13), scale = 0.2, the output in
    channels 64 .. 64+C of a NaN-filled [B, Sq, C + 128] buffer whose border stays NaN.  nan_behind_keys: k
    and v are [:, :Sk] of [B, Sk + 31, C] buffers whose extra rows are NaN — the last tile's rows past Sk
    must reach neither the scores nor P·V (0 · NaN is NaN)."""
    K_ = _k()
    cs = _att_case()
    B, Sq, Sk, C = ATT["B"], ATT["Sq"], ATT["Sk"], ATT["H"] * 64
    k, v = _dev(cs["k"]), _dev(cs["v"])
    if poison:
        kbig = torch.full((B, Sk + 31, C), NAN, device=DEV)
        vbig = torch.full((B, Sk + 31, C), NAN, device=DEV)
        kbig[:, :Sk], vbig[:, :Sk] = k, v
        k, v = kbig[:, :Sk], vbig[:, :Sk]
    big = torch.full((B, Sq, C + 128), NAN, device=DEV)
    o = K_.attention(_dev(cs["q"]), k, v, ATT["H"], out=big[..., 64:64 + C], scale=ATT["scale"])
    assert o.dtype == F32 and torch.isfinite(o).all()
    err = (o.double().cpu() - cs["ref"]).abs().max().item()
    print(f"f32 attention ({f32_engine}) Sq={Sq} Sk={Sk}{' poison' if poison else ''}: max |Δ| {err:.2e}")
    assert err < ATT_TOL[f32_engine]
    assert torch.isnan(big[..., :64]).all() and torch.isnan(big[..., 64 + C:]).all()


def test_f32_attention_every_key_tile_counts(f32_engine):
    """S = 256, one head, q ≡ 0 (uniform softmax); batch t has v = 1 on the keys of tile t and 0 elsewhere, so
    every output is 64/256: a skipped or doubled key tile is off by 0.25."""
    K_ = _k()
    g = torch.Generator().manual_seed(5001)
    q = torch.zeros(4, 256, 64, device=DEV)
    k = torch.randn(4, 256, 64, generator=g).to(DEV)
    v = torch.zeros(4, 256, 64, device=DEV)
    for t in range(4):
        v[t, 64 * t:64 * t + 64] = 1.0
    o = K_.attention(q, k, v, 1)
    err = (o.double() - 0.25).abs().max().item()
    print(f"f32 attention ({f32_engine}) key tiles: max |o - 1/4| {err:.2e}")
    assert err <= 1e-6
