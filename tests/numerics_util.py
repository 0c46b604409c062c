"""Elementwise, derived tolerance for the f16 GEMM / conv epilogue tests, the GEMM case table they
share with the CPU test of the tolerance itself, and the f64 references (computed once per case on
the CPU and cached: every engine of a parametrised test compares against the same tensor).

Bound per output element, against an f64 reference built from the same f16-rounded inputs:

    f16 output: |y − ref| ≤ 2⁻¹⁰·|ref| + (K + 8)·2⁻²⁴·S + 2⁻²⁴
    f32 output: |y − ref| ≤ (K + 8)·2⁻²⁴·S + 2⁻²⁴·|ref|

with S = |alpha|·(|a| @ |w|ᵀ) + |bias| + |rowbias| + |residual| and K the reduction length.
2⁻¹⁰ is twice the half-ulp of the one f16 rounding (one ulp of slack for the fast exp2 / rcp of the
SiLU); (K + 8)·2⁻²⁴·S is the worst case of an f32 sum of K exact products plus the epilogue's adds;
2⁻²⁴ covers the f16 subnormal spacing.  With SiLU the bound is applied after the activation and the
accumulation term grows by |silu′| ≤ 1.1.  Nothing here is tuned to a kernel's output.

The f32 engines (gemm_f32.hip: exact f32-input MFMA, x3 two-way and x6 three-way bf16 split; np = 1, 2, 3)
have their own branch below (GEMM_F32_CASES, gemm_f32_ref, gemm_emulate_f32, conv_case_f32).  Inputs are
f32 and not f16-rounded, so the low parts of the splits carry data; the reference is f64 of the same f32
values.  With P = |alpha|·(|a| @ |w|ᵀ), S = P + |bias| + |rowbias| + |residual|, u = 2⁻²⁴:

    |y − ref| ≤ c_np·P + (m_np·K + 8)·u·S·(1.1 if silu) + u·|ref|,  c = {0, 2⁻¹⁶, 2⁻²⁴},  m = {1, 3, 6}

  * bf16 round-to-nearest-even leaves ≤ 2⁻⁹ relative; split_bf16x2 / split3_bf16x2 (common.h) and
    split_bf16 / split3_bf16 (kernels.py) are RNE at every step, each remainder exact in f32.
  * Two parts leave ≤ 2⁻¹⁸|x| per operand (two operands: 2·2⁻¹⁸, plus their product 2⁻³⁶), and the dropped
    lo·lo term is ≤ 2⁻¹⁸|a||w|: together < 2⁻¹⁶|a||w|, summed over K: c₂·P.
  * Three parts leave ≤ 2⁻²⁷|x| per operand; the three dropped products (mid·lo, lo·mid, lo·lo) are
    ≤ 2·2⁻²⁷ + 2⁻³⁶: together < 2⁻²⁴|a||w|: c₃·P.
  * m counts the f32 accumulations per K position (the kept products), each rounding ≤ u of a partial sum
    that S bounds; + 8 for the epilogue's multiply and adds.
GEGLU (out = h·gelu(g) + R, h and g two columns of the same GEMM with errors e_h, e_g inside the bound above,
|gelu′| ≤ 1.13, |gelu(g)| ≤ |g|, erff and the 1 + erf cancellation ≤ 8u·|g| absolute):
    |y − ref| ≤ |gelu(g)|·e_h + 1.13·(|h| + e_h)·e_g + 8u·|h|·|g| + 2u·(|h·gelu(g)| + |R|).

A worst-case elementwise bound cannot see an x6 engine that drops one of its three small products (≈ 2⁻¹⁸
per product, under the accumulation term).  f32-equivalence is therefore held statistically: the relative RMS
error e(y) = rms(y − ref) / rms(ref) of a pure product (no epilogue, unit-variance a, w ~ N(0, 1/K)) against
e_seq, the same product as a strictly sequential f32 chain y += a[:, k]·w[:, k] on the CPU.  exact and x6:
e ≤ 3·e_seq at K = 64 and 320 (CPU: e_seq 1.5e-7 / 3.3e-7, the right x6 emulation 0.8e-7 / 1.4e-7, one small
product dropped 2.4–2.8e-6; at K = 1280 e_seq has grown past the defect, so no long K here); x3:
e ≤ 2·e(x3 emulation)."""
import functools
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


def epilogue_bound(ref: torch.Tensor, S: torch.Tensor, K: int, out_f32: bool, silu: bool = False) -> torch.Tensor:
    acc = (K + 8) * U24 * S.double() * (1.1 if silu else 1.0)
    if out_f32:
        return acc + U24 * ref.abs()
    return 2.0 ** -10 * ref.abs() + acc + U24


def excess(y: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over the elements of |y − ref| / bound (≤ 1: inside the bound); NaN / inf in y → inf."""
    y = y.detach().double().cpu()
    if not torch.isfinite(y).all():
        return float("inf")
    return ((y - ref).abs() / bound).max().item()


# ----------------------------------------------------------------------------- GEMM case table
def _c(M, N, K, bias=False, rpg=0, residual=False, silu=False, out_f32=False, batch=1):
    return dict(M=M, N=N, K=K, bias=bias, rpg=rpg, residual=residual, silu=silu, out_f32=out_f32, batch=batch)


GEMM_CASES = {
    # SiLU epilogue (the time-embedding MLP's shapes, a ragged vector tail, a scalar-only N)
    "silu_3x1280x320": _c(3, 1280, 320, bias=True, silu=True),
    "silu_130x320x1280": _c(130, 320, 1280, bias=True, silu=True),
    "silu_257x200x40": _c(257, 200, 40, bias=True, silu=True),
    "silu_257x202x40": _c(257, 202, 40, bias=True, silu=True),
    # scalar epilogue by shape (ldc % 4 != 0)
    "scalar_70x130x64_f16": _c(70, 130, 64, bias=True, rpg=35, residual=True),
    "scalar_70x130x64_f32": _c(70, 130, 64, bias=True, rpg=35, residual=True, out_f32=True),
    "scalar_70x67x64_f16": _c(70, 67, 64, bias=True, rpg=35, residual=True),
    "scalar_70x67x64_f32": _c(70, 67, 64, bias=True, rpg=35, residual=True, out_f32=True),
    # scalar epilogue by pointer only
    "ptr_130x128x64": _c(130, 128, 64, bias=True, residual=True),
    # vector epilogue with operand strides
    "strided_300x320x320": _c(300, 320, 320, residual=True),
    "batched_3x200x256x96": _c(200, 256, 96, residual=True, batch=3),
    # f32 output with bias / row bias
    "f32_2x960x1280": _c(2, 960, 1280, bias=True, out_f32=True),
    "f32_400x256x96": _c(400, 256, 96, rpg=100, out_f32=True),
    # row edges
    "rows_1x320x64": _c(1, 320, 64, residual=True),
    "rows_129x320x64": _c(129, 320, 64, residual=True),
    "rows_257x320x64": _c(257, 320, 64, residual=True),
    # K tail (the GPU test follows the valid K with NaN)
    "ktail_70x128x8": _c(70, 128, 8),
    "ktail_70x128x24": _c(70, 128, 24),
    "ktail_70x128x72": _c(70, 128, 72),
    # gn=True at an N without moments
    "gn_64x130x64": _c(64, 130, 64, bias=True),
}


@functools.lru_cache(maxsize=None)
def gemm_inputs(name: str) -> dict:
    """Seeded CPU inputs of a case, f16-rounded where the kernel reads f16: a [B?, M, K] f16,
    w [B?, N, K] f16 (3-D when batched), bias [N] f32, rowbias [⌈M/rpg⌉, N] f32, residual [B?, M, N] f16."""
    c = GEMM_CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(GEMM_CASES).index(name))
    lead = (c["batch"],) if c["batch"] > 1 else ()
    t = {"a": torch.randn(*lead, c["M"], c["K"], generator=g).half(),
         "w": (torch.randn(*lead, c["N"], c["K"], generator=g) / math.sqrt(c["K"])).half()}
    t["bias"] = torch.randn(c["N"], generator=g) if c["bias"] else None
    t["rowbias"] = torch.randn(-(-c["M"] // c["rpg"]), c["N"], generator=g) if c["rpg"] else None
    t["residual"] = torch.randn(*lead, c["M"], c["N"], generator=g).half() if c["residual"] else None
    return t


def _gemm_terms(name: str, dtype, drop_bias_col=None, shift_residual=False):
    """(a @ wᵀ, the epilogue's addend) in `dtype`, optionally with a deliberately wrong epilogue."""
    c, t = GEMM_CASES[name], gemm_inputs(name)
    prod = torch.matmul(t["a"].to(dtype), t["w"].to(dtype).transpose(-1, -2))
    add = torch.zeros_like(prod)
    if t["bias"] is not None:
        b = t["bias"].to(dtype).clone()
        if drop_bias_col is not None:
            b[drop_bias_col] = 0
        add = add + b
    if t["rowbias"] is not None:
        add = add + t["rowbias"].to(dtype).repeat_interleave(c["rpg"], 0)[:c["M"]]
    if t["residual"] is not None:
        r = t["residual"].to(dtype)
        add = add + (torch.roll(r, 1, dims=-2) if shift_residual else r)
    return prod, add


@functools.lru_cache(maxsize=None)
def gemm_ref(name: str):
    """(f64 reference, its bound) of a case."""
    c, t = GEMM_CASES[name], gemm_inputs(name)
    prod, add = _gemm_terms(name, torch.float64)
    ref = prod + add
    if c["silu"]:
        ref = F.silu(ref)
    S = torch.matmul(t["a"].double().abs(), t["w"].double().abs().transpose(-1, -2))
    for k in ("bias", "rowbias", "residual"):
        if t[k] is not None:
            v = t[k].double().abs()
            S = S + (v.repeat_interleave(c["rpg"], 0)[:c["M"]] if k == "rowbias" else v)
    return ref, epilogue_bound(ref, S, c["K"], c["out_f32"], c["silu"])


def gemm_emulate(name: str, wrong: str = "") -> torch.Tensor:
    """Plain emulation of the kernel: f32 matmul on the f16-rounded inputs, epilogue in f32, one
    rounding to the output dtype.  wrong: "bias" (bias of one column dropped), "silu" (activation
    omitted) or "residual" (residual rows shifted by one)."""
    c = GEMM_CASES[name]
    prod, add = _gemm_terms(name, torch.float32, drop_bias_col=c["N"] // 2 if wrong == "bias" else None,
                            shift_residual=wrong == "residual")
    y = prod + add
    if c["silu"] and wrong != "silu":
        y = F.silu(y)
    return y if c["out_f32"] else y.half()


# ----------------------------------------------------------------------------- conv reference
@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, Cin, Cout, k, stride, pad, alpha, rowbias=0, seed=0):
    """Seeded CPU inputs of a conv (x NHWC f16, w [Cout, Cin, k, k] f16-rounded f32, bias f32, residual
    NHWC f16, rowbias: 0 none, 1 per channel [Cout], 2 per image [B, Cout]) with the f64 reference
    alpha·conv(x, w) + bias (+ rowbias) + residual (NHWC) and its bound."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(B, H, W, Cin, generator=g).half()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).half().float()
    bias = torch.randn(Cout, generator=g)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    prod = F.conv2d(xd, wd, stride=stride, padding=pad).permute(0, 2, 3, 1)
    S = abs(alpha) * F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    res = torch.randn(prod.shape, generator=g).half()
    ref = alpha * prod + bias.double() + res.double()
    S = S + bias.double().abs() + res.double().abs()
    rb = None
    if rowbias:
        rb = torch.randn((Cout,) if rowbias == 1 else (B, Cout), generator=g)
        rbd = rb.double() if rowbias == 1 else rb.double()[:, None, None, :]
        ref, S = ref + rbd, S + rbd.abs()
    return dict(x=x, w=w, bias=bias, residual=res, rowbias=rb, ref=ref,
                bound=epilogue_bound(ref, S, k * k * Cin, False))


# ============================================================================= f32 engines
BF16 = torch.bfloat16
F32_NP = {"exact": 1, "x3": 2, "x6": 3}
F32_C = {1: 0.0, 2: 2.0 ** -16, 3: 2.0 ** -24}
F32_M = {1: 1, 2: 3, 3: 6}
# the kept products as (weight part, activation part) in the kernel's order (gemm_f32.hip: the X3 MFMA
# triple, wpart / apart of X6)
F32_PRODUCTS = {1: ((0, 0),), 2: ((0, 0), (1, 0), (0, 1)), 3: ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))}
RMS_FACTOR = 3.0     # exact / x6: e ≤ RMS_FACTOR · e_seq
RMS_FACTOR_X3 = 2.0  # x3: e ≤ RMS_FACTOR_X3 · e(x3 emulation)


def f32_bound(ref, P, S, K: int, np_: int, silu: bool = False) -> torch.Tensor:
    return F32_C[np_] * P + (F32_M[np_] * K + 8) * U24 * S * (1.1 if silu else 1.0) + U24 * ref.abs()


def _c32(M, N, K, bias=False, rpg=0, residual=False, silu=False, batch=1, geglu=False):
    return dict(M=M, N=N, K=K, bias=bias, rpg=rpg, residual=residual, silu=silu, batch=batch, geglu=geglu)


GEMM_F32_CASES = {
    # scalar epilogue by shape (ldc % 4 != 0), with SiLU (N = 202), and the ragged vector tail (N = 200)
    "scalar_70x130x64": _c32(70, 130, 64, bias=True, rpg=35, residual=True),
    "scalar_70x67x64": _c32(70, 67, 64, bias=True, rpg=35, residual=True),
    "silu_257x202x40": _c32(257, 202, 40, bias=True, silu=True),
    "silu_257x200x40": _c32(257, 200, 40, bias=True, silu=True),
    # scalar epilogue by pointer only
    "ptr_130x128x64": _c32(130, 128, 64, bias=True, residual=True),
    # vector epilogue with operand strides; the dense RDMI_F32_SLOTS case
    "strided_300x320x320": _c32(300, 320, 320, residual=True),
    "slots_300x320x320": _c32(300, 320, 320, bias=True, residual=True),
    "batched_3x200x256x96": _c32(200, 256, 96, residual=True, batch=3),
    # row edges: M = 1 and one row past a 64- (x6) / 128-row tile
    "rows_1x320x64": _c32(1, 320, 64, residual=True),
    "rows_65x320x64": _c32(65, 320, 64, residual=True),
    "rows_129x320x64": _c32(129, 320, 64, residual=True),
    "rows_257x320x64": _c32(257, 320, 64, residual=True),
    # K tail (the GPU test follows the valid K with NaN)
    "ktail_70x128x8": _c32(70, 128, 8),
    "ktail_70x128x24": _c32(70, 128, 24),
    "ktail_70x128x40": _c32(70, 128, 40),
    "ktail_70x128x72": _c32(70, 128, 72),
    # GEGLU: C = 64, N = 8C value | gate columns → 4C outputs, residual [M, 4C]
    "geglu_70x512x64": _c32(70, 512, 64, bias=True, residual=True, geglu=True),
    # pure products for the RMS criterion
    "rms_70x130x64": _c32(70, 130, 64),
    "rms_130x320x320": _c32(130, 320, 320),
}
RMS_CASES = ("rms_70x130x64", "rms_130x320x320")


@functools.lru_cache(maxsize=None)
def gemm_f32_inputs(name: str) -> dict:
    """Seeded CPU f32 inputs of a case (not f16-rounded): a [B?, M, K], w [B?, N, K] ~ N(0, 1/K), bias [N],
    rowbias [⌈M/rpg⌉, N], residual [B?, M, N] (GEGLU: [M, N/2]; w and bias in value | gate column order)."""
    c = GEMM_F32_CASES[name]
    g = torch.Generator().manual_seed(3000 + sorted(GEMM_F32_CASES).index(name))
    lead = (c["batch"],) if c["batch"] > 1 else ()
    no = c["N"] // 2 if c["geglu"] else c["N"]
    t = {"a": torch.randn(*lead, c["M"], c["K"], generator=g),
         "w": torch.randn(*lead, c["N"], c["K"], generator=g) / math.sqrt(c["K"])}
    t["bias"] = torch.randn(c["N"], generator=g) if c["bias"] else None
    t["rowbias"] = torch.randn(-(-c["M"] // c["rpg"]), c["N"], generator=g) if c["rpg"] else None
    t["residual"] = torch.randn(*lead, c["M"], no, generator=g) if c["residual"] else None
    return t


def _addend32(name: str, dtype, drop_bias_col=None, shift_residual=False, geglu_part=None):
    """The epilogue's addend in `dtype`.  GEGLU: geglu_part "pre" = the bias of the value | gate columns,
    "out" = the residual of the outputs."""
    c, t = GEMM_F32_CASES[name], gemm_f32_inputs(name)
    add = torch.zeros((), dtype=dtype)
    if t["bias"] is not None and geglu_part != "out":
        b = t["bias"].to(dtype).clone()
        if drop_bias_col is not None:
            b[drop_bias_col] = 0
        add = add + b
    if t["rowbias"] is not None:
        add = add + t["rowbias"].to(dtype).repeat_interleave(c["rpg"], 0)[:c["M"]]
    if t["residual"] is not None and geglu_part != "pre":
        r = t["residual"].to(dtype)
        add = add + (torch.roll(r, 1, dims=-2) if shift_residual else r)
    return add


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))


@functools.lru_cache(maxsize=None)
def _gemm_f32_terms(name: str):
    """The np-independent f64 terms: (ref, P, S) — GEGLU: (ref, h, g, P, S of the value | gate columns, |R|)."""
    c, t = GEMM_F32_CASES[name], gemm_f32_inputs(name)
    ad, wd = t["a"].double(), t["w"].double()
    prod = torch.matmul(ad, wd.transpose(-1, -2))
    P = torch.matmul(ad.abs(), wd.abs().transpose(-1, -2))
    if c["geglu"]:
        pre = prod + _addend32(name, torch.float64, geglu_part="pre")
        S = P + t["bias"].double().abs()
        h, g = pre.chunk(2, dim=-1)
        R = _addend32(name, torch.float64, geglu_part="out")
        return h * _gelu(g) + R, h, g, P, S, R.abs() + torch.zeros_like(h)
    ref = prod + _addend32(name, torch.float64)
    S = P.clone()
    for k in ("bias", "rowbias", "residual"):
        if t[k] is not None:
            v = t[k].double().abs()
            S = S + (v.repeat_interleave(c["rpg"], 0)[:c["M"]] if k == "rowbias" else v)
    if c["silu"]:
        ref = F.silu(ref)
    return ref, P, S


@functools.lru_cache(maxsize=None)
def gemm_f32_ref(name: str, np_: int):
    """(f64 reference, its bound for engine np_) of an f32 case."""
    c = GEMM_F32_CASES[name]
    if not c["geglu"]:
        ref, P, S = _gemm_f32_terms(name)
        return ref, f32_bound(ref, P, S, c["K"], np_, c["silu"])
    ref, h, g, P, S, R = _gemm_f32_terms(name)
    e = F32_C[np_] * P + (F32_M[np_] * c["K"] + 8) * U24 * S + U24 * torch.cat((h, g), -1).abs()
    eh, eg = e.chunk(2, dim=-1)
    return ref, _gelu(g).abs() * eh + 1.13 * (h.abs() + eh) * eg + 8 * U24 * (h * g).abs() + \
        2 * U24 * ((h * _gelu(g)).abs() + R)


def split_parts_bf16(x: torch.Tensor, np_: int):
    """x (f32) → its np_ bf16 parts as f32 tensors: RNE at every step, each remainder exact in f32."""
    parts, r = [], x
    for _ in range(np_):
        p = r.to(BF16).float()
        parts.append(p)
        r = r - p
    return parts


def gemm_product_f32(a: torch.Tensor, w: torch.Tensor, np_: int, drop=None) -> torch.Tensor:
    """a @ wᵀ as the engine forms it: exact f32 matmul (np_ = 1), or the kept products of the bf16 parts as
    f32 matmuls added in the kernel's order; drop = index of a kept product to leave out."""
    if np_ == 1:
        return torch.matmul(a, w.transpose(-1, -2))
    ap, wp = split_parts_bf16(a, np_), split_parts_bf16(w, np_)
    y = None
    for i, (wi, ai) in enumerate(F32_PRODUCTS[np_]):
        if i == drop:
            continue
        t = torch.matmul(ap[ai], wp[wi].transpose(-1, -2))
        y = t if y is None else y + t
    return y


def gemm_emulate_f32(name: str, np_: int, wrong: str = "") -> torch.Tensor:
    """Plain CPU emulation of engine np_ on an f32 case: split with .to(bfloat16), the kept part pairs as f32
    matmuls in the kernel's order, the epilogue in f32.  wrong: "bias" (bias of one column dropped), "silu"
    (activation omitted), "residual" (residual rows shifted by one), "ktail" (one NaN at column K of A leaks
    in) or "part<i>" (kept product i dropped)."""
    c, t = GEMM_F32_CASES[name], gemm_f32_inputs(name)
    a, w = t["a"], t["w"]
    if wrong == "ktail":  # column K: NaN in one row of A against a zero weight column
        col = torch.zeros(*a.shape[:-1], 1)
        col[..., c["M"] // 2, 0] = float("nan")
        a, w = torch.cat((a, col), -1), torch.cat((w, torch.zeros(*w.shape[:-1], 1)), -1)
    drop = int(wrong[4:]) if wrong.startswith("part") else None
    if drop is not None and not 0 <= drop < len(F32_PRODUCTS[np_]):
        raise ValueError(f"engine np={np_} keeps no product {drop}")
    y = gemm_product_f32(a, w, np_, drop)
    kw = dict(drop_bias_col=c["N"] // 2 if wrong == "bias" else None, shift_residual=wrong == "residual")
    if c["geglu"]:
        h, g = (y + _addend32(name, torch.float32, geglu_part="pre", **kw)).chunk(2, dim=-1)
        return h * _gelu(g) + _addend32(name, torch.float32, geglu_part="out", **kw)
    y = y + _addend32(name, torch.float32, **kw)
    if c["silu"] and wrong != "silu":
        y = F.silu(y)
    return y


def rel_rms(y: torch.Tensor, ref: torch.Tensor) -> float:
    """rms(y − ref) / rms(ref); NaN / inf in y → inf."""
    y = y.detach().double().cpu()
    if not torch.isfinite(y).all():
        return float("inf")
    return ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@functools.lru_cache(maxsize=None)
def e_seq(name: str) -> float:
    """Relative RMS error of the strictly sequential f32 chain y += a[:, k]·w[:, k], k = 0 .. K−1."""
    c, t = GEMM_F32_CASES[name], gemm_f32_inputs(name)
    y = torch.zeros(c["M"], c["N"])
    for k in range(c["K"]):
        y = y + t["a"][:, k, None] * t["w"][None, :, k]
    return rel_rms(y, _gemm_f32_terms(name)[0])


@functools.lru_cache(maxsize=None)
def rms_limit(name: str, np_: int) -> float:
    """The largest relative RMS error engine np_ may leave on a pure-product case."""
    if np_ == 2:
        return RMS_FACTOR_X3 * rel_rms(gemm_emulate_f32(name, 2), _gemm_f32_terms(name)[0])
    return RMS_FACTOR * e_seq(name)


@functools.lru_cache(maxsize=None)
def conv_case_f32(B, H, W, Cin, Cout, k, stride, pad, alpha=1.0, rowbias=0, seed=0, pad_tl=None, out_hw=None,
                  upsample=False, image_scale=False):
    """conv_case's f32 sibling: seeded CPU f32 inputs (x NHWC, w [Cout, Cin, k, k], bias, residual NHWC,
    rowbias: 0 none, 1 [Cout], 2 per image [B, Cout]; not f16-rounded) with the f64 reference
    alpha·conv(x, w) + bias (+ rowbias) + residual and the terms P, S, K of f32_bound.  pad_tl / out_hw /
    upsample as kernels.conv2d (top/left padding pad_tl, bottom/right implied by out_hw; nearest ×2 upsample
    ahead of the conv); image_scale: image i scaled and offset by 0.6·(i + 1)."""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(B, H, W, Cin, generator=g)
    if image_scale:
        sc = torch.arange(1, B + 1).view(B, 1, 1, 1) * 0.6
        x = x * sc + sc
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    bias = torch.randn(Cout, generator=g)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    if upsample:
        xd = F.interpolate(xd, scale_factor=2.0, mode="nearest")
    Hi, Wi = xd.shape[2:]
    pt = pad if pad_tl is None else pad_tl
    Ho, Wo = out_hw or ((Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1)
    xp = F.pad(xd, (pt, max(0, (Wo - 1) * stride + k - Wi - pt), pt, max(0, (Ho - 1) * stride + k - Hi - pt)))

    def conv(xx, ww):
        return F.conv2d(xx, ww, stride=stride)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)

    P = abs(alpha) * conv(xp.abs(), wd.abs())
    res = torch.randn(B, Ho, Wo, Cout, generator=g)
    ref = alpha * conv(xp, wd) + bias.double() + res.double()
    S = P + bias.double().abs() + res.double().abs()
    rb = None
    if rowbias:
        rb = torch.randn((Cout,) if rowbias == 1 else (B, Cout), generator=g)
        rbd = rb.double() if rowbias == 1 else rb.double()[:, None, None, :]
        ref, S = ref + rbd, S + rbd.abs()
    return dict(x=x, w=w, bias=bias, residual=res, rowbias=rb, ref=ref, P=P, S=S, K=k * k * Cin)


def conv_f32_bound(cs: dict, np_: int) -> torch.Tensor:
    return f32_bound(cs["ref"], cs["P"], cs["S"], cs["K"], np_)
