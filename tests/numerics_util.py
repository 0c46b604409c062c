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
accumulation term grows by |silu′| ≤ 1.1.  Nothing here is tuned to a kernel's output."""
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
