"""Inputs, f64 references and derived bounds of the GroupNorm / LayerNorm / decoder-head tests
(tests/test_norm_gpu.py), with plain f32 emulations of the kernels for the CPU check of the bounds
themselves (tests/test_norm_cpu.py).  Everything here is device-agnostic torch; nothing is tuned to a
kernel's output.

GroupNorm data: x[b, :, c] = randn·σ_b + off[b, group(c)], off[b, g] = ±ρ·σ_b·u (u ∈ [0.5, 1], random
sign), σ_b = 0.5, 4, 1 by image — every (image, group) has its own mean and rstd, so statistics of a
wrong image or group are an O(1) error, and |mean|/σ reaches ρ.

Bounds (u = 2⁻²⁴, the f32 unit roundoff; all against f64 of the stored inputs):
  stats, stand-alone pass   |mean − m| ≤ 4u·(|m| + σ)            |rstd/r − 1| ≤ 4u
                            (an exact sum rounded once to f32 gives u: a 4× margin)
  stats, producer moments   |mean − m| ≤ 9u·(|m| + σ)            |rstd/r − 1| ≤ 14u·(1 + ρ_g²)
                            (f32 sums over 128 elements, about 9 roundings, then E[x²] − E[x]²)
  GroupNorm output, f32     |y − ref| ≤ 8u·(R_c + |ref| + 1), R_c = |mean·rstd·γ_c|
                            (fma(x, sc, sh) cancels two terms of size R_c)
  output, f16               |y − ref| ≤ ½·ulp16(ref) + 2⁻¹⁴·max(1, |ref|)
  LayerNorm output, f32     |y − ref| ≤ (8·NV + 8)·u·ρ_row·|γ_c| + 8u·(|ref| + 1)
                            (the f32 row mean: 8·NV sequential adds per lane + 6 butterfly levels)
"""
import functools
import math

import torch

U24 = 2.0 ** -24
U22 = 2.0 ** -22
SIGMAS = (0.5, 4.0, 1.0)  # per image (GroupNorm, head) / per row, cycling (LayerNorm)


def ulp16(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of f16 at |ref| (2⁻²⁴ in the subnormal range)."""
    _, e = torch.frexp(ref.abs().double().clamp_min(2.0 ** -14))  # |ref| = m·2^e, m ∈ [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - 11)


def f16_out_bound(ref: torch.Tensor) -> torch.Tensor:
    return 0.5 * ulp16(ref) + 2.0 ** -14 * ref.abs().clamp_min(1.0)


def excess(y: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max |y − ref| / bound on ref's device (≤ 1: inside the bound); NaN / inf in y → inf."""
    y = y.detach().double().to(ref.device)
    if not torch.isfinite(y).all():
        return float("inf")
    return ((y - ref).abs() / bound).max().item()


# ----------------------------------------------------------------------------- GroupNorm
def group_stats64(x: torch.Tensor, G: int, eps: float):
    """(mean, σ, rstd) f64 [B, G] of x [B, ..., C] as stored, two-pass."""
    B, C = x.shape[0], x.shape[-1]
    xd = x.double().reshape(B, -1, G, C // G)
    m = xd.mean(dim=(1, 3))
    var = ((xd - m[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return m, var.sqrt(), (var + eps).rsqrt()


def gn_eps(C: int) -> float:
    return 1e-5 if C in (320, 2560) else 1e-6


@functools.lru_cache(maxsize=None)
def gn_case(C: int, G: int, HW: int, rho: float, f16: bool, B: int = 3, device: str = "cpu") -> dict:
    """Seeded inputs (drawn on the CPU, moved to `device`) with the f64 statistics of the stored x."""
    g = torch.Generator().manual_seed(C * 1000003 + HW * 101 + int(rho) * 7 + int(f16))
    cpg = C // G
    sig = torch.tensor(SIGMAS[:B])
    u = 0.5 + 0.5 * torch.rand(B, G, generator=g)
    sign = torch.randint(0, 2, (B, G), generator=g).float() * 2 - 1
    off = sign * rho * sig[:, None] * u
    x = torch.randn(B, HW, C, generator=g) * sig[:, None, None] + off.repeat_interleave(cpg, 1)[:, None, :]
    x = (x.half() if f16 else x).to(device)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(device)
    beta = (0.1 * torch.randn(C, generator=g)).to(device)
    eps = gn_eps(C)
    m, s, r = group_stats64(x, G, eps)
    return dict(x=x, gamma=gamma, beta=beta, eps=eps, G=G, off=off, m64=m, s64=s, r64=r)


def stats_excess(mr: torch.Tensor, m64, s64, r64, km: float = 4.0, kr=4.0):
    """(mean error / bound, rstd error / bound), the largest over (image, group): bounds km·u·(|m| + σ)
    and kr·u on the relative rstd (kr may be a [B, G] tensor)."""
    mr = mr.double().to(m64.device).view(*m64.shape, 2)
    if not torch.isfinite(mr).all():
        return float("inf"), float("inf")
    dm = (mr[..., 0] - m64).abs()
    em = torch.where(dm == 0, dm, dm / (km * U24 * (m64.abs() + s64)))  # an all-zero image: bound 0, met exactly
    er = (mr[..., 1] / r64 - 1).abs() / (kr * U24)
    return em.max().item(), er.max().item()


def gn_ref(cs: dict):
    """(f64 GroupNorm output [B, HW, C] before any SiLU, R_c [B, 1, C])."""
    cpg = cs["x"].shape[-1] // cs["G"]
    m = cs["m64"].repeat_interleave(cpg, 1)[:, None, :]
    r = cs["r64"].repeat_interleave(cpg, 1)[:, None, :]
    gm = cs["gamma"].double()
    ref = (cs["x"].double() - m) * r * gm + cs["beta"].double()
    return ref, (m * r * gm).abs()


def gn_out_bound(ref: torch.Tensor, R: torch.Tensor, f16: bool) -> torch.Tensor:
    return f16_out_bound(ref) if f16 else 2.0 ** -21 * (R + ref.abs() + 1)


def gn_emulate(cs: dict, accum: str = "f64") -> tuple:
    """(mean_rstd [B, G, 2] f32, y) of a plain model of the kernels: the statistics from exact sums
    rounded once to f32 (accum="f64"), or from sequential f32 Σx / Σx² over 64-row strips combined in
    f64 with var = Σx²/n − mean² (accum="f32": the arithmetic the bounds must reject at ρ ≥ 8); then
    y = fma(x, sc, sh) in f32 with sc = rstd·γ, sh = β − mean·sc, rounded to x's dtype."""
    x, G, eps = cs["x"], cs["G"], cs["eps"]
    B, HW, C = x.shape
    cpg = C // G
    if accum == "f64":
        mean, rstd = cs["m64"].float(), cs["r64"].float()
    else:
        xf = x.float()
        S = torch.zeros(B, C, dtype=torch.float64, device=x.device)
        SS = torch.zeros_like(S)
        for r0 in range(0, HW, 64):
            s = torch.zeros(B, C, device=x.device)
            ss = torch.zeros_like(s)
            for r in range(r0, min(r0 + 64, HW)):
                s = s + xf[:, r]
                ss = torch.addcmul(ss.double(), xf[:, r].double(), xf[:, r].double()).float()  # fma: one rounding
            S, SS = S + s.double(), SS + ss.double()
        n = HW * cpg
        md = S.view(B, G, cpg).sum(-1) / n
        var = (SS.view(B, G, cpg).sum(-1) / n - md * md).clamp_min(0)
        mean, rstd = md.float(), (var + eps).rsqrt().float()
    sc = rstd.repeat_interleave(cpg, 1) * cs["gamma"]
    sh = cs["beta"] - mean.repeat_interleave(cpg, 1) * sc
    # f32 fma: the exact product and sum in f64 (24 + 24 bits fit), rounded once
    y = (x.double() * sc.double()[:, None, :] + sh.double()[:, None, :]).float()
    return torch.stack([mean, rstd], -1), y.to(x.dtype)


# ----------------------------------------------------------------------------- LayerNorm
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(M: int, C: int, f16: bool, device: str = "cpu") -> dict:
    """Rows randn·σ + ρ·σ·sign: σ cycles through SIGMAS, ρ is 0 or 32 and the sign ±1 by row, at random
    (a single row: ρ = 32).  With the f64 reference and its bound."""
    g = torch.Generator().manual_seed(M * 7919 + C * 13 + int(f16))
    sig = torch.tensor([SIGMAS[i % 3] for i in range(M)])[:, None]
    rho = 32.0 * torch.randint(0, 2, (M, 1), generator=g).float() if M > 1 else torch.full((1, 1), 32.0)
    sign = torch.randint(0, 2, (M, 1), generator=g).float() * 2 - 1
    x = torch.randn(M, C, generator=g) * sig + rho * sig * sign
    x = (x.half() if f16 else x).to(device)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(device)
    beta = (0.1 * torch.randn(C, generator=g)).to(device)
    xd = x.double()
    m = xd.mean(-1, keepdim=True)
    var = ((xd - m) ** 2).mean(-1, keepdim=True)
    ref = (xd - m) * (var + LN_EPS).rsqrt() * gamma.double() + beta.double()
    if f16:
        bound = f16_out_bound(ref)
    else:
        nv = (C // 8 + 63) // 64
        rho_row = m.abs() * (var + LN_EPS).rsqrt()
        bound = (8 * nv + 8) * U24 * rho_row * gamma.double().abs() + 2.0 ** -21 * (ref.abs() + 1)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref, bound=bound)


def ln_emulate(cs: dict) -> torch.Tensor:
    """f32 model of the two-pass kernel: lane l owns the 8-element vectors l, l + 64, …; it adds its
    elements one after another, the 64 lanes combine in a 6-level butterfly; mean = Σ/C, then the same for
    Σ(x − mean)²; y = (x − mean)·rstd·γ + β, every step rounded to f32."""
    x = cs["x"].float()
    M, C = x.shape
    nv = (C // 8 + 63) // 64
    pad = torch.zeros(M, nv * 512, device=x.device)
    pad[:, :C] = x
    valid = torch.zeros(nv * 512, dtype=torch.bool, device=x.device)
    valid[:C] = True

    def wave_sum(v):  # v [M, nv·512] → [M, 1]: per-lane sequential sums, then the butterfly
        lanes = v.view(M, nv, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, nv * 8)
        s = torch.zeros(M, 64, device=x.device)
        for j in range(nv * 8):
            s = s + lanes[:, :, j]
        o = 32
        while o:
            s = s + s[:, torch.arange(64, device=x.device) ^ o]
            o >>= 1
        return s[:, :1]

    mean = wave_sum(pad) / C
    d = torch.where(valid, pad - mean, torch.zeros_like(pad))
    rstd = (wave_sum(d * d) / C + LN_EPS).rsqrt()
    y = (x - mean) * rstd * cs["gamma"] + cs["beta"]
    return y.to(cs["x"].dtype)


# ----------------------------------------------------------------------------- decoder head
def head_groups(C: int) -> int:
    return {8: 4, 16: 8, 24: 8, 32: 8}.get(C, 32)


@functools.lru_cache(maxsize=None)
def head_case(B: int, H: int, W: int, C: int, rho: float, f16: bool, device: str = "cpu") -> dict:
    """GroupNorm data of gn_case as [B, H, W, C], tap weights w9 [9, C] (tap = 3·dy + dx) scaled
    1/√(9C), and the f64 references GroupNorm → (SiLU) → 3×3 conv (zero padding 1) to one channel + bias,
    [B, H, W, 1], without and with the SiLU."""
    G = head_groups(C)
    cs = dict(gn_case(C, G, H * W, rho, f16, B, device))
    g = torch.Generator().manual_seed(C * 31 + H * 7 + W)
    w9 = (torch.randn(9, C, generator=g) / math.sqrt(9 * C)).to(device)
    bias = 0.3
    n, _ = gn_ref(cs)
    refs = {}
    for silu in (False, True):
        a = (n * torch.sigmoid(n) if silu else n).view(B, H, W, C)
        p = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device=a.device)
        p[:, 1:-1, 1:-1] = a
        out = torch.full((B, H, W), bias, dtype=torch.float64, device=a.device)
        for dy in range(3):
            for dx in range(3):
                out = out + (p[:, dy:dy + H, dx:dx + W] * w9[3 * dy + dx].double()).sum(-1)
        refs[silu] = out[..., None]
    cs.update(x=cs["x"].view(B, H, W, C), w9=w9, bias=bias, refs=refs)
    return cs
