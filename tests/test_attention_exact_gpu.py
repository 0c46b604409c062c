"""The f16 flash-attention kernels on exactly computable inputs (tests/attention_util.py): attn_fwd_d64,
attn_fwd_d64_pipe and both rdmi_attention_d512 variants against the f64 softmax, each element within
    2⁻¹¹·|ref| + (T + 4)·2⁻²⁴·A + 2⁻²⁵        (T = the kernel's own key tiles)
— one f16 rounding and the f32 roundings of l, P·V, 1/l and the product.  q / k / v are column slices
of one fused buffer whose rows past Sq / Sk are NaN (a read past Sk shows: 0·NaN = NaN), the output a
channel slice of a NaN-filled parent whose border must stay NaN.  tests/test_attention_exact_cpu.py
shows what the bound rejects (a dropped, doubled or unmasked key, a missing l / O rescale, a stale ring
slot, swapped heads) and that the inputs themselves stay inside it."""
import collections

import pytest
import torch

from tests import attention_util as U
from tests.test_kernels_gpu import attn_engine, d512_kernel  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
_cache = {}
_worst = collections.defaultdict(float)  # (kernel, case group) → largest excess seen


def _k():
    from rollingdepth_amd import kernels as K
    return K


def _case(name):
    """The case with its f64 reference, computed once and shared (read-only)."""
    if name not in _cache:
        c = U.dyadic_case(name)
        c["ref"], c["A"] = U.reference(c)
        _cache[name] = c
    return _cache[name]


def _group(c):
    return "uniform" if c["uniform"] else "flat" if not any(c["off"] + c["off1"]) else "schedule"


def _note(kernel, c, e):
    key = (kernel, _group(c))
    _worst[key] = max(_worst[key], e)
    print(f"{kernel} {c['name']}: excess {e:.3f} (largest so far for {key[1]} cases: {_worst[key]:.3f})")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch_d64(c):
    """→ (out [B, Sq, C], parent, border mask): q / k / v from one fused [B, S + 8, 3C] buffer."""
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    C = H * 64
    buf = torch.full((B, max(Sq, Sk) + 8, 3 * C), NAN, dtype=torch.float16, device=DEV)
    buf[:, :Sq, :C] = c["q"].to(DEV)
    buf[:, :Sk, C:2 * C] = c["k"].to(DEV)
    buf[:, :Sk, 2 * C:] = c["v"].to(DEV)
    parent = torch.full((B, Sq + 3, C + 16), NAN, dtype=torch.float16, device=DEV)
    out = parent[:, :Sq, 8:8 + C]
    _k().attention(buf[:, :Sq, :C], buf[:, :Sk, C:2 * C], buf[:, :Sk, 2 * C:], H, out=out, scale=U.SCALE)
    border = torch.ones_like(parent, dtype=torch.bool)
    border[:, :Sq, 8:8 + C] = False
    return out, parent, border


@pytest.mark.parametrize("name", list(U.D64_CASES))
def test_attention_d64_exact(name, attn_engine):
    c = _case(name)
    out, parent, border = _launch_d64(c)
    T = U.tiles(c["Sk"], U.TK_PIPE if attn_engine == "pipe" else U.KB_D64)
    e = U.excess(out, c["ref"], U.bound(c["ref"], c["A"], T))
    _note(attn_engine, c, e)
    assert torch.isnan(parent[border]).all()  # nothing written outside the slice or past Sq
    assert torch.equal(_bits(_launch_d64(c)[0]), _bits(out))  # a repeated launch: the same bits
    assert e <= 1.0


def test_attention_d64_setprio_bitwise(monkeypatch):
    """attn_fwd_d64 with its softmax block at raised priority (RDMI_ATTN_SPRIO=1): a scheduling switch,
    the same bits."""
    monkeypatch.setenv("RDMI_ATTN_PIPE", "0")
    c = _case("sk769_wrap")
    monkeypatch.setenv("RDMI_ATTN_SPRIO", "0")
    o0 = _launch_d64(c)[0]
    monkeypatch.setenv("RDMI_ATTN_SPRIO", "1")
    o1 = _launch_d64(c)[0]
    assert torch.isfinite(o0).all() and torch.equal(_bits(o0), _bits(o1))


def _launch_d512(c):
    """q, k, v with row strides of their own; NaN rows behind q and k, NaN columns beside all three
    (v's batch stride must be Sk rows: it is transposed into the kernel's Vᵀ operand first)."""
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    qb = torch.full((B, Sq + 8, 512 + 24), NAN, dtype=torch.float16, device=DEV)
    kb = torch.full((B, Sk + 8, 512 + 40), NAN, dtype=torch.float16, device=DEV)
    vb = torch.full((B, Sk, 512 + 8), NAN, dtype=torch.float16, device=DEV)
    qb[:, :Sq, 8:520] = c["q"].to(DEV)
    kb[:, :Sk, 16:528] = c["k"].to(DEV)
    vb[:, :, :512] = c["v"].to(DEV)
    # the kernel's output is allocated inside attention_d512: leave a freed NaN block of its size for
    # the allocator to hand out, so that a query block nobody writes does not show an earlier result
    poison = torch.full((B, Sq, 512), NAN, dtype=torch.float16, device=DEV)
    del poison
    return _k().attention_d512(qb[:, :Sq, 8:520], kb[:, :Sk, 16:528], vb[:, :, :512], U.SCALE)


@pytest.mark.parametrize("name", list(U.D512_CASES))
def test_attention_d512_exact(name, d512_kernel):
    c = _case(name)
    out = _launch_d512(c)
    e = U.excess(out, c["ref"], U.bound(c["ref"], c["A"], U.tiles(c["Sk"], U.KT_D512)))
    _note("d512_" + d512_kernel, c, e)
    assert torch.equal(_bits(_launch_d512(c)), _bits(out))  # a repeated launch: the same bits
    assert e <= 1.0


def test_report_largest_excess():
    """The largest excess per kernel and case group over this run (printed; the tests above assert)."""
    for (kernel, group), e in sorted(_worst.items()):
        print(f"{kernel:8s} {group:8s} largest excess {e:.3f}")
