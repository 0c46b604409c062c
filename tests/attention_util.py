"""Exactly computable inputs for the f16 flash-attention kernels (attn_fwd_d64, attn_fwd_d64_pipe,
the two rdmi_attention_d512 variants), their f64 reference with a derived elementwise bound, and a
torch restatement of the kernels' loop with switchable defects.  CPU only.

Dyadic inputs.  With scale = ln 2 the kernels' scale·log2(e) rounds to 1 in f32, so the prescaled Q
is Q.  Query i is one-hot (value 1) at dimension i mod D, K holds small integers and V integers in
[−8, 8]: every log2-score is an integer, P = exp2(S′) a power of two, and as long as the scores of
one tile span at most 5 units the packed-f16 row-sum tree, the f32 l and the f32 P·V accumulation
are exact.  What is left is 1/l, the product o·(1/l) and the f16 store, so per element

    |o − ref| ≤ 2⁻¹¹·|ref| + (T + 4)·2⁻²⁴·A + 2⁻²⁵,     A = Σⱼ pⱼ|vⱼ| (f64), T = key tiles:

the half-ulp of the one f16 rounding; the f32 roundings of l and P·V (one per tile, where a jump of
m̃ pushes the range past 24 bits), of 1/l and of the product; the f16 subnormal spacing.

K[j, d] = base[j, d] + off[j // ot, class(d)], base ∈ {0..4} random: `off` is a case's schedule of
integer tile offsets (ot = the offset tile: 128 keys for the d = 64 cases, 32 for d = 512, multiples
of every kernel tile, so that one kernel tile never spans more than 5 units).  Schedules are written
with their maximum at 0 and their last tile near it, so that a zero-filled key past Sk (score 0) and
the last key both carry visible weight.
"""
import math
import zlib

import torch

KB_D64 = 128      # attention.hip: KB, keys per tile of attn_fwd_d64
NSLOT_D64 = 5     # attention.hip: NSLOT, its LDS ring
TK_PIPE = 64      # attention.hip: pp::TK, keys per tile of attn_fwd_d64_pipe
NSL_PIPE = 4      # attention.hip: pp::NSL
KT_D512 = 32      # attention_d512.hip: KT5, keys per tile of both d = 512 kernels
NSTAGE_D512 = 2   # attention_d512.hip: the two LDS stages
SCALE = math.log(2.0)

DEFECTS = ("drop_last_key", "duplicate_last_key", "unmasked_padding", "skip_l_rescale", "skip_o_rescale",
           "stale_tile_after_ring_wrap", "swap_two_heads")


def _case(Sq, Sk, off=None, off1=None, cls="dim4", uniform=False, D=64, B=2, H=3):
    """off: offsets per offset tile for the dimensions of class 0; off1: for class 1 (default: off).
    cls: "dim4" class(d) = (d // 4) & 1 (both classes inside every wave); "blk128" class(d) =
    (d // 128) & 1 (d = 512: the odd 128-query blocks)."""
    ot = KB_D64 if D == 64 else KT_D512
    n = (Sk + ot - 1) // ot
    off = [0] * n if off is None else list(off)
    off1 = off if off1 is None else list(off1)
    assert len(off) == n and len(off1) == n, (Sq, Sk, off, off1)
    return dict(Sq=Sq, Sk=Sk, off=off, off1=off1, cls=cls, uniform=uniform, D=D, B=B, H=H, ot=ot)


# (Sq, Sk) pairs: a lane half without a valid key (4), every mask pattern, ±1 around 32 / 64 / 128 /
# pp::QB, one key in a new tile, the ring wrap at tile 5 (641) and tile 6 (769).
D64_CASES = {
    "sk1": _case(1, 1),
    "sk4": _case(33, 4),
    "sk5": _case(33, 5),
    "sk31": _case(255, 31),
    "sk32": _case(256, 32),
    "sk33": _case(257, 33),
    "sk63": _case(513, 63),
    "sk64": _case(1, 64),
    "sk65": _case(33, 65),
    "sk95": _case(255, 95),
    "sk96": _case(256, 96),
    "sk97": _case(257, 97),
    "sk127": _case(511, 127),
    "sk128": _case(512, 128),
    # a jump of +12 in the last, ragged tile (one key)
    "sk129_last_jump": _case(513, 129, [-12, 0]),
    # the pipe kernel's steady-state loop runs while u + 1 < Sk / 32 − 1: none, one pair, one pair and
    # a guarded sub-tile
    "sk159_rise": _case(33, 159, [-3, 0]),
    "sk160_rise": _case(256, 160, [-3, 0]),
    "sk161_rise": _case(257, 161, [-3, 0]),
    "sk191_rise": _case(255, 191, [-3, 0]),
    "sk192_rise": _case(256, 192, [-3, 0]),
    "sk193_rise": _case(257, 193, [-3, 0]),
    # +3 per tile: no re-set
    "sk257_rise": _case(257, 257, [-6, -3, 0]),
    # only the class-1 queries see a jump (+13 at tile 1); class 0 drops by 2 there, so its lanes are
    # re-set by the wave-wide vote with a negative tile maximum (the max(mx, 0) branch)
    "sk257_partial": _case(33, 257, [0, -2, 0], [-13, 0, 0]),
    # +3, then +12: the row sum leaves the f16 range, P stays finite
    "sk385_jump12": _case(255, 385, [-15, -12, 0, 0]),
    # −20 below m̃: P in the f16 subnormals
    "sk385_drop20": _case(256, 385, [0, -20, 0, 0]),
    # rise, jump, subnormal drop, +35 to the top (P = inf before the re-set) in the tile before the ring
    # wraps, the wrapping tile ragged
    "sk641_jump30": _case(257, 641, [-34, -31, -19, -35, 0, -6]),
    # jump with re-set at tile 2, subnormal tiles, the top again in the tile that re-uses slot 0, one
    # key in tile 6
    "sk769_wrap": _case(513, 769, [-12, -9, 0, -20, -15, 0, -5]),
    "sk129_uniform": _case(33, 129, uniform=True),
    # one miscounted key moves an output by ≈ 1e-3·|v|, the bound is ≈ 1e-5
    "sk3073_uniform": _case(33, 3073, uniform=True),
}

# d = 512: ±1 around 16 / 32 / 128 queries and around multiples of 32 keys; offset tiles of 32 keys
D512_CASES = {
    "d512_sq15_sk31": _case(15, 31, D=512, H=1),
    "d512_sq16_sk32": _case(16, 32, D=512, H=1),
    "d512_sq17_sk33_last_jump": _case(17, 33, [-12, 0], D=512, H=1),
    "d512_sq31_sk63_rise": _case(31, 63, [-3, 0], D=512, H=1),
    "d512_sq32_sk64_drop20": _case(32, 64, [0, -20], D=512, H=1),
    "d512_sq33_sk65_drop20": _case(33, 65, [0, -20, 0], D=512, H=1),
    "d512_sq127_sk95_rise": _case(127, 95, [-6, -3, 0], D=512, H=1),
    "d512_sq128_sk96_jump13": _case(128, 96, [-13, 0, 0], D=512, H=1),
    "d512_sq129_sk97_jump30": _case(129, 97, [-34, -31, 0, -1], D=512, H=1),
    # only the odd 128-query blocks overflow (+31: P = inf under the 32-query pass's fixed m̃, so their
    # result can only come from the fix-up): flagged and unflagged blocks in one launch
    "d512_sq513_sk129_odd_blocks": _case(513, 129, [0, 0, -1, 0, 0], [-34, -31, 0, 0, 0], cls="blk128", D=512, H=1),
    "d512_sq33_sk129_uniform": _case(33, 129, uniform=True, D=512, H=1),
}

CASES = {**D64_CASES, **D512_CASES}


def _cls(d: torch.Tensor, kind: str) -> torch.Tensor:
    return (d // 4) % 2 if kind == "dim4" else (d // 128) % 2


def dyadic_case(name: str) -> dict:
    """q [B, Sq, H·D], k, v [B, Sk, H·D] as f16 CPU tensors, plus the case's metadata."""
    c = dict(CASES[name])
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    base = torch.randint(0, 5, (B, Sk, H * D), generator=g)
    v = torch.randint(-8, 9, (B, Sk, H * D), generator=g)
    d = torch.arange(H * D) % D
    tile = torch.arange(Sk) // c["ot"]
    off = torch.stack([torch.tensor(c["off"]), torch.tensor(c["off1"])], 1)  # [tiles, class]
    k = base + off[tile][:, _cls(d, c["cls"])][None]
    q = torch.zeros(B, Sq, H, D)
    if not c["uniform"]:
        i = torch.arange(Sq)
        q[:, i, :, i % D] = 1.0
    c.update(name=name, q=q.view(B, Sq, H * D).half(), k=k.half(), v=v.half(), scale=SCALE)
    return c


def _heads(t: torch.Tensor, H: int) -> torch.Tensor:
    B, S, HD = t.shape
    return t.view(B, S, H, HD // H).transpose(1, 2)  # [B, H, S, D]


def reference(case: dict, scale=None):
    """(ref, A) in f64, [B, Sq, H·D]: softmax(q kᵀ·scale) v and Σⱼ pⱼ|vⱼ|."""
    H = case["H"]
    q, k, v = (_heads(case[n].double(), H) for n in "qkv")
    p = torch.softmax(q @ k.transpose(-1, -2) * (case["scale"] if scale is None else scale), -1)
    B, _, Sq, D = q.shape
    return ((p @ v).transpose(1, 2).reshape(B, Sq, H * D), (p @ v.abs()).transpose(1, 2).reshape(B, Sq, H * D))


def tiles(Sk: int, KB: int) -> int:
    return (Sk + KB - 1) // KB


def bound(ref: torch.Tensor, A: torch.Tensor, T: int) -> torch.Tensor:
    return 2.0 ** -11 * ref.abs() + (T + 4) * 2.0 ** -24 * A + 2.0 ** -25


def excess(y: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> float:
    """max over the elements of |y − ref| / bound (≤ 1: inside the bound); NaN / inf in y → inf."""
    y = y.detach().double().cpu()
    if not torch.isfinite(y).all():
        return float("inf")
    return ((y - ref).abs() / bnd).max().item()


def _half_sums(p: torch.Tensor) -> torch.Tensor:
    """Row sums of the f16 P [.., KB] as the kernel forms them: per lane half (keys with (j % 8) // 4 =
    hh) a pairwise tree of f16 adds down to two values, added in f32 → [.., 2] f32."""
    KB = p.shape[-1]
    j = torch.arange(KB)
    x = torch.stack([p[..., (j % 8) // 4 == hh] for hh in (0, 1)], -2)  # [.., 2, KB / 2]
    while x.shape[-1] > 2:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0].float() + x[..., 1].float()


def flash_restatement(case: dict, KB: int, defect=None, nslot=None, wave: int = 32, scale=None) -> torch.Tensor:
    """attn_fwd_d64's loop (attention.hip, the tile loop and the epilogue) in torch f32 / f16 for tiles
    of KB keys: Q·scale·log2(e) rounded to f16 once; per tile S′ = scores − m̃, P = f16(exp2(S′)), the row
    sum of each lane half a pairwise f16 tree; m̃ set on the first tile and re-set to f16(m̃ + max) —
    with l and O rescaled by exp2(−δ) and P recomputed — when a half's sum exceeds 2¹⁵ for any query of
    its wave (`wave` consecutive queries); O += P·V in f32; result f16(O·(1/l)).  → [B, Sq, H·D] f16.
    defect: one of DEFECTS (stale_tile_after_ring_wrap: tile t ≥ nslot reads tile t − nslot's K / V)."""
    assert defect is None or defect in DEFECTS
    H, Sk = case["H"], case["Sk"]
    nslot = {KB_D64: NSLOT_D64, TK_PIPE: NSL_PIPE, KT_D512: NSTAGE_D512}[KB] if nslot is None else nslot
    q, k, v = (_heads(case[n].float(), H) for n in "qkv")
    if defect == "swap_two_heads":
        v = v[:, [1, 0] + list(range(2, H))]
    if defect == "duplicate_last_key":
        k, v = torch.cat([k, k[..., -1:, :]], -2), torch.cat([v, v[..., -1:, :]], -2)
    nvalid = k.shape[-2] - (defect == "drop_last_key")
    nt = tiles(k.shape[-2], KB)
    pad = nt * KB - k.shape[-2]
    k = torch.nn.functional.pad(k, (0, 0, 0, pad))  # keys past Sk read as zeros
    v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    if defect == "unmasked_padding":
        nvalid = nt * KB
    sl2 = torch.tensor(case["scale"] if scale is None else scale, dtype=torch.float32) * torch.tensor(
        1.4426950408889634, dtype=torch.float32)
    s_all = (q * sl2).half().float() @ k.transpose(-1, -2)  # [B, H, Sq, nt·KB]
    B, _, Sq, D = q.shape
    NEG = torch.tensor(float("-inf"))
    o = torch.zeros(B, H, Sq, D)
    l = torch.zeros(B, H, Sq, 2)
    mt = torch.zeros(B, H, Sq)
    nw = (Sq + wave - 1) // wave
    for t in range(nt):
        src = t - nslot if defect == "stale_tile_after_ring_wrap" and t >= nslot else t
        valid = torch.arange(t * KB, (t + 1) * KB) < nvalid
        s = torch.where(valid, s_all[..., src * KB:(src + 1) * KB] - mt[..., None], NEG)
        p = torch.exp2(s).half()
        rs = _half_sums(p)
        over = torch.nn.functional.pad(~(rs <= 32768.0).all(-1), (0, nw * wave - Sq))
        reset = over.view(B, H, nw, wave).any(-1, keepdim=True).expand(B, H, nw, wave).reshape(B, H, -1)[..., :Sq]
        if t == 0:
            reset = torch.ones_like(reset)
        if reset.any():
            mx = s.max(-1).values
            if t != 0:
                mx = mx.clamp_min(0.0)  # never lower m̃
            mnew = torch.where(reset, (mt + mx).half().float(), mt)
            delta = mnew - mt
            alpha = torch.exp2(-delta)
            if defect != "skip_l_rescale":
                l = l * alpha[..., None]
            if defect != "skip_o_rescale":
                o = o * alpha[..., None]
            mt = mnew
            p2 = torch.exp2(s - delta[..., None]).half()
            p = torch.where(reset[..., None], p2, p)
            rs = torch.where(reset[..., None], _half_sums(p2), rs)
        l = l + rs
        o = o + p.float() @ v[..., src * KB:(src + 1) * KB, :]
    inv = 1.0 / (l[..., 0] + l[..., 1])
    return (o * inv[..., None]).half().transpose(1, 2).reshape(B, Sq, H * D)
