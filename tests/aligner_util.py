"""One DepthAligner iteration restated stage by stage, and a mirror of the optimiser's workspace layout.

Neither needs a GPU.  The restatement follows the formulas of oracle/rd_oracle.py::aligner_optimize's
docstring and of csrc/aligner.hip's header, from an arbitrary state (s, t, m, v, step) and for arbitrary
hyper-parameters, and returns every stage:

  A = x·s + t per (snippet, slot, pixel); `alive`: a slot whose row of the [Σw, N, P] tensors a later
      dilation writes at the same frame is overwritten — it counts nowhere;
  T, Td  [N, P]   per frame the mean over its alive slots, in row order, of A and of 1/clip(A, 1e-3);
  sc, scd [N]     the per-frame L1 scales mean|T|, mean|Td|;
  terms           per (snippet, slot, pixel): z = A − T, zd = 1/clip(A) − Td,
                  g = sign(z)/sc + depth_w·sign(zd)/scd·(−1/clip(A)²)·[A ≥ 1e-3]   (dLoss/dA · numel/loss_scale),
                  gs = g·x, gt = g, l1 = |z|/sc, l2 = |zd|/scd;
  partials        their sums per (snippet, pixel chunk), chunk c = [P·c//8, P·(c+1)//8);
  loss            loss_scale·(Σl1 + depth_w·Σl2)/numel + Σ_d λ2·mean(relu(1 − s_d)²) + λ3·mean(t_d²), numel = Σw·N·P;
  grad            Σ partials · loss_scale/numel + the soft terms' −2λ2·relu(1 − s)/n_d and 2λ3·t/n_d;
  Adam            torch.optim.Adam's single-tensor update (lerp with both of its branches, mul + addcmul,
                  sqrt / sqrt(bc2) + eps, addcdiv);
  hist            (loss, min T, max T).

dt = np.float64 evaluates all of it in f64.  dt = np.float32 reproduces the kernels' operation order op by
op (with fused=True also their two fused multiply-adds, see one_iteration; without, the oracle's mul then
add): every f32 operation is one IEEE operation (numpy never contracts), the slots of a pixel are summed in
row order, the means divide by (float)count, 1/ac, isc = 1/sc, (sign·iscd)·(−1/(ac·ac)), g = f64(g1) +
f64(dw)·f64(g2), f64 sums, adam_param's sequence.  The hyper-parameters are the f32 values the C ABI
carries, in both modes.  The device's own earlier stages can be passed in (T / Td, fpart, partials, bct), so
that a stage is judged on the numbers the device itself went on with.
"""
from types import SimpleNamespace

import numpy as np

PS = 8       # csrc/aligner_ws.h RDMI_ALIGNER_PS
HBLK = 128   # csrc/aligner_ws.h RDMI_ALIGNER_HBLK
CLIP = np.float32(1e-3)
U32 = 2.0 ** -24   # unit roundoff of f32
U64 = 2.0 ** -53

LAYOUT_FIELDS = ("gs", "gt", "l1", "l2", "fpart", "T", "Td", "m", "v", "cnt", "bct", "hl", "hmm", "hst", "slots",
                 "total")

DEFAULT_WEIGHTS = dict(depth_w=1.0, loss_scale=1.0, lmda2=0.1, lmda3=10.0, lr=1e-3, betas=(0.5, 0.9), eps=1e-8)
WEIGHT_SETS = {
    "default": DEFAULT_WEIGHTS,
    # 1 − β1 = 0.1 < 0.5: torch.lerp's other branch
    "other": dict(depth_w=0.25, loss_scale=3.0, lmda2=0.5, lmda3=2.0, lr=3e-3, betas=(0.9, 0.999), eps=1e-6),
    "nodepth": dict(DEFAULT_WEIGHTS, depth_w=0.0),
}


def ws_layout(N, P, ntot, iters, hist):
    """Python mirror of rdmi_aligner_ws_layout (csrc/aligner_ws.h): offsets in floats."""
    nps, nfs = ntot * PS, N * PS
    L = {}
    L["gs"] = 0
    L["gt"] = L["gs"] + 2 * nps
    L["l1"] = L["gt"] + 2 * nps
    L["l2"] = L["l1"] + 2 * nps
    L["fpart"] = L["l2"] + 2 * nps
    L["T"] = L["fpart"] + 8 * nfs
    L["Td"] = L["T"] + N * P
    L["m"] = L["Td"] + N * P
    L["v"] = L["m"] + 2 * ntot
    L["cnt"] = L["v"] + 2 * ntot
    L["bct"] = L["cnt"] + ((ntot + 1) & ~1)
    L["hl"] = L["bct"] + 4 * (iters + 1)
    L["slots"] = 0 if not hist else min(iters, HBLK)
    L["hmm"] = L["hl"] + L["slots"] * 4 * nps
    L["hst"] = L["hmm"] + L["slots"] * 2 * nfs
    L["total"] = L["hst"] + L["slots"] * 2 * ntot + (2 if hist else 0) + 64
    return L


def read_workspace(ws, N, P, ntot, iters, hist=True):
    """The regions of a workspace (1-D f32 numpy array, as kernels.aligner_optimize returns it) that the
    three-launch loop leaves behind: the last iteration's intermediates."""
    L = ws_layout(N, P, ntot, iters, hist)

    def f64(name, count):
        return ws[L[name]:L[name] + 2 * count].view(np.float64).copy()

    return SimpleNamespace(
        gs=f64("gs", ntot * PS).reshape(ntot, PS), gt=f64("gt", ntot * PS).reshape(ntot, PS),
        l1=f64("l1", ntot * PS).reshape(ntot, PS), l2=f64("l2", ntot * PS).reshape(ntot, PS),
        fpart=f64("fpart", N * PS * 4).reshape(N, PS, 4),
        T=ws[L["T"]:L["T"] + N * P].reshape(N, P).copy(), Td=ws[L["Td"]:L["Td"] + N * P].reshape(N, P).copy(),
        m=ws[L["m"]:L["m"] + 2 * ntot].copy(), v=ws[L["v"]:L["v"] + 2 * ntot].copy(),
        bct=f64("bct", 2 * (iters + 1)).reshape(iters + 1, 2))


def chunk_bounds(P):
    """Pixel chunk c of a frame or snippet is [b[c], b[c + 1]) (aligner.hip chunk_lo)."""
    return [P * c // PS for c in range(PS + 1)]


def snippet_index(N, w, dilation, start_step=1):
    """[n, w] frame of (snippet, slot): snippets start every start_step frames, plus the last window."""
    last = N - ((w - 1) * dilation + 1)
    assert last >= 0
    starts = list(range(0, last + 1, start_step))
    if starts[-1] != last:
        starts.append(last)
    return np.array([[k + j * dilation for j in range(w)] for k in starts], np.int64)


def alive_mask(idx):
    """alive[d][k, j]: slot j of snippet k of dilation d is not overwritten.  Slot j of dilation d is row
    d·w_d + j; a later dilation with a slot on the same row overwrites it at every frame that slot covers."""
    ws = [ix.shape[1] for ix in idx]
    rb = [d * w for d, w in enumerate(ws)]
    assert all(rb[d] + ws[d] <= sum(ws) for d in range(len(ws))), "rows exceed Σw"
    alive = [np.ones(ix.shape, bool) for ix in idx]
    for d in range(len(idx)):
        for j in range(ws[d]):
            for d2 in range(d + 1, len(idx)):
                j2 = rb[d] + j - rb[d2]
                if 0 <= j2 < ws[d2]:
                    alive[d][:, j] &= ~np.isin(idx[d][:, j], idx[d2][:, j2])
    return alive


def cover_count(idx, N):
    cnt = np.zeros(N, np.int64)
    for ix, al in zip(idx, alive_mask(idx)):
        np.add.at(cnt, ix[al], 1)
    return cnt


def _w32(weights):
    """The hyper-parameters as the f32 values rdmi_aligner_args carries."""
    w = dict(DEFAULT_WEIGHTS, **weights)
    f = np.float32
    return SimpleNamespace(dw=f(w["depth_w"]), ls=f(w["loss_scale"]), l2=f(w["lmda2"]), l3=f(w["lmda3"]), lr=f(w["lr"]),
                           b1=f(w["betas"][0]), b2=f(w["betas"][1]), eps=f(w["eps"]))


def bias_corrections(weights, step):
    """adam_bc_k: 1 − β^step in f64, β the f32 value."""
    w = _w32(weights)
    return 1.0 - float(w.b1) ** step, 1.0 - float(w.b2) ** step


def scales_from_fpart(fpart, P, dt=np.float32):
    """frame_scales: chunk partials Σ|T|, Σ|Td| added in chunk order in f64, ÷ P, rounded to dt."""
    A = np.zeros(fpart.shape[0])
    D = np.zeros(fpart.shape[0])
    for c in range(PS):
        A = A + fpart[:, c, 0]
        D = D + fpart[:, c, 1]
    return (A / float(P)).astype(dt), (D / float(P)).astype(dt)


def fpart_of(T, Td):
    """frame_stats' chunk partials from T, Td: f64 sums of |·|, min and max of T; an empty chunk gives
    0, 0, +inf, −inf."""
    N, P = T.shape
    b = chunk_bounds(P)
    out = np.zeros((N, PS, 4))
    for c in range(PS):
        t = T[:, b[c]:b[c + 1]]
        out[:, c, 0] = np.abs(t.astype(np.float64)).sum(-1)
        out[:, c, 1] = np.abs(Td[:, b[c]:b[c + 1]].astype(np.float64)).sum(-1)
        out[:, c, 2] = t.min(-1) if t.shape[1] else np.inf
        out[:, c, 3] = t.max(-1) if t.shape[1] else -np.inf
    return out


def fma32(a, b, c):
    """fl32(a·b + c) with ONE rounding, for f32 arrays: the product of two f32 is exact in f64; the f64 sum is
    rounded to odd (TwoSum's exact residual as the sticky bit: where the sum is inexact and its last bit even,
    the neighbour towards the residual), after which rounding to f32 is the correct rounding of the exact
    a·b + c (53 ≥ 2·24 + 2 bits)."""
    D = np.float64
    p = np.asarray(a, np.float32).astype(D) * np.asarray(b, np.float32).astype(D)
    p, c = np.broadcast_arrays(p, np.asarray(c, np.float32).astype(D))
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s = np.ascontiguousarray(s)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s).astype(np.float32)


def one_iteration(xs, idx, N, s, t, m, v, step, weights, dt, T=None, Td=None, fpart=None, partials=None, bct=None,
                  fused=False):
    """One iteration from the state (s, t per dilation; m, v flat [2·ntot], s then t) at Adam step `step`.

    fused (dt = np.float32 only): the two places where the kernels round once instead of twice (aligner.hip,
    mulrn): A = fma(x, s, t), and m + lw·diff as one fma in the lerp's weight < 0.5 branch.  fused=False is the
    reference's and the oracle's arithmetic (mul then add).

    xs[d] [n_d, w_d, P] f32, idx[d] [n_d, w_d] frames.  dt: np.float64 or np.float32 (module docstring).
    Optional stage inputs replace the restatement's own (the device's): T and Td [N, P]; fpart [N, PS, 4];
    partials (gs, gt, l1, l2) each [ntot, PS]; bct (bc1, bc2)."""
    F = dt
    f32 = F is np.float32
    W = _w32(weights)
    nd = len(xs)
    P = xs[0].shape[-1]
    wl = [x.shape[1] for x in xs]
    R = sum(wl)
    rb = [d * w for d, w in enumerate(wl)]
    ns = [x.shape[0] for x in xs]
    ntot = sum(ns)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(int)
    denom = float(R) * N * float(P)
    alive = alive_mask(idx)
    cnt = cover_count(idx, N)
    o = SimpleNamespace(alive=alive, cnt=cnt, denom=denom, P=P, ntot=ntot, off=off)

    # ---- A, clip, inverse: A as one fma (fused) or as mul then add, each rounded
    xF = [x.astype(F) for x in xs]
    assert f32 or not fused
    if fused:
        A = [fma32(xF[d], s[d][:, None, None], t[d][:, None, None]) for d in range(nd)]
    else:
        A = [xF[d] * s[d].astype(F)[:, None, None] + t[d].astype(F)[:, None, None] for d in range(nd)]
    Ac = [np.maximum(a, F(CLIP)) for a in A]
    Ad = [F(1.0) / a for a in Ac]
    o.A, o.Ac, o.Ad = A, Ac, Ad

    # ---- frame means, slots in row order
    summ = np.zeros((N, P), F)
    summd = np.zeros((N, P), F)
    for r in range(R):
        for d in range(nd):
            j = r - rb[d]
            if 0 <= j < wl[d]:
                al = alive[d][:, j]
                summ[idx[d][al, j]] += A[d][al, j]
                summd[idx[d][al, j]] += Ad[d][al, j]
    cF = np.maximum(cnt, 1).astype(F)[:, None]
    o.T_own = np.where(cnt[:, None] > 0, summ / cF, F(0))
    o.Td_own = np.where(cnt[:, None] > 0, summd / cF, F(0))
    o.T = o.T_own if T is None else T.astype(F)
    o.Td = o.Td_own if Td is None else Td.astype(F)

    # ---- per-frame scales
    o.fpart_own = fpart_of(o.T, o.Td)
    if f32:
        o.sc, o.scd = scales_from_fpart(o.fpart_own if fpart is None else fpart, P)
    else:
        o.sc, o.scd = np.abs(o.T).sum(-1) / P, np.abs(o.Td).sum(-1) / P

    # ---- per (snippet, slot, pixel) terms
    D = np.float64
    dw = D(W.dw)
    o.z, o.zd, o.terms = [], [], []
    b = chunk_bounds(P)
    own = {k: np.zeros((ntot, PS)) for k in ("gs", "gt", "l1", "l2")}
    o.abs_partials = {k: np.zeros((ntot, PS)) for k in ("gs", "gt", "l1", "l2")}
    with np.errstate(divide="ignore", invalid="ignore"):
        for d in range(nd):
            isc = (F(1.0) / o.sc)[idx[d]][..., None]
            iscd = (F(1.0) / o.scd)[idx[d]][..., None]
            z = A[d] - o.T[idx[d]]
            zd = Ad[d] - o.Td[idx[d]]
            g1 = np.sign(z) * isc
            g2 = np.where(A[d] >= F(CLIP), (np.sign(zd) * iscd) * (F(-1.0) / (Ac[d] * Ac[d])), F(0))
            g = g1.astype(D) + dw * g2.astype(D)
            live = alive[d][..., None]
            tm = dict(gs=np.where(live, g * xs[d].astype(D), 0.0), gt=np.where(live, g, 0.0),
                      l1=np.where(live, np.abs(z.astype(D)) * isc.astype(D), 0.0),
                      l2=np.where(live, np.abs(zd.astype(D)) * iscd.astype(D), 0.0))
            o.z.append(z)
            o.zd.append(zd)
            o.terms.append(tm)
            for c in range(PS):
                for k, a in tm.items():
                    own[k][off[d]:off[d + 1], c] = a[:, :, b[c]:b[c + 1]].sum(axis=(1, 2))
                    o.abs_partials[k][off[d]:off[d + 1], c] = np.abs(a[:, :, b[c]:b[c + 1]]).sum(axis=(1, 2))
    o.partials_own = own
    pr = own if partials is None else dict(zip(("gs", "gt", "l1", "l2"), partials))

    # ---- loss and history row (the parameters before the update)
    soft = 0.0
    for d in range(nd):
        r = np.maximum(F(0), F(1) - s[d].astype(F))
        td = t[d].astype(F)
        a = float(np.sum(r.astype(D) * r.astype(D)))
        bb = float(np.sum(td.astype(D) * td.astype(D)))
        soft += D(W.l2) * a / ns[d] + D(W.l3) * bb / ns[d]
    L1, L2 = float(pr["l1"].sum()), float(pr["l2"].sum())
    o.loss = D(W.ls) * (L1 / denom + dw * L2 / denom) + soft
    o.hist = (F(o.loss), o.T.min(), o.T.max())

    # ---- gradient and Adam
    bc1, bc2 = bias_corrections(weights, step) if bct is None else (float(bct[0]), float(bct[1]))
    gsum = np.zeros(2 * ntot)
    for c in range(PS):  # chunk order
        gsum = gsum + np.concatenate([pr["gs"][:, c], pr["gt"][:, c]])
    sflat = np.concatenate([x.astype(F) for x in s])
    tflat = np.concatenate([x.astype(F) for x in t])
    pv = np.concatenate([sflat, tflat])
    nn = np.concatenate([np.full(n, n, F) for n in ns] * 2)
    if f32:
        one = F(1)
        gscale = F(D(W.ls) / denom)
        g = (gsum * D(gscale)).astype(F)
        r = np.maximum(F(0), one - sflat)
        gsoft = np.concatenate([((W.l2 * F(2)) * r) * F(-1), (W.l3 * F(2)) * tflat]) / nn
        g = g + gsoft
        step_size = F(D(W.lr) / bc1)
        bc2s = F(np.sqrt(bc2))
        lw, vw = one - W.b1, one - W.b2
        mo, vo = m.astype(F), v.astype(F)
        diff = g - mo
        if lw < F(0.5):
            mn = fma32(lw, diff, mo) if fused else mo + lw * diff
        else:
            mn = g - diff * (one - lw)
        vn = vo * W.b2 + (vw * g) * g
        den = np.sqrt(vn) / bc2s + W.eps
        pn = pv + (-step_size * mn) / den
        assert g.dtype == mn.dtype == vn.dtype == pn.dtype == np.float32
    else:
        r = np.maximum(0.0, 1.0 - sflat)
        gsoft = np.concatenate([-2.0 * D(W.l2) * r, 2.0 * D(W.l3) * tflat]) / nn
        g = gsum * D(W.ls) / denom + gsoft
        b1, b2 = D(W.b1), D(W.b2)
        mn = m.astype(D) + (1.0 - b1) * (g - m.astype(D))
        vn = b2 * v.astype(D) + (1.0 - b2) * g * g
        pn = pv - (D(W.lr) / bc1) * mn / (np.sqrt(vn) / np.sqrt(bc2) + D(W.eps))
    o.grad, o.grad_soft, o.m, o.v = g, gsoft, mn, vn
    o.s = [pn[off[d]:off[d + 1]] for d in range(nd)]
    o.t = [pn[ntot + off[d]:ntot + off[d + 1]] for d in range(nd)]
    return o


# ------------------------------------------------------------------------------------------------ bounds
def rounding_bounds(xs, idx, N, s, t, weights, r64):
    """First-order bounds on what f32 evaluation (the kernels' operation order) can differ from the f64
    reference r64 = one_iteration(..., dt=np.float64) of the same inputs, u = 2⁻²⁴, each rounding at most u
    times the magnitude of its own result:

    a = fl(fl(x·s) + t):    |δa| ≤ u·(|x·s| + |a|);
    T = fl(Σ_c a_i / c):     the kernels' arithmetic (a = fma(x, s, t), ONE rounding, relative to |a|): c + 2
                             roundings per pixel (the fma, c running-sum adds counting the first, the division),
                             every rounded quantity at most Σ_i |a_i|: |δT| ≤ `T_tight` = (c + 3)·u·Σ_i|a_i|/c on
                             every pixel.  Mul then add rounds the product relative to |x·s|, which exceeds |a|
                             where t < 0 cancels it: c + 3 roundings of quantities ≤ M = Σ_i (|x_i·s_i| + |t_i|),
                             |δT| ≤ `T` = (c + 3)·u·M/c; where every covering t_i ≥ 0 (`T_nocancel`, x ≥ 0, s > 0)
                             M = Σ|a_i| and `T_tight` holds for two roundings as well.
    ad = fl(1/ac):           |δad| ≤ ad·(|δa|/ac + u), ac = max(a, 1e-3) (the clip is 1-Lipschitz);
    Td = fl(Σ ad_i / c):     |δTd| ≤ (Σ_i |δad_i| + (c + 1)·u·Σ_i ad_i)/c;
    sc = fl(mean|T|):        |δsc| ≤ mean_p |δT| + u·sc (its f64 sums add ≤ P·2⁻⁵³, absorbed in the 5 % below).

    A term is undecidable when f32 and f64 may take different branches of sign(z), sign(zd) or the clip mask:
    |z| ≤ max(|δa| + |δT|, 2 ulp), |zd| ≤ max(|δad| + |δTd|, 2 ulp) or |a − 1e-3| ≤ max(|δa|, 2 ulp) — except at
    frames with one covering slot, where T = a and Td = ad exactly in either arithmetic (z = zd = 0).  An
    undecidable term may flip: it contributes twice its magnitude.  A decidable term keeps its sign and carries
    the relative error of its factors: sign/sc: δsc/sc + 3u (sc's rounding, the reciprocal, the product);
    sign/scd·(−1/ac²): δscd/scd + 2|δa|/ac + 6u.  The f64 sums of the terms, the scale by loss_scale/numel, the
    soft term and Adam's lerp (m = (1 − β1)·g after the first step) add 8 roundings of f32 on the gradient's
    two parts.  Everything is multiplied by 1.05 for the second-order terms dropped.

    Returns bounds for T, Td, the gradient (flat [2·ntot]), the loss, the undecidable fraction of the terms and
    their number per snippet."""
    W = _w32(weights)
    D = np.float64
    u = U32
    nd = len(xs)
    P = xs[0].shape[-1]
    cnt = r64.cnt
    ntot, off = r64.ntot, r64.off
    c1 = np.maximum(cnt, 1)[:, None].astype(D)
    M = np.zeros((N, P))
    Mabs = np.zeros((N, P))
    dAd_sum = np.zeros((N, P))
    ad_sum = np.zeros((N, P))
    nocancel = np.ones(N, bool)
    dA, dAd = [], []
    for d in range(nd):
        xsv = np.abs(xs[d].astype(D) * s[d].astype(D)[:, None, None])
        da = u * (xsv + np.abs(r64.A[d]))
        dad = r64.Ad[d] * (da / r64.Ac[d] + u)
        dA.append(da)
        dAd.append(dad)
        tt = np.abs(t[d].astype(D))[:, None, None] + 0 * xsv
        for j in range(xs[d].shape[1]):
            al = r64.alive[d][:, j]
            f = idx[d][al, j]
            M[f] += (xsv + tt)[al, j]
            Mabs[f] += np.abs(r64.A[d])[al, j]
            dAd_sum[f] += dad[al, j]
            ad_sum[f] += r64.Ad[d][al, j]
            nocancel[f[t[d][al] < 0]] = False
    dT = (c1 + 3) * u * M / c1
    dT_tight = (c1 + 3) * u * Mabs / c1
    dTd = (dAd_sum + (c1 + 1) * u * ad_sum) / c1
    dsc = dT.mean(-1) + u * r64.sc
    dscd = dTd.mean(-1) + u * r64.scd
    esc, escd = dsc / r64.sc, dscd / r64.scd
    gb = np.zeros(2 * ntot)
    lb = 0.0
    und = 0
    tot = 0
    und_k = np.zeros(ntot, np.int64)
    dw, ls = D(W.dw), D(W.ls)
    sp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(D)  # noqa: E731
    for d in range(nd):
        f = idx[d]
        live = r64.alive[d][..., None] & np.ones(xs[d].shape, bool)
        single = (cnt[f] == 1)[..., None]
        isc, iscd = (1.0 / r64.sc)[f][..., None], (1.0 / r64.scd)[f][..., None]
        z, zd, a, ac = r64.z[d], r64.zd[d], r64.A[d], r64.Ac[d]
        dz = dA[d] + dT[f]
        dzd = dAd[d] + dTd[f]
        und_z = (np.abs(z) <= np.maximum(dz, 2 * sp(a))) & ~single
        und_d = ((np.abs(zd) <= np.maximum(dzd, 2 * sp(r64.Ad[d]))) & ~single) | \
                (np.abs(a - D(CLIP)) <= np.maximum(dA[d], 2 * sp(a)))
        m1 = isc * np.where(single, 0.0, 1.0)
        m2 = dw * iscd / (ac * ac) * np.where(single | (a < D(CLIP)) & ~und_d, 0.0, 1.0)
        e1 = np.where(und_z, 2 * m1, m1 * (esc[f][..., None] + 3 * u))
        e2 = np.where(und_d, 2 * m2, m2 * (escd[f][..., None] + 2 * dA[d] / ac + 6 * u))
        e = np.where(live, e1 + e2, 0.0)
        gb[off[d]:off[d + 1]] = (e * np.abs(xs[d].astype(D))).sum(axis=(1, 2))
        gb[ntot + off[d]:ntot + off[d + 1]] = e.sum(axis=(1, 2))
        el1 = dz * isc + np.abs(z) * isc * (esc[f][..., None] + 3 * u)
        el2 = dzd * iscd + np.abs(zd) * iscd * (escd[f][..., None] + 3 * u)
        lb += float(np.where(live, el1 + dw * el2, 0.0).sum())
        und += int(((und_z | und_d) & live).sum())
        und_k[off[d]:off[d + 1]] = ((und_z | und_d) & live).sum(axis=(1, 2))
        tot += int(live.sum())
    gdata = np.abs(r64.grad - r64.grad_soft)
    grad_bound = 1.05 * (gb * ls / r64.denom + 8 * u * (gdata + np.abs(r64.grad_soft)))
    loss_bound = 1.05 * (ls * lb / r64.denom + 4 * u * abs(float(r64.loss)))
    return SimpleNamespace(T=1.05 * dT, T_tight=1.05 * dT_tight, T_nocancel=nocancel, Td=1.05 * dTd, grad=grad_bound,
                           loss=loss_bound, undecidable=und / max(tot, 1), undecidable_per_snippet=und_k)


def single_rounding_bounds(xs, idx, N, s, r2):
    """How far T, Td of the kernels' arithmetic (A = fma(x, s, t), one rounding) may lie from the two-rounding
    restatement r2 = one_iteration(..., np.float32) of the same state.  Per term the two are roundings of values
    that differ by the product's rounding, ≤ u·|x·s|: |Δa_i| ≤ δ_i = u·|x_i·s_i| + ulp(a_i) — one ulp of A where
    nothing cancels (t ≥ 0), more where x·s ≈ −t.  That does NOT make T agree to 1 ulp of T: the c terms'
    differences add, T can be small where the terms cancel, and 1/max(A, 1e-3) amplifies a relative step of A.
    What follows is |ΔT| ≤ (Σ_i δ_i + 2·(c + 1)·u·Σ_i|a_i|)/c (the c adds and the division round on both sides)
    and, with ad = 1/ac, |ΔTd| ≤ (Σ_i ad_i·(δ_i/ac_i + 2u) + 2·(c + 1)·u·Σ_i ad_i)/c; ×1.05 for second-order
    terms.  `delta` returns the δ_i per dilation."""
    u = U32
    D = np.float64
    P = r2.T.shape[1]
    sa, su, sd, sdu = (np.zeros((N, P)) for _ in range(4))
    delta = []
    for d in range(len(idx)):
        a = np.abs(r2.A[d].astype(D))
        ulp = np.spacing(np.abs(r2.A[d])).astype(D) + u * np.abs(xs[d].astype(D) * s[d].astype(D)[:, None, None])
        delta.append(ulp)
        ad, ac = r2.Ad[d].astype(D), r2.Ac[d].astype(D)
        for j in range(idx[d].shape[1]):
            al = r2.alive[d][:, j]
            f = idx[d][al, j]
            sa[f] += a[al, j]
            su[f] += ulp[al, j]
            sd[f] += ad[al, j]
            sdu[f] += (ad * (ulp / ac + 2 * u))[al, j]
    c = np.maximum(r2.cnt, 1)[:, None].astype(D)
    return SimpleNamespace(T=1.05 * (su + 2 * (c + 1) * u * sa) / c, Td=1.05 * (sdu + 2 * (c + 1) * u * sd) / c,
                           delta=delta)


# ------------------------------------------------------------------------------------------------- cases
def make_case(P, N=7, dilations=(1, 2), lengths=(3, 3), start_steps=(1, 1), seed=0):
    """Prepared aligner inputs as tests/test_aligner_gpu.py::_synth makes them (frames, per-snippet scale and
    shift, 0.01 noise), at P subsampled pixels, min-shifted so x ≥ 0; and a start state s ~ U[0.6, 1.6],
    t ~ N(0, 0.2²)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (N, P)).astype(np.float32)
    idx = [snippet_index(N, w, d, ss) for d, w, ss in zip(dilations, lengths, start_steps)]
    xs = []
    for ix in idx:
        n = ix.shape[0]
        sc = 0.5 + rng.uniform(0, 1, (n, 1, 1))
        sh = 0.3 * rng.standard_normal((n, 1, 1))
        xs.append((base[ix] * sc + sh + 0.01 * rng.standard_normal(base[ix].shape)).astype(np.float32))
    mn = min(x.min() for x in xs)
    xs = [(x - mn).astype(np.float32) for x in xs]
    s = [rng.uniform(0.6, 1.6, ix.shape[0]).astype(np.float32) for ix in idx]
    t = [(0.2 * rng.standard_normal(ix.shape[0])).astype(np.float32) for ix in idx]
    return SimpleNamespace(P=P, N=N, dilations=list(dilations), lengths=list(lengths), start_steps=list(start_steps),
                           idx=idx, xs=xs, s=s, t=t, ntot=sum(ix.shape[0] for ix in idx), seed=seed)


# geometry name → make_case arguments; the seeds are those at which every coverage condition holds
# (tests/test_aligner_step_cpu.py::test_cases_cover_what_they_claim asserts them)
GEOMETRIES = {
    "P7": dict(P=7, seed=0),
    "P8": dict(P=8, seed=0),
    "P36": dict(P=36, seed=0),
    "P2056": dict(P=2056, seed=2),
    "P2500": dict(P=2500, seed=0),
    "P5929": dict(P=5929, seed=1),
    "P9001": dict(P=9001, seed=3),
    "mixed2500": dict(P=2500, lengths=(3, 2), seed=2),
    "strided5929": dict(P=5929, N=11, dilations=(1, 3), start_steps=(2, 3), seed=17),
}
CASES = [(g, w) for g in GEOMETRIES for w in WEIGHT_SETS]
_cache = {}


def get_case(geometry):
    if geometry not in _cache:
        _cache[geometry] = make_case(**GEOMETRIES[geometry])
    return _cache[geometry]


def zero_moments(case):
    return np.zeros(2 * case.ntot, np.float32), np.zeros(2 * case.ntot, np.float32)
