"""Exact device quantiles (rdmi_quantiles: a radix select over an order-preserving key) against the numpy
reference of tests/quantile_util.py — bitwise, no tolerance — the clipped renormalisation, the split
(histogram-summing) form, and renorm_percentiles / percentiles through RollingDepthPipeline.forward,
shard.sharded_forward and colorize_depth_multi_thread.

Sizes: 1, 2, 63, 64, 65 (around one wave), 255 (under one workgroup), 1027 (several workgroups, a scalar tail in both
dtypes) and BIG = 2048 · 256 · 8 + 1027: the counting grid is capped at 2048 workgroups of 256 lanes that take 8 halves
(4 floats) per step, so at BIG the grid-stride loop runs twice for f16 and three times for f32, with a tail."""
import json
import os
import socket

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from tests import quantile_util as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")

BIG = 2048 * 256 * 8 + 1027
SIZES = [1, 2, 63, 64, 65, 255, 1027, BIG]
KINDS = ["normal", "offset", "equal", "two", "lastdigit", "salted"]
QS = [0.0, 0.02, 0.5, 0.98, 1.0]
DTYPES = {"f32": (np.float32, torch.float32), "f16": (np.float16, torch.float16)}


def _data(kind, n, nm):
    """One input as a numpy array of the case's dtype."""
    npdt = DTYPES[nm][0]
    rng = np.random.default_rng(n % 100003 + 17 * KINDS.index(kind))
    if kind in ("normal", "offset"):
        return (rng.standard_normal(n) * 3).astype(npdt)
    if kind == "equal":
        return np.full(n, 1.25, npdt)
    if kind == "two":  # half 0.5, half 0.75 (shuffled): the median's rank lies at the boundary of two long runs
        x = np.where(np.arange(n) < (n + 1) // 2, 0.5, 0.75).astype(npdt)
        rng.shuffle(x)
        return x
    if kind == "lastdigit":  # one bin in every pass but the one that holds the lowest mantissa bits of the dtype
        if nm == "f32":
            return (np.uint32(0x3F800000) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
        return (np.uint16(0x3C00) | rng.integers(0, 8, n).astype(np.uint16)).view(np.float16)
    x = (rng.standard_normal(n) * 3).astype(npdt)  # salted
    tiny = np.finfo(npdt).smallest_subnormal
    salt = np.array([np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 3 * tiny, np.nan, np.nan, -np.nan], npdt)
    reps = max(1, n // 40)
    pos = rng.permutation(n)[:min(n, reps * len(salt))]
    x[pos] = np.tile(salt, reps)[:len(pos)]
    return x


def _to_dev(x, offset):
    """x on the device; offset: in a buffer that starts one element into an allocation (off the 16-byte grid)."""
    t = torch.from_numpy(x)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(x.size + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 == x.itemsize
    return v


def _same(got: torch.Tensor, want: np.ndarray, what=""):
    """NaN where the reference is NaN, bitwise equal elsewhere."""
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, (what, g.dtype, g.shape)
    assert np.array_equal(np.isnan(g), np.isnan(want)), (what, g, want)
    ok = ~np.isnan(want)
    assert np.array_equal(g[ok].view(np.uint32), want[ok].view(np.uint32)), (what, g, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nm", list(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_quantiles_equal_the_reference(n, nm, kind):
    """Four fractions at a time (two groups that cover all five) and each singly: every value bitwise the
    reference's.  The result is always one of the data values (or +0 for −0)."""
    from rollingdepth_amd import kernels as K

    x = _data(kind, n, nm)
    xd = _to_dev(x, kind == "offset")
    want = Q.select(x, QS)
    if kind == "equal":
        assert (want == 1.25).all()
    if kind == "two" and n >= 2:
        assert want[0] == 0.5 and want[-1] == 0.75
    if kind == "salted" and n >= 63:
        assert want[0] == -np.inf and want[-1] == np.inf and np.isnan(x).sum() >= 3
    for grp in (QS[:4], QS[1:]):
        _same(K.quantiles(xd, grp), Q.select(x, grp), f"{kind} n {n} {nm} q {grp}")
    for i, q in enumerate(QS):
        _same(K.quantiles(xd, [q]), want[i:i + 1], f"{kind} n {n} {nm} q {q}")
    # a multi-dimensional view of the same data gives the same values
    if n == 1027:
        _same(K.quantiles(xd[:1026].view(2, 27, 19), QS[1:]), Q.select(x[:1026], QS[1:]))


_MASKED = [(n, nm, off) for n in (1, 65, 1027) for nm in DTYPES for off in (False, True)] + \
          [(BIG, "f32", False), (BIG, "f16", True)]


@pytest.mark.parametrize("n,nm,offset", _MASKED)
def test_quantiles_with_masks(n, nm, offset):
    """A random mask as bool and as uint8 with values other than 1, an all-false mask (NaN) and a mask with exactly
    one true.  offset: the data starts one element off the 16-byte grid; the bool mask then stays aligned, so behind
    the scalar head its bytes are off their grid and are read one by one, while the uint8 mask is offset with the
    data and is read in whole words again."""
    from rollingdepth_amd import kernels as K

    x = _data("salted", n, nm)
    xd = _to_dev(x, offset)
    rng = np.random.default_rng(n + 5)
    m = rng.random(n) < 0.4
    md = _to_dev(m, False)
    assert md.dtype == torch.bool
    _same(K.quantiles(xd, QS[:4], mask=md), Q.select(x, QS[:4], m), f"random mask n {n} {nm}")
    m8 = (m * rng.integers(1, 256, n)).astype(np.uint8)
    _same(K.quantiles(xd, QS[1:], mask=_to_dev(m8, offset)), Q.select(x, QS[1:], m), f"uint8 mask n {n} {nm}")
    none = K.quantiles(xd, QS[:4], mask=torch.zeros(n, dtype=torch.bool, device=DEV))
    assert torch.isnan(none).all() and none.shape == (4,)
    one = np.zeros(n, bool)
    keep = int(np.flatnonzero(~np.isnan(x.astype(np.float32)))[-1]) if (~np.isnan(x.astype(np.float32))).any() else 0
    one[keep] = True
    want = Q.select(x, [0.0, 0.5, 1.0], one)
    _same(K.quantiles(xd, [0.0, 0.5, 1.0], mask=_to_dev(one, offset)), want, f"one true n {n} {nm}")
    if not np.isnan(want[0]):
        assert want[0] == want[1] == want[2] == np.float32(x[keep]) + np.float32(0)


def test_quantiles_of_nothing_and_of_nans():
    from rollingdepth_amd import kernels as K

    assert torch.isnan(K.quantiles(torch.empty(0, device=DEV), [0.0, 1.0])).all()
    assert torch.isnan(K.quantiles(torch.full((300,), float("nan"), device=DEV), [0.5])).all()
    x = torch.tensor([float("nan"), -0.0, float("nan")], device=DEV)
    got = K.quantiles(x, [0.0, 1.0]).cpu().numpy()
    assert got.view(np.uint32).tolist() == [0, 0]  # −0 comes back as +0


# ------------------------------------------------------------------------------------------------ renormalize_clip_
@pytest.mark.parametrize("n", [1027, 70001])
def test_renormalize_clip(n):
    """Handed minmax it is renormalize_ bitwise; with an inner range it is the numpy restatement in f32, every
    output in [−1, 1] and both ends attained."""
    from rollingdepth_amd import kernels as K

    x = _data("normal", n, "f32")
    xd = torch.from_numpy(x).to(DEV)
    mm = K.minmax(xd)
    a, b = K.renormalize_(xd.clone(), mm), K.renormalize_clip_(xd.clone(), mm)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    lohi = K.quantiles(xd, [0.02, 0.98])
    lo, hi = Q.select(x, [0.02, 0.98])
    assert lohi.cpu().numpy().tolist() == [lo, hi] and x.min() < lo < hi < x.max()
    got = K.renormalize_clip_(xd.clone(), lohi).cpu().numpy()
    want = Q.renorm_clip(x, lo, hi)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.min() == -1.0 and got.max() == 1.0
    assert (got == -1.0).sum() >= int(0.02 * n) and (got == 1.0).sum() >= int(0.02 * n) - 1


# ------------------------------------------------------------------------------------------------ split form
@pytest.mark.parametrize("nm", list(DTYPES))
def test_split_form_sums_histograms_of_uneven_chunks(nm):
    """The sharded form on one device: three uneven chunks, one of them empty, select_hist per chunk into its own
    histogram, the histograms summed with torch, one select_pick per pass — bitwise kernels.quantiles of the whole
    (and the reference)."""
    from rollingdepth_amd import kernels as K

    n = 40001
    x = _data("salted", n, nm)
    xd = torch.from_numpy(x).to(DEV)
    chunks = [xd[:1027], xd[1027:1027], xd[1027:]]
    assert [c.numel() for c in chunks] == [1027, 0, n - 1027]
    q = QS[1:]
    k = len(q)
    qd, state = K.select_q(q, DEV), K.select_state(DEV)
    out = torch.full((k,), 7.0, device=DEV)
    for p in range(K.select_passes()):
        hs = []
        for c in chunks:
            h = torch.zeros((k, K.select_bins()), dtype=torch.int64, device=DEV)
            hs.append(K.select_hist(c, state, p, k, h))
        total = torch.stack(hs).sum(0)
        assert not hs[1].any()
        if p == 0:  # pass 0 counts every kept element, for every quantile
            assert total.sum(1).tolist() == [int((~np.isnan(x.astype(np.float32))).sum())] * k
        K.select_pick(total, qd, p, k, state, out)
    whole = K.quantiles(xd, q)
    assert torch.equal(out.view(torch.int32), whole.view(torch.int32))
    _same(out, Q.select(x, q))


# ------------------------------------------------------------------------------------------------ pipeline
class _Spy:
    """Records, while active, the tensors handed to kernels.minmax / quantiles (clones) and to scale_spread_."""
    NAMES = ("minmax", "quantiles", "scale_spread_", "renormalize_", "renormalize_clip_")

    def __enter__(self):
        from rollingdepth_amd import kernels as K

        self.K, self.calls, self.args = K, [], {n: [] for n in self.NAMES}
        self.orig = {n: getattr(K, n) for n in self.NAMES}

        def wrap(name):
            def f(*a, **kw):
                self.calls.append(name)
                self.args[name].append(tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in a))
                return self.orig[name](*a, **kw)
            return f

        for n in self.NAMES:
            setattr(K, n, wrap(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.K, n, f)
        return False


_PIPES = {}


def _fixture_pipe(name, snippet_batch=8):
    if name not in _PIPES:
        from rollingdepth_amd.pipeline import RollingDepthPipeline

        t = load_file(os.path.join(G, name + ".safetensors"))
        meta = json.load(open(os.path.join(G, name + ".json")))
        pipe = RollingDepthPipeline.from_synthetic(meta["unet"], meta["vae"], meta["scheduler"], device="cuda")
        pipe.empty_text_embed = t["context"]
        _PIPES[name] = (t, meta, pipe)
    t, meta, pipe = _PIPES[name]
    pipe.snippet_batch = snippet_batch
    return t, meta, pipe


def _forward(pipe, t, meta, refine_step, **kw):
    return pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], [1], None, refine_step,
                        3, meta.get("refine_start_dilation", 6), None, False, 4, False, init_noise=t["init_noise"], **kw)


def test_forward_full_range_reproduces_the_default():
    """renorm_percentiles=(0, 100): ranks 0 and count − 1 are the min and the max, so depth_pred, depth_coaligned
    and depth_uncertainty are bitwise the default call's — through the quantile and clip kernels, not through
    minmax / renormalize_."""
    t, meta, pipe = _fixture_pipe("tiny_pipeline")
    with _Spy() as s0:
        base = _forward(pipe, t, meta, 0, output_uncertainty=True)
    assert "quantiles" not in s0.calls and "renormalize_clip_" not in s0.calls and "renormalize_" in s0.calls
    with _Spy() as s1:
        out = _forward(pipe, t, meta, 0, output_uncertainty=True, renorm_percentiles=(0.0, 100.0))
    assert s1.calls.count("quantiles") == 1 and s1.calls.count("renormalize_clip_") == 1
    assert "renormalize_" not in s1.calls
    for name in ("depth_pred", "depth_coaligned", "depth_uncertainty"):
        a, b = getattr(out, name), getattr(base, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert all(torch.equal(a, b) for a, b in zip(out.snippet_ls, base.snippet_ls))


def test_forward_percentile_range():
    """renorm_percentiles=(2, 98) on tiny_pipeline.  The map handed to kernels.quantiles is the merged map the
    default call hands to minmax (bitwise); depth_coaligned is the restatement — reference quantiles, then the f32
    renormalisation and clamp of quantile_util — of that map, cast to the pipeline dtype; −1 and +1 are both
    attained; snippet_ls is untouched.
    depth_uncertainty: default u0 = fl(fl(s / r0) · 2) and here u1 = fl(fl(s / r1) · 2) with r0 = fl(max − min),
    r1 = fl(v_hi − v_lo).  The doubling is exact and each division has relative error ≤ 2⁻²⁴, so
    |u1 − u0 · r0 / r1| ≤ u0 · (r0 / r1) · (2⁻²³ + 2⁻⁴⁶), plus half a denormal step (2⁻¹⁵⁰) where a quotient is
    subnormal."""
    t, meta, pipe = _fixture_pipe("tiny_pipeline")
    with _Spy() as s0:
        base = _forward(pipe, t, meta, 0, output_uncertainty=True)
    with _Spy() as s1:
        out = _forward(pipe, t, meta, 0, output_uncertainty=True, renorm_percentiles=(2.0, 98.0))
    merged = s1.args["quantiles"][0][0]
    assert s1.args["quantiles"][0][1] == [0.02, 0.98]
    merged0 = [a[0] for a in s0.args["minmax"] if a[0].shape == merged.shape][-1]
    assert torch.equal(merged.view(torch.int32), merged0.view(torch.int32))
    m = merged.cpu().numpy()
    lo, hi = Q.select(m, [0.02, 0.98])
    assert m.min() < lo < hi < m.max()
    want = torch.from_numpy(Q.renorm_clip(m, lo, hi)).to(pipe.dtype)
    assert out.depth_coaligned.dtype == pipe.dtype and torch.equal(out.depth_coaligned, want)
    assert torch.equal(out.depth_pred, out.depth_coaligned)
    assert out.depth_coaligned.min().item() == -1.0 and out.depth_coaligned.max().item() == 1.0
    assert not torch.equal(out.depth_coaligned, base.depth_coaligned)
    assert all(torch.equal(a, b) for a, b in zip(out.snippet_ls, base.snippet_ls))
    r0 = np.float64(np.float32(m.max()) - np.float32(m.min()))
    r1 = np.float64(np.float32(hi) - np.float32(lo))
    u0 = base.depth_uncertainty.numpy().astype(np.float64)
    u1 = out.depth_uncertainty.numpy().astype(np.float64)
    bound = u0 * (r0 / r1) * (2.0 ** -23 + 2.0 ** -46) + 2.0 ** -150
    err = np.abs(u1 - u0 * (r0 / r1))
    print(f"range {r0:.6f} -> {r1:.6f}; uncertainty error / bound max {np.max(err / bound):.3f}")
    assert out.depth_uncertainty.dtype == torch.float32 and u1.max() > 0 and r1 < r0
    assert (err <= bound).all()


def test_forward_refine_starts_from_the_clipped_map():
    """tiny_refine (refine_step 2): depth_coaligned is the clipped map of the same run without refine, the refine
    stage's depth encode receives exactly that map, and depth_pred is its refinement."""
    t, meta, pipe = _fixture_pipe("tiny_refine")
    base = _forward(pipe, t, meta, meta["refine_step"])
    plain = _forward(pipe, t, meta, 0, renorm_percentiles=(2.0, 98.0))
    seen, enc = [], pipe.encode_rgb
    pipe.encode_rgb = lambda x, *a, **kw: (seen.append(x.detach().clone()), enc(x, *a, **kw))[1]
    try:
        refined = _forward(pipe, t, meta, meta["refine_step"], renorm_percentiles=(2.0, 98.0))
    finally:
        del pipe.encode_rgb
    assert torch.equal(refined.depth_coaligned, plain.depth_pred)
    assert refined.depth_coaligned.min().item() == -1.0 and refined.depth_coaligned.max().item() == 1.0
    last = seen[-1].cpu()
    assert last.shape[1] == 3 and all(torch.equal(last[:, c:c + 1], refined.depth_coaligned) for c in range(3))
    assert not torch.equal(refined.depth_pred, refined.depth_coaligned)
    assert not torch.equal(refined.depth_pred, base.depth_pred)


# ------------------------------------------------------------------------------------------------ sharded
def _worker(rank, world, port, res):
    """One of `world` ranks on the one GPU (gloo).  res: [0 … 2] depth_pred_full / depth_coaligned_full /
    depth_uncertainty_full torch.equal to the single-GPU forward(renorm_percentiles=(2, 98))'s, [3] the ranks whose
    chunk has the right shape and that took the histogram path (select_hist / select_pick, no minmax of the map)."""
    import torch.distributed as dist
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.shard import chunk_bounds, sharded_forward

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t, meta, pipe = _fixture_pipe("tiny_pipeline", 3)
    N = t["frames"].shape[0]
    picks, pick = [], K.select_pick
    K.select_pick = lambda *a, **kw: (picks.append(a[2]), pick(*a, **kw))[1]
    try:
        so = sharded_forward(pipe, t["frames"][None].cuda(), list(meta["dilations_in"]), True, 3, None,
                             init_noise=t["init_noise"].cuda(), gather=True, output_uncertainty=True,
                             renorm_percentiles=(2.0, 98.0))
        torch.cuda.synchronize()
    finally:
        K.select_pick = pick
    f0, f1 = chunk_bounds(N, world)[rank]
    H, W = so.depth_pred.shape[-2:]
    ok = torch.tensor([float(tuple(so.depth_coaligned.shape) == (f1 - f0, 1, H, W) and
                             picks == list(range(K.select_passes())))])
    dist.all_reduce(ok)
    dist.barrier()
    if rank == 0:
        pipe.snippet_batch = 8
        out = _forward(pipe, t, meta, 0, output_uncertainty=True, renorm_percentiles=(2.0, 98.0))
        res[0] = float(torch.equal(so.depth_pred_full.cpu(), out.depth_pred))
        res[1] = float(torch.equal(so.depth_coaligned_full.cpu(), out.depth_coaligned))
        res[2] = float(torch.equal(so.depth_uncertainty_full.cpu(), out.depth_uncertainty))
        res[3] = ok.item()
        print(f"tiny_pipeline world {world}: depth_pred / depth_coaligned / depth_uncertainty equal to the "
              f"single-GPU forward's: {res[0]:.0f} {res[1]:.0f} {res[2]:.0f}")
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_forward_percentile_range(world):
    """sharded_forward(renorm_percentiles=(2, 98), output_uncertainty=True) over 2 and 3 ranks on the one GPU
    (collectives over gloo, every child under its own join limit): the full outputs are torch.equal to the
    single-GPU forward's — the summed integer histograms give every rank the single-GPU range."""
    import torch.multiprocessing as mp

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    res = ctx.Array("d", [0.0, 0.0, 0.0, 0.0])
    procs = [ctx.Process(target=_worker, args=(r, world, port, res)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert not any(alive) and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert list(res) == [1.0, 1.0, 1.0, float(world)], list(res)


# ------------------------------------------------------------------------------------------------ colorize
@pytest.mark.parametrize("nm", ["f32", "f16"])
def test_colorize_percentiles(nm):
    """percentiles=(0, 100) is byte-identical to the default call, with and without valid_mask; (2, 98) with a mask
    is the image the colorize kernel gives when handed the reference quantiles of the masked pixels — and not the
    default image."""
    from rollingdepth_amd import colorize as Cz

    t = load_file(os.path.join(G, "colorize.safetensors"))
    d = t[f"depth_{nm}"]
    m = t["mask"].numpy()[:, 0]
    base = Cz.colorize_depth_multi_thread(d.numpy())
    base_m = Cz.colorize_depth_multi_thread(d.numpy(), valid_mask=m)
    assert np.array_equal(Cz.colorize_depth_multi_thread(d.numpy(), percentiles=(0, 100)), base)
    assert np.array_equal(Cz.colorize_depth_multi_thread(d.numpy(), valid_mask=m, percentiles=(0, 100)), base_m)
    # the fixture's depth saturates at ±1 (its 2nd / 98th percentiles are its min / max), so the inner range is
    # checked on it and on a draw without ties, where it must also change the image
    draw = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, tuple(d.shape)).astype(np.float32)).to(d.dtype)
    for dep, changes in ((d, False), (draw, True)):
        dd = dep.cuda().squeeze(1)
        nt = Cz._np_dtype(dd)
        lo, hi = (nt(v) for v in Q.select(dep.numpy()[:, 0], [0.02, 0.98], m.astype(bool)))
        want = Cz._launch(dd, (lo, hi - lo), "Spectral", index=False).cpu().numpy()
        got = Cz.colorize_depth_multi_thread(dep.numpy(), valid_mask=m, percentiles=(2, 98))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        if changes:
            v = dep.numpy()[:, 0][m.astype(bool)]
            assert v.min() < lo < hi < v.max()
            assert not np.array_equal(got, Cz.colorize_depth_multi_thread(dep.numpy(), valid_mask=m))
        lo_a, hi_a = (nt(v) for v in Q.select(dep.numpy()[:, 0], [0.02, 0.98]))
        want_a = Cz._launch(dd, (lo_a, hi_a - lo_a), "Spectral", index=False).cpu().numpy()
        assert np.array_equal(Cz.colorize_depth_multi_thread(dep.cuda(), percentiles=(2.0, 98.0)), want_a)
