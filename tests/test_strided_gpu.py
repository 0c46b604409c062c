"""Snippet strides > 1 on the device: the co-alignment kernels and the merge with snippets that start
every `stride` frames plus the last window (aligner.hip, merge.hip, csrc/aligner_index.h) against the numpy
oracle with the same strided index arrays (itself pinned to a strided run of the reference's
DepthAligner in tests/test_strided_cpu.py), and RollingDepthPipeline.forward with strides."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from oracle import rd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")

# (N, dilations, snippet lengths, start steps)
LAYOUTS = [
    (14, (1, 3), (3, 3), (2, 2)),          # the last window appended for both dilations
    (14, (1, 3), (3, 3), (1, 3)),
    (14, (1, 3), (3, 3), (3, 1)),
    (15, (1, 3), (3, 3), (2, 5)),          # last % step == 0 for dilation 1, appended for dilation 3
    (14, (1, 3), (3, 2), (2, 3)),          # mixed lengths, coinciding rows
    (14, (1, 3, 2), (4, 2, 2), (1, 2, 3)),
    (9, (1, 2), (3, 3), (2, 2)),
    (9, (1, 2), (3, 3), (1, 3)),
    (9, (1, 2), (3, 3), (3, 1)),
    (14, (1, 3), (3, 3), (1, 20)),         # step larger than the range: the first and the last window
]


def _indices(N, dil, lengths, steps):
    return [np.array(O.snippet_indices(0, 1, N, w, d, d, s), np.int64) for d, w, s in zip(dil, lengths, steps)]


def _synth(N, dil, lengths, steps, H=40, W=44, seed=0, dtype=np.float32):
    """tests/test_aligner_gpu.py::_synth with the snippets of the strided index lists."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (N, 1, H, W)).astype(np.float32)
    out = []
    for ix in _indices(N, dil, lengths, steps):
        n = ix.shape[0]
        s = base[ix]  # [n, w, 1, H, W]
        sc = 0.5 + rng.uniform(0, 1, (n, 1, 1, 1, 1))
        sh = 0.3 * rng.standard_normal((n, 1, 1, 1, 1))
        out.append((s * sc + sh + 0.01 * rng.standard_normal(s.shape)).astype(dtype))
    return out


def _oracle_run(snips, idx, N, iters, border=2, factor=10):
    """oracle.aligner_run (DepthAligner.run + merge_scaled_triplets) with explicit index arrays."""
    mn = min(float(s.min()) for s in snips)
    dt = snips[0].dtype
    shifted = [(s - np.asarray(mn, dtype=dt)).astype(dt) for s in snips]
    sub = [s[:, :, :, border:-border, border:-border][..., ::factor, ::factor] for s in shifted]
    xs = [s.reshape(s.shape[0], s.shape[1], -1).astype(np.float32) for s in sub]
    sc, tr, hist = O.aligner_optimize(xs, idx, N, iters=iters)
    return O.aligner_merge(shifted, idx, sc, tr, N), sc, tr, hist


@functools.lru_cache(maxsize=None)
def _case(li, iters):
    """Snippets and the oracle's result of layout li, computed once for both loop modes."""
    N, dil, lengths, steps = LAYOUTS[li]
    snips = _synth(N, dil, lengths, steps)
    return snips, _oracle_run(snips, _indices(N, dil, lengths, steps), N, iters)


def _device_run(snips, dil, steps, N, iters):
    from rollingdepth_amd.aligner import DepthAligner

    al = DepthAligner(device=torch.device(DEV), num_iterations=iters)
    m, s, t, h = al.run([torch.from_numpy(x).to(DEV) for x in snips], list(dil), strides=steps, sequence_length=N)
    torch.cuda.synchronize()
    return m.cpu(), [v.cpu() for v in s], [v.cpu() for v in t], h


@pytest.mark.parametrize("mode", ["0", None], ids=["three_launch", "default_loop"])
@pytest.mark.parametrize("iters", [1, 20])
@pytest.mark.parametrize("li", range(len(LAYOUTS)))
def test_strided_optimize_and_merge_match_oracle(li, iters, mode, monkeypatch):
    """Every layout at 1 and 20 iterations, in the three-launch loop (RDMI_ALIGNER_FUSED=0) and the
    default two-launch loop, with the tolerances of
    tests/test_aligner_gpu.py::test_aligner_optimize_matches_oracle.  (20 iterations: the reference
    and the oracle agree to 5e-7 there on all ten layouts; at 50 the (2, 2) layout has taken the other
    branch of an L1 sign tie.)"""
    if mode is None:
        monkeypatch.delenv("RDMI_ALIGNER_FUSED", raising=False)
    else:
        monkeypatch.setenv("RDMI_ALIGNER_FUSED", mode)
    N, dil, lengths, steps = LAYOUTS[li]
    snips, (ref_m, ref_s, ref_t, ref_h) = _case(li, iters)
    m, s, t, h = _device_run(snips, dil, list(steps), N, iters)
    ds = max(np.abs(s[d].numpy().ravel() - ref_s[d]).max() for d in range(len(dil)))
    dt = max(np.abs(t[d].numpy().ravel() - ref_t[d]).max() for d in range(len(dil)))
    dh = np.abs(np.array(h)[:, 0] / np.array(ref_h)[:, 0] - 1).max()
    dm = np.abs(m.numpy() - ref_m).max()
    print(f"layout {li} iters {iters} mode {mode}: |ds| {ds:.2e} |dt| {dt:.2e} hist rel {dh:.2e} merged {dm:.2e}")
    assert ds < 2e-5 and dt < 2e-5
    np.testing.assert_allclose(np.array(h)[:, 0], np.array(ref_h)[:, 0], rtol=1e-5)
    assert dm < 1e-4


def test_strided_merge_f16_rounding():
    """tests/test_aligner_gpu.py::test_aligner_merge_f16_rounding on layout 1 (both dilations strided,
    the last window appended): f16 snippets in the reference's f16 arithmetic."""
    from rollingdepth_amd import kernels as K

    N, dil, lengths, steps = LAYOUTS[0]
    snips = _synth(N, dil, lengths, steps, seed=1, dtype=np.float16)
    idx = _indices(N, dil, lengths, steps)
    rng = np.random.default_rng(2)
    sc = [(1 + 0.1 * rng.standard_normal(x.shape[0])).astype(np.float32) for x in snips]
    tr = [(0.1 * rng.standard_normal(x.shape[0])).astype(np.float32) for x in snips]
    mn = min(float(x.min()) for x in snips)
    shifted = [(x - np.float16(mn)).astype(np.float16) for x in snips]
    ref = O.aligner_merge(shifted, idx, sc, tr, N)
    xf = [torch.from_numpy(x[:, :, 0]).to(DEV) for x in snips]
    shift = torch.tensor([mn], dtype=torch.float32, device=DEV)
    out = K.aligner_merge(xf, [torch.from_numpy(s).to(DEV) for s in sc], [torch.from_numpy(t).to(DEV) for t in tr],
                          list(dil), N, shift, start_steps=list(steps))
    got = out.half().float().cpu().numpy()
    assert np.abs(got - ref[:, 0].astype(np.float32)).max() <= 2e-3


@pytest.mark.parametrize("mode", [None, "0"], ids=["default_loop", "three_launch"])
def test_explicit_ones_are_bitwise_the_default(mode, monkeypatch):
    """run(…, strides=[1, 1], sequence_length=N) is the call without strides, bit for bit."""
    from rollingdepth_amd.aligner import DepthAligner

    if mode is None:
        monkeypatch.delenv("RDMI_ALIGNER_FUSED", raising=False)
    else:
        monkeypatch.setenv("RDMI_ALIGNER_FUSED", mode)
    N, dil = 14, (1, 3)
    xs = [torch.from_numpy(x).to(DEV) for x in _synth(N, dil, (3, 3), (1, 1))]
    al = DepthAligner(device=torch.device(DEV), num_iterations=140)  # two history blocks
    a = al.run(xs, list(dil))
    b = al.run(xs, list(dil), strides=[1, 1], sequence_length=N)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0])
    for d in range(len(dil)):
        assert torch.equal(a[1][d], b[1][d]) and torch.equal(a[2][d], b[2][d])
    assert a[3] == b[3]
    with pytest.raises(ValueError, match="sequence_length"):
        al.run(xs, list(dil), strides=[1, 1])


def test_strided_2000_iterations_vs_reference_golden():
    """The reference's DepthAligner.optimize + merge_scaled_triplets with strided index tensors
    (aligner_strided fixture: N = 20, 64², dilations (1, 4), strides (2, 3)), with the bounds of
    tests/test_aligner_gpu.py::test_aligner_2000_iterations_vs_reference_golden for its `aligner`
    fixture.  (The oracle holds half of each bound against this fixture, tests/test_strided_cpu.py.)"""
    t = load_file(os.path.join(G, "aligner_strided.safetensors"))
    meta = json.load(open(os.path.join(G, "aligner_strided.json")))
    dil, N = meta["dilations"], meta["N"]
    snips = [t[f"snippet_{i}"].float().numpy() for i in range(len(dil))]
    m, s, tr, h = _device_run(snips, dil, meta["strides"], N, meta["iterations"])
    ref_h = t["loss_hist"].numpy()
    ref_m = t["merged"].numpy()
    rng = ref_m.max() - ref_m.min()
    err = np.abs(m.numpy() - ref_m)
    ds = max(np.abs(s[i].numpy().ravel() - t[f"scale_{i}"].numpy().ravel()).max() for i in range(len(dil)))
    dt = max(np.abs(tr[i].numpy().ravel() - t[f"trans_{i}"].numpy().ravel()).max() for i in range(len(dil)))
    rel = np.abs(np.array(h)[:, 0] / ref_h[:, 0] - 1)
    print(f"aligner_strided: max |Δs| {ds:.2e}, max |Δt| {dt:.2e}, merged mean {err.mean() / rng:.2e} max "
          f"{err.max() / rng:.2e} of the range, history rel {rel[:50].max():.2e} (50 rows) {rel.max():.2e} (all)")
    np.testing.assert_allclose(np.array(h)[:50, 0], ref_h[:50, 0], rtol=1e-5)
    np.testing.assert_allclose(np.array(h)[:, 0], ref_h[:, 0], rtol=2e-3)
    assert ds <= 1e-2 and dt <= 1e-2
    assert err.mean() <= 1e-3 * rng and err.max() <= 5e-3 * rng


def test_wrong_snippet_count_is_rejected():
    """K.aligner_optimize with start step 2 and an n[d] the index map does not give: RdmiError before
    any launch (N = 14, dilation 3, length 3, start step 2: 5 snippets, not 4)."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd._native import RdmiError

    xs = [torch.zeros((n, 3, 9), dtype=torch.float32, device=DEV) for n in (7, 4)]
    sc = [torch.ones(x.shape[0], dtype=torch.float32, device=DEV) for x in xs]
    tr = [torch.zeros(x.shape[0], dtype=torch.float32, device=DEV) for x in xs]
    with pytest.raises(RdmiError, match="gives 5"):
        K.aligner_optimize(xs, sc, tr, [1, 3], 14, 1e-3, (0.5, 0.9), 1e-8, 0.1, 10.0, 1.0, 1.0, 1, None,
                           start_steps=[2, 2])
    assert all(bool((s == 1).all()) for s in sc)


# ----------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def tiny():
    """The tiny_pipeline fixture (9 frames 32², dilations used [1, 2]), its pipeline and the default
    (stride 1) forward, shared by the tests below."""
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    t = load_file(os.path.join(G, "tiny_pipeline.safetensors"))
    meta = json.load(open(os.path.join(G, "tiny_pipeline.json")))
    pipe = RollingDepthPipeline.from_synthetic(meta["unet"], meta["vae"], meta["scheduler"], device="cuda")
    pipe.snippet_batch = 8
    pipe.empty_text_embed = t["context"]

    def run(strides, frames=None, dilations=None, record=None):
        return pipe.forward(t["frames"][None] if frames is None else frames,
                            list(meta["dilations_in"]) if dilations is None else dilations, meta["cap_dilation"],
                            [3], [1], strides, {"num_iterations": 20}, 0, 3, 6, None, False, 4, False,
                            init_noise=t["init_noise"], record=record)

    return t, meta, pipe, run, run([1])


@pytest.mark.parametrize("strides,counts", [([2, 2], [4, 3]), ([1, 3], [7, 3]), ([3, 1], [3, 5])])
def test_pipeline_strides(tiny, strides, counts, monkeypatch):
    t, meta, pipe, run, _ = tiny
    N, dil = 9, meta["dilations_used"]
    captured = []
    infer = pipe.init_snippet_infer

    def spy(*a, **kw):  # the decoded snippets as the aligner receives them (f32 on the device)
        out = infer(*a, **kw)
        captured.append([s.float().cpu().numpy() for s in out])
        return out

    monkeypatch.setattr(pipe, "init_snippet_infer", spy)
    rec = {}
    out = run(list(strides), record=rec)
    assert rec["dilations"] == dil
    assert [s.shape[0] for s in out.snippet_ls] == counts
    idx = _indices(N, dil, [3, 3], strides)
    # each decoded snippet against the reference's stride-1 snippet with the same first frame
    for d in range(len(dil)):
        for i, ix in enumerate(idx[d]):
            err = (out.snippet_ls[d][i].float() - t[f"snippet_{d}"][int(ix[0])]).abs().mean().item()
            assert err <= 1e-3, (d, i, err)  # tests/test_pipeline_gpu.py DEPTH_L1
    # depth_coaligned against the oracle's strided aligner on the device's own decoded snippets,
    # renormalised and rounded to the pipeline's dtype as forward() does
    snips = [s[:, :, None] for s in captured[0]]
    merged, _, _, _ = _oracle_run(snips, idx, N, 20)
    mn, mx = merged.min(), merged.max()
    want = torch.from_numpy((merged - mn) / (mx - mn) * 2 - 1).to(pipe.dtype).float()
    err = (out.depth_coaligned.float() - want).abs().mean().item()
    print(f"strides {strides}: coaligned mean |Δ| {err:.2e}")
    assert out.depth_coaligned.shape == (N, 1, 32, 32)
    assert err <= 1e-4
    assert torch.equal(out.depth_pred, out.depth_coaligned)


@pytest.mark.parametrize("strides", [[1], [1, 1]])
def test_pipeline_unit_strides_are_the_default(tiny, strides):
    t, meta, pipe, run, base = tiny
    out = run(list(strides))
    assert torch.equal(out.depth_pred, base.depth_pred) and torch.equal(out.depth_coaligned, base.depth_coaligned)
    for a, b in zip(out.snippet_ls, base.snippet_ls):
        assert torch.equal(a, b)


def test_pipeline_rejects_uncovered_frames_and_bad_strides(tiny):
    """strides [4] with dilation 1 at 14 frames: snippets start at 0, 4, 8 and 11, frames 3 and 7 are in
    none — refused before any inference (the reference warns and then divides 0 / 0)."""
    t, meta, pipe, run, _ = tiny
    frames = torch.rand((1, 14, 3, 32, 32), generator=torch.Generator().manual_seed(0)) * 2 - 1
    rec = {}
    with pytest.raises(ValueError, match="frame 3"):
        run([4], frames=frames, dilations=[1], record=rec)
    assert rec == {}
    for bad in ([0], [1, -2], [1.5], [True]):
        with pytest.raises(ValueError, match="strides"):
            run(bad, record=rec)
    assert rec == {}
