"""CPU side of the depth-boundary metrics: the new library symbols, the argument checks that run before any launch in
the C entry and before any device work in boundary_metrics, the properties of the f64 restatement
(tests/boundary_util.py) that give the metric its meaning, and the conditions on the GPU test's inputs without which
tests/test_boundary_gpu.py could pass vacuously (no edge met, or every edge met) or fail for a rounding in the last
bit (a pair lying on a threshold)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import boundary_util as B
from tests import upsample_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDMI_E_ARG, RDMI_E_ALIGN = 1001, 1002


def test_new_symbols_declared_bound_and_exported():
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import metrics as M

    hdr = open(os.path.join(ROOT, "include", "rdmi.h")).read()
    assert "Depth boundaries (since rdmi_version 12)" in hdr
    assert "#define RDMI_BOUNDARY_MAX_THRESHOLDS 16" in hdr
    for name in ("rdmi_depth_boundary_workspace", "rdmi_depth_boundary"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in N_.EXPORTED and callable(getattr(N_.lib, name)), name
    assert N_.lib.rdmi_version() >= 12
    assert (K.BOUNDARY_MAX_THRESHOLDS, M.MAX_BOUNDARY_THRESHOLDS) == (16, 16)
    assert os.path.exists(os.path.join(ROOT, "rollingdepth_amd", "csrc", "boundary.hip"))


def test_workspace_size_is_host_arithmetic():
    """Bytes, a function of the shape alone (one row per workgroup, so proportional to N), 0 for refused arguments."""
    from rollingdepth_amd import _native as N_

    ws = N_.lib.rdmi_depth_boundary_workspace
    assert ws(1, 1, 1, 1) > 0 and ws(1, 1, 1, 1) % 16 == 0
    assert ws(3, 70, 131, 10) == 3 * ws(1, 70, 131, 10) == 3 * ws(1, 70, 131, 16)
    assert ws(1, 1080, 1920, 10) > ws(1, 768, 768, 10) > ws(1, 8, 8, 10)
    for bad in ((0, 4, 4, 10), (1, 0, 4, 10), (1, 4, 0, 10), (1, 4, 4, 0), (1, 4, 4, 17)):
        assert ws(*bad) == 0, bad


def _call(**over):
    """One call of the C entry with valid arguments except for what `over` replaces.  The device pointers are dummies
    that are never dereferenced — every call below is refused before a launch; the thresholds are a real host array,
    which the entry reads."""
    from rollingdepth_amd import _native as N_

    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    tau = over.pop("tau", [1.05, 1.15, 1.25])
    arr = (ctypes.c_double * max(len(tau), 1))(*tau)
    a = dict(pred=p, pred_dtype=N_.RDMI_F16, target=p, target_dtype=N_.RDMI_F32, mask=None, N=2, H=3, W=4, lo=1e-3,
             hi=math.inf, st=p, space=N_.RDMI_SPACE_DEPTH, clip_lo=-math.inf, clip_hi=math.inf,
             thresholds=ctypes.addressof(arr), M=len(tau), counts=p, pairs=p, edges=None, edge_index=0, workspace=p,
             stream=None)
    a.update(over)
    rc = N_.lib.rdmi_depth_boundary(*a.values())
    return rc, N_.lib.rdmi_last_error().decode()


def test_library_checks_run_before_any_launch():
    """Every rejected argument gets one call, on a machine without a GPU: nothing can have been launched."""
    from rollingdepth_amd import _native as N_

    nan, inf = math.nan, math.inf
    edges = ctypes.addressof(ctypes.create_string_buffer(64))
    bad = [dict(pred=None), dict(target=None), dict(st=None), dict(thresholds=None), dict(counts=None),
           dict(pairs=None), dict(workspace=None),
           dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-3), dict(W=-1),
           dict(pred_dtype=N_.RDMI_U8), dict(target_dtype=N_.RDMI_U8), dict(pred_dtype=7), dict(target_dtype=-1),
           dict(space=3), dict(space=-1),
           dict(lo=1.0, hi=1.0), dict(lo=nan),
           dict(clip_lo=2.0, clip_hi=1.0), dict(clip_lo=nan), dict(clip_hi=nan),
           dict(M=0), dict(M=-1), dict(M=17, tau=[1.0 + 0.01 * (i + 1) for i in range(17)]),
           dict(tau=[1.05, inf]), dict(tau=[nan]), dict(tau=[1.05, nan, 1.25]),
           dict(tau=[1.0]), dict(tau=[0.5, 1.2]), dict(tau=[-2.0]),
           dict(tau=[1.1, 1.1]), dict(tau=[1.2, 1.1]), dict(tau=[1.05, 1.25, 1.15]),
           dict(edges=edges, edge_index=-1), dict(edges=edges, edge_index=3), dict(edges=edges, edge_index=16)]
    for kw in bad:
        rc, msg = _call(**dict(kw))
        assert rc == RDMI_E_ARG and "depth_boundary" in msg, (kw, rc, msg)
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    for off in (1, 4, 8):
        rc, msg = _call(workspace=p + off)
        assert rc == RDMI_E_ALIGN and "depth_boundary" in msg, (off, rc, msg)


def test_boundary_metrics_checks_come_before_any_device_work():
    import rollingdepth_amd
    from rollingdepth_amd import metrics as M

    assert rollingdepth_amd.boundary_metrics is M.boundary_metrics
    assert rollingdepth_amd.BoundaryMetrics is M.BoundaryMetrics
    sig = inspect.signature(M.boundary_metrics).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [
        ("mask", None), ("align", "video"), ("space", "depth"), ("valid_range", (1e-3, math.inf)), ("clip", None),
        ("thresholds", None), ("return_edges", False), ("edge_threshold", None)]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in list(sig.items())[3:])
    assert np.array_equal(np.array(M.DEFAULT_BOUNDARY_THRESHOLDS), np.linspace(1.05, 1.25, 10))
    assert [f for f in M.BoundaryMetrics.__dataclass_fields__] == [
        "f1", "precision", "recall", "f1_per_threshold", "precision_per_threshold", "recall_per_threshold",
        "thresholds", "counts", "pairs", "n_pairs", "scale", "shift", "frames_skipped", "edges"]
    assert "pixel-exact" in M.boundary_metrics.__doc__

    d = torch.ones(2, 4, 5)
    ok = dict(pred=d, target=d)
    type_errors = [(dict(pred=d.numpy()), "pred"), (dict(pred=d.double()), "pred"), (dict(target=d.int()), "target"),
                   (dict(target=None), "target"), (dict(mask=d), "mask"), (dict(mask=d.numpy() > 0), "mask"),
                   (dict(thresholds=1.1), "thresholds"), (dict(thresholds=["1.1"]), "thresholds"),
                   (dict(thresholds=[True]), "thresholds"), (dict(return_edges=1), "return_edges"),
                   (dict(edge_threshold="1.05"), "edge_threshold"), (dict(edge_threshold=True), "edge_threshold")]
    for kw, word in type_errors:
        with pytest.raises(TypeError, match=word):
            M.boundary_metrics(**dict(ok, **kw))
    inf, nan = math.inf, math.nan
    value_errors = [(dict(align="both"), "align"), (dict(space="inverse"), "space"), (dict(clip=(2.0, 1.0)), "clip"),
                    (dict(clip=(nan, 1.0)), "clip"), (dict(space="disparity"), "finite upper clip"),
                    (dict(space="disparity", clip=(0.1, inf)), "finite upper clip"),
                    (dict(pred=d[0]), "pred"), (dict(target=d[:, :3]), "target"), (dict(mask=d[:1] > 0), "mask"),
                    (dict(pred=d[:, :0], target=d[:, :0]), "empty"), (dict(valid_range=(1.0, 1.0)), "valid_range"),
                    (dict(thresholds=[]), "thresholds"), (dict(thresholds=[1.01 + 0.01 * i for i in range(17)]), "1 to 16"),
                    (dict(thresholds=[1.0]), "> 1"), (dict(thresholds=[0.9, 1.1]), "> 1"),
                    (dict(thresholds=[1.1, nan]), "finite"), (dict(thresholds=[1.1, inf]), "finite"),
                    (dict(thresholds=[1.1, 1.1]), "increasing"), (dict(thresholds=[1.2, 1.1]), "increasing"),
                    (dict(edge_threshold=1.06), "edge_threshold"),
                    (dict(thresholds=[1.1, 1.2], edge_threshold=1.05), "edge_threshold")]
    for kw, word in value_errors:
        with pytest.raises(ValueError, match=word):
            M.boundary_metrics(**dict(ok, **kw))
    assert M._boundary_thresholds(None, None) == (list(M.DEFAULT_BOUNDARY_THRESHOLDS), 5)
    assert M._boundary_thresholds([1.1, 1.2, 1.3], 1.3) == ([1.1, 1.2, 1.3], 2)
    assert M._boundary_thresholds(torch.tensor([1.5]), None) == ([1.5], 0)


def test_pooling_on_the_host_is_the_restatements():
    """metrics._pool_boundary and boundary_util.pool are two writings of the same f64 arithmetic on the same integers:
    equal bit for bit on the counts of a GPU case, NaN without a pair."""
    from rollingdepth_amd import metrics as M

    (counts, pairs, _, _), (s, t) = B.restate_case(13)
    tau = B.case_inputs(13)[3]["thresholds"]
    got = M._pool_boundary(torch.from_numpy(counts), torch.from_numpy(pairs), tau, torch.from_numpy(s),
                           torch.from_numpy(t), None)
    want = B.pool(counts, pairs, tau)
    for k in ("f1", "precision", "recall", "n_pairs"):
        assert getattr(got, k) == want[k], k
    for k in ("f1_per_threshold", "precision_per_threshold", "recall_per_threshold"):
        assert getattr(got, k).tolist() == want[k], k
    assert got.frames_skipped == [1] and got.thresholds.tolist() == tau and got.edges is None
    assert 0.0 < got.f1 < 1.0
    none = M._pool_boundary(torch.zeros((1, 2, 4, 3), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int64),
                            [1.1, 1.2], torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), None)
    assert none.n_pairs == 0 and all(math.isnan(v) for v in (none.f1, none.precision, none.recall))
    assert all(math.isnan(v) for v in none.f1_per_threshold.tolist() + none.recall_per_threshold.tolist())


# ----------------------------------------------------------------------------- what the restatement says
ONE, ZERO = np.ones(8), np.zeros(8)


def _score(pred, target, **kw):
    N = pred.shape[0]
    counts, pairs, edges, _ = B.restate(pred, target, None, kw.pop("s", ONE[:N]), ZERO[:N], **kw)
    return counts, pairs, edges, B.pool(counts, pairs, kw.get("thresholds", B.DEFAULT_THRESHOLDS))


def test_prediction_equal_to_the_target_scores_one_wherever_an_edge_exists():
    """TP = NP = NG in every cell; a direction's term TP / max(N, 1) is 1 where it has an edge and 0 where it has
    none, so the pooled precision = recall = f1 is the share of directions with an edge: exactly 1.0 for a scene with
    edges in all four (the rectangles of the GPU cases), ¼ for the single vertical step of the upsampling tests."""
    gt, _ = B.scene((3, 17, 67), 1)
    counts, pairs, _, r = _score(gt, gt)
    assert (counts[..., 0] == counts[..., 1]).all() and (counts[..., 0] == counts[..., 2]).all()
    assert (counts.sum(0)[..., 0] > 0).all()
    assert r["f1"] == r["precision"] == r["recall"] == 1.0
    assert r["f1_per_threshold"] == [1.0] * 10
    for ei in range(len(U.EDGE_CASES)):
        truth = (1.0 + U.edge_inputs(ei)[3].numpy())[None]
        counts, _, _, r = _score(truth, truth)
        H = U.EDGE_CASES[ei][2]
        assert (counts[0, :, 0] == H).all() and (counts[0, :, 1:] == 0).all()  # one R edge per row, nothing else
        assert r["f1"] == r["precision"] == r["recall"] == 0.25


def test_a_step_displaced_by_one_pixel_is_a_miss():
    g = np.ones((1, 6, 12))
    g[..., 5:] = 2.0
    p = np.ones((1, 6, 12))
    p[..., 6:] = 2.0
    counts, _, _, r = _score(p, g)
    assert (counts[..., 0] == 0).all()
    assert (counts[0, :, 0, 1] == 6).all() and (counts[0, :, 0, 2] == 6).all()
    assert r["f1"] == r["precision"] == r["recall"] == 0.0


def test_scale_and_symmetries():
    """Multiplying the prediction by 2 changes no count (align none); a horizontal flip swaps R and L, a transpose
    swaps R with D and L with U."""
    gt, pr = B.scene((2, 5, 7), 1)
    counts, pairs, _, _ = _score(pr, gt)
    assert (counts.sum(0)[..., 0] > 0).any()
    c2, p2, _, _ = _score(2.0 * pr, gt)
    assert np.array_equal(c2, counts) and np.array_equal(p2, pairs)
    cf, pf, _, _ = _score(pr[..., ::-1].copy(), gt[..., ::-1].copy())
    assert np.array_equal(cf, counts[:, :, [1, 0, 2, 3]]) and np.array_equal(pf, pairs)
    ct, pt, _, _ = _score(pr.transpose(0, 2, 1).copy(), gt.transpose(0, 2, 1).copy())
    assert np.array_equal(ct, counts[:, :, [2, 3, 0, 1]]) and np.array_equal(pt, pairs[:, ::-1])


def test_targets_at_or_below_zero_follow_the_definition():
    """With lo < 0 in depth space a valid target may be ≤ 0; the test d(j) > τ·d(i) is then taken as written, and the
    thresholds at which a pair is an edge need not be the lowest ones: looking left from −1 at −1.1, −1.1 > τ·(−1)
    holds only for τ > 1.1.  R edges of the row below: at pixels 0, 1 and 3 for every τ; L edges: at pixel 5 for every
    τ and at pixel 1 from the second threshold on."""
    g = np.array([[[-1.1, -1.0, 0.0, 0.0, 2.0, -3.0]]])
    p = np.ones_like(g)
    tau = [1.05, 1.1 + 1e-12, 1.25]
    counts, pairs, _, _ = B.restate(p, g, None, ONE[:1], ZERO[:1], tau, lo=-10.0)
    assert pairs.tolist() == [[5, 0]]
    assert counts[0, :, 0, 2].tolist() == [3, 3, 3] and counts[0, :, 1, 2].tolist() == [1, 2, 2]
    assert (counts[..., :2] == 0).all()


@pytest.mark.parametrize("ei", range(len(U.EDGE_CASES)))
def test_ramp_against_joint_bilateral_on_the_restatement(ei):
    """Depth 1 + side of upsample_util.edge_inputs: the truth has one R edge per row.  The restatement of the joint
    bilateral output reproduces the truth's counts exactly — every direction's term is 1 where an edge exists, and the
    pooled f1 is the scene's maximum, the ¼ of the truth against itself.  The bilinear ramp spreads the step over
    several pixels: NP exceeds NG at the lowest threshold in all three cases (precision lost), and in cases 1 and 2 the
    ramp's step at the truth's contour falls below the upper thresholds, so recall there drops to 0; in case 0 that
    step stays above 1.25 and recall is kept.  Measured f1: bilinear 0.134, 0.111, 0.060 against 0.25."""
    values, guide_lo, guide_hi, side = U.edge_inputs(ei)
    h, w, H, W, X0 = U.EDGE_CASES[ei]
    truth = (1.0 + side.numpy())[None]
    c_self, _, _, r_self = _score(truth, truth)
    jb = 1.0 + U.restate(values, guide_lo, guide_hi, 2)[0].numpy()
    c_jb, _, _, r_jb = _score(jb, truth)
    assert np.array_equal(c_jb, c_self)
    assert r_jb["f1"] == r_self["f1"] == 0.25 and r_jb["recall_per_threshold"] == [0.25] * 10
    bil = Fn.interpolate(1.0 + values.double(), size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    c_bil, _, _, r_bil = _score(bil, truth)
    print(f"edge case {U.EDGE_CASES[ei]}: bilinear f1 {r_bil['f1']:.4f} precision {r_bil['precision']:.4f} recall "
          f"{r_bil['recall']:.4f}; recall per threshold {np.round(r_bil['recall_per_threshold'], 3).tolist()}")
    assert r_bil["f1"] < r_jb["f1"]
    assert c_bil[0, 0, 0, 1] > c_bil[0, 0, 0, 2] and r_bil["precision"] < r_jb["precision"]
    if ei > 0:
        assert r_bil["recall_per_threshold"][-1] == 0.0 < r_bil["recall_per_threshold"][0]
        assert r_bil["recall"] < r_jb["recall"]
    else:
        assert r_bil["recall_per_threshold"] == [0.25] * 10


# ----------------------------------------------------------------------------- the GPU test's inputs
@pytest.mark.parametrize("ci", range(len(B.CASES)), ids=B.IDS)
def test_gpu_case_inputs_are_decisive(ci):
    """With the f64 restatement's own fit: every direction that has pairs meets, at some threshold, edges matched and
    edges unmatched on both sides (0 < TP < min(NP, NG)), and where the aligned value is not the operand itself no
    pair lies within 1e-9 of a threshold — so equal counts on the device are neither vacuous nor at the mercy of the
    last bit of an fma or an exp."""
    (counts, pairs, _, ties), _ = B.restate_case(ci)
    c = B.CASES[ci]
    tot = counts.sum(0)
    ph, pv = pairs.sum(0)
    assert ph + pv > 0
    for k in range(4):
        if (ph if k < 2 else pv) == 0:
            continue
        tp, npred, ngt = tot[:, k, 0], tot[:, k, 1], tot[:, k, 2]
        assert ((tp > 0) & (tp < np.minimum(npred, ngt))).any(), (B.DIRS[k], tot[:, k].tolist())
    if c["align"] != "none" or c["space"] != "depth":
        assert ties == 0, ties
    if c["dead"] is not None:
        assert (counts[c["dead"]] == 0).all() and (pairs[c["dead"]] == 0).all() and (counts.sum() > 0)
