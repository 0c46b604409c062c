"""The optical-flow kernels on the device against tests/flow_util.py's f64 restatement, their bitwise properties, the
end-to-end path through temporal_metrics, and librdmi's own checks of the new entry points."""
import pytest
import torch

from rollingdepth_amd import flow as FL
from tests import flow_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(c, dt) for c in U.GPU_CASES for dt in U.GPU_DTYPES]
IDS = [f"{c[0]}x{c[1]}x{c[2]}-k{c[3]}-r{c[4]}-{U.DT_NAME[dt]}" for c, dt in CASES]


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8).view(-1),
                                                                      b.contiguous().view(torch.uint8).view(-1))


def compare(got_flow, got_bwd, got_valid, ref, what):
    """Flows within U.TOL_PX of the f64 restatement at every pixel; masks equal wherever a flow error of that size
    cannot turn the decision, and at most 0.1 % of the pixels may be undecidable."""
    fw, bw, valid, margin = ref
    df = (got_flow.cpu().double() - fw).abs().max().item()
    db = (got_bwd.cpu().double() - bw).abs().max().item()
    print(f"{what}: max |device - f64 restatement| forward {df:.3e} px, backward {db:.3e} px (allowed {U.TOL_PX:.2e})")
    assert df <= U.TOL_PX and db <= U.TOL_PX, (what, df, db)
    und = torch.stack([U.undecidable(fw[i], bw[i], margin[i], U.FB_TOL[0], U.TOL_PX) for i in range(fw.shape[0])])
    gv = got_valid.cpu()
    assert gv.dtype == torch.uint8 and gv.max() <= 1
    wrong = ((gv != 0) != valid) & ~und
    print(f"{what}: {int(und.sum())} of {und.numel()} pixels undecidable, valid share {valid.double().mean():.3f}")
    assert not wrong.any(), (what, int(wrong.sum()))
    assert und.double().mean().item() <= 1e-3, (what, int(und.sum()))


@pytest.mark.parametrize("case,dtype", CASES, ids=IDS)
def test_device_against_the_restatement(case, dtype):
    N, H, W, k, r = case
    frames = U.gpu_video(case, dtype)
    res = FL.optical_flow(frames.to(DEV), k, radius=r)
    assert res.levels == U.level_rule(H, W, r)
    assert res.flow.shape == (N - k, H, W, 2) and res.flow.dtype == torch.float32 and res.valid.shape == (N - k, H, W)
    compare(res.flow, res.flow_backward, res.valid, U.gpu_reference(case, dtype), f"{case} {U.DT_NAME[dtype]}")


def test_three_levels_on_the_accuracy_case():
    """96 × 128 at r = 5 through three levels — one more than the level rule grants, so through the kernel-level
    chain, which takes the count as given — and the accuracy the specification has there."""
    from rollingdepth_amd import kernels as K

    case = U.GPU_CASES[-1]
    frames = U.gpu_video(case, U.F32)
    flow, bwd, valid = K.flow_estimate(frames.to(DEV), 1, U.ACC_LEVELS)
    compare(flow, bwd, valid, U.gpu_reference(case, U.F32, U.F64, U.ACC_LEVELS), "96 x 128, three levels")
    truth = U.true_flow(96, 128, U.ACCURACY_CASES[0][0], 1.0)
    e = U.interior(U.epe(flow.cpu(), truth)[0])
    assert e.mean() <= 0.05 and e.max() <= 0.25, (e.mean(), e.max())
    assert U.interior(valid[0].cpu()).all()
    # a request above the rule is clamped by the public function: two levels, the bits of levels=None
    a, b = FL.optical_flow(frames.to(DEV), levels=3), FL.optical_flow(frames.to(DEV))
    assert a.levels == b.levels == 2 and bits(a.flow, b.flow) and bits(a.valid, b.valid)
    assert not bits(a.flow, flow)


def test_split_form_equals_the_chain():
    from rollingdepth_amd import kernels as K

    case = U.GPU_CASES[1]  # 33 × 31 at r = 1: two levels
    N, H, W, k, r = case
    x = U.gpu_video(case, U.F16).to(DEV)
    flow, bwd, valid = K.flow_estimate(x, k, 2, r)
    pyr = K.flow_pyramid(x, 2)
    assert [tuple(p.shape) for p in pyr] == [(N, 33, 31), (N, 17, 16)]
    got = []
    for f0, f1 in ((0, k), (k, 0)):
        c = K.flow_lk_level(pyr[1], f0, f1, N - k, None, r)
        got.append(K.flow_lk_level(pyr[0], f0, f1, N - k, c, r))
    assert bits(got[0], flow) and bits(got[1], bwd) and bits(K.flow_fb_check(got[0], got[1]), valid)
    only = FL.optical_flow(x, k, radius=r, backward=False)
    assert only.flow_backward is None and only.valid is None and bits(only.flow, flow)
    Y = U.luma(x.cpu(), U.F64)
    # |luma| < 2: three f32 roundings of at most 2^-24 · 2 each; a level above adds three more to the mean of four
    assert (pyr[0].cpu().double() - Y).abs().max() <= 4e-7 and (pyr[1].cpu().double() - U.down(Y)).abs().max() <= 8e-7


def test_bitwise_properties():
    case = U.GPU_CASES[3]  # three frames of 37 × 45: two pairs, tile remainders both ways
    N, H, W, k, r = case
    x = U.gpu_video(case, U.F32).to(DEV)
    a, b = FL.optical_flow(x), FL.optical_flow(x)
    for name in ("flow", "flow_backward", "valid"):
        assert bits(getattr(a, name), getattr(b, name)), name
    for i in range(N - 1):  # a pair alone is the pair in the batch
        one = FL.optical_flow(x[i:i + 2])
        for name in ("flow", "flow_backward", "valid"):
            assert bits(getattr(one, name)[0], getattr(a, name)[i]), (name, i)
    rev = FL.optical_flow(x.flip(0).contiguous())
    assert bits(rev.flow, a.flow_backward.flip(0)) and bits(rev.flow_backward, a.flow.flip(0))
    # frame_step 2 on five frames: the backward flow of pair i is the forward flow of the reversed video's pair P − 1 − i
    case = U.GPU_CASES[4]
    y = U.gpu_video(case, U.F16).to(DEV)
    a2, rev2 = FL.optical_flow(y, 2), FL.optical_flow(y.flip(0), 2)
    assert bits(rev2.flow, a2.flow_backward.flip(0))


@pytest.mark.parametrize("dtype", U.GPU_DTYPES, ids=[U.DT_NAME[d] for d in U.GPU_DTYPES])
def test_a_view_at_a_storage_offset(dtype):
    case = U.GPU_CASES[1]
    x = U.gpu_video(case, dtype).to(DEV)
    buf = torch.empty(x.numel() + 3, dtype=x.dtype, device=DEV)
    view = buf[3:].view(x.shape)
    view.copy_(x)
    assert view.storage_offset() == 3 and view.data_ptr() % 16 != 0
    a, b = FL.optical_flow(x, radius=1), FL.optical_flow(view, radius=1)
    assert bits(a.flow, b.flow) and bits(a.flow_backward, b.flow_backward) and bits(a.valid, b.valid)
    if dtype != U.U8:  # a channel-last float video is a strided view of the same values
        cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not cl.is_contiguous() and bits(FL.optical_flow(cl, radius=1).flow, a.flow)


def test_end_to_end_through_temporal_metrics():
    from rollingdepth_amd.metrics import temporal_metrics

    frames, depth = U.e2e_inputs()
    frames, depth = frames.to(DEV), depth.to(DEV)
    r = FL.optical_flow(frames)
    a = temporal_metrics(depth, depth, frames=frames)
    b = temporal_metrics(depth, depth, flow=r.flow, pair_mask=r.valid)
    assert torch.equal(a.per_pair.view(torch.int64), b.per_pair.view(torch.int64))
    assert (a.flicker, a.tge, a.n_valid) == (b.flicker, b.tge, b.n_valid)
    plain = temporal_metrics(depth, depth)
    print(f"flicker without a flow {plain.flicker:.5f}, with frames {a.flicker:.5f}: factor {plain.flicker / a.flicker:.1f}")
    assert a.n_valid >= 0.8 * r.valid.numel()
    assert plain.flicker >= 5 * a.flicker
    # a pair_mask of the caller's is ANDed with the estimated mask
    pm = torch.zeros_like(r.valid, dtype=torch.bool)
    pm[:, :, : pm.shape[2] // 2] = True
    c = temporal_metrics(depth, depth, frames=frames, pair_mask=pm)
    d = temporal_metrics(depth, depth, flow=r.flow, pair_mask=pm & (r.valid != 0))
    assert torch.equal(c.per_pair.view(torch.int64), d.per_pair.view(torch.int64)) and 0 < c.n_valid < a.n_valid


def test_library_checks_run_before_any_launch():
    """Every RDMI_E_* check of the five launching entry points, with null, misaligned and out-of-range arguments;
    the dummy pointers are never dereferenced, nothing is launched."""
    from rollingdepth_amd import _native as N_

    lib, x, nan = N_.lib, 4096, float("nan")  # x: a non-null, 16-byte aligned pointer value

    def pyr(**bad):
        a = dict(frames=x, dtype=1, N=2, H=8, W=9, levels=2, pyr=x)
        a.update(bad)
        return lib.rdmi_flow_pyramid(a["frames"], a["dtype"], 216, 72, 9, 1, a["N"], a["H"], a["W"], a["levels"],
                                     a["pyr"], None), lib.rdmi_last_error()

    def lk(**bad):
        a = dict(img=x, N=3, H=8, W=9, f0=0, f1=1, pairs=2, coarse=None, Hc=0, Wc=0, flow=x, r=5, it=3, damping=0.01)
        a.update(bad)
        return lib.rdmi_flow_lk_level(a["img"], a["N"], a["H"], a["W"], a["f0"], a["f1"], a["pairs"], a["coarse"],
                                      a["Hc"], a["Wc"], a["flow"], a["r"], a["it"], a["damping"],
                                      None), lib.rdmi_last_error()

    def fb(**bad):
        a = dict(fwd=x, bwd=x, pairs=2, H=8, W=9, alpha=0.01, beta=0.5, valid=x)
        a.update(bad)
        return lib.rdmi_flow_fb_check(a["fwd"], a["bwd"], a["pairs"], a["H"], a["W"], a["alpha"], a["beta"],
                                      a["valid"], None), lib.rdmi_last_error()

    def est(**bad):
        a = dict(frames=x, dtype=1, N=3, H=8, W=9, k=1, levels=0, r=5, it=3, damping=0.01, backward=1, alpha=0.01,
                 beta=0.5, flow=x, bwd=x, valid=x, ws=x)
        a.update(bad)
        return lib.rdmi_flow_estimate(a["frames"], a["dtype"], 216, 72, 9, 1, a["N"], a["H"], a["W"], a["k"],
                                      a["levels"], a["r"], a["it"], a["damping"], a["backward"], a["alpha"], a["beta"],
                                      a["flow"], a["bwd"], a["valid"], a["ws"], None), lib.rdmi_last_error()

    E_ARG, E_ALIGN, E_UNSUP = 1001, 1002, 1003
    cases = {
        "pyramid null frames": (pyr(frames=None), E_ARG, b"null"), "pyramid null pyr": (pyr(pyr=None), E_ARG, b"null"),
        "pyramid N": (pyr(N=0), E_ARG, b"N (0)"), "pyramid H": (pyr(H=0), E_ARG, b"H (0)"),
        "pyramid W": (pyr(W=-3), E_ARG, b"W (-3)"), "pyramid dtype": (pyr(dtype=3), E_ARG, b"dtype"),
        "pyramid levels 0": (pyr(levels=0), E_ARG, b"levels"), "pyramid levels 6": (pyr(levels=6), E_ARG, b"levels"),
        "pyramid misaligned": (pyr(pyr=x + 2), E_ALIGN, b"aligned"),
        "pyramid too large": (pyr(H=1 << 16, W=(1 << 14) + 1), E_UNSUP, b"2^30"),
        "lk null img": (lk(img=None), E_ARG, b"null"), "lk null flow": (lk(flow=None), E_ARG, b"null"),
        "lk N": (lk(N=0), E_ARG, b"positive"), "lk pairs": (lk(pairs=0), E_ARG, b"positive"),
        "lk H": (lk(H=0), E_ARG, b"H (0)"), "lk W": (lk(W=0), E_ARG, b"W (0)"),
        "lk first0": (lk(f0=-1), E_ARG, b"outside"), "lk first1": (lk(f1=2), E_ARG, b"outside"),
        "lk radius 0": (lk(r=0), E_ARG, b"radius"), "lk radius 8": (lk(r=8), E_ARG, b"radius"),
        "lk iterations": (lk(it=0), E_ARG, b"iterations"), "lk damping": (lk(damping=-1.0), E_ARG, b"damping"),
        "lk nan damping": (lk(damping=nan), E_ARG, b"damping"),
        "lk coarse size": (lk(coarse=x, Hc=4, Wc=4), E_ARG, b"halved"),
        "lk img misaligned": (lk(img=x + 1), E_ALIGN, b"img"), "lk flow misaligned": (lk(flow=x + 4), E_ALIGN, b"flow"),
        "lk coarse misaligned": (lk(coarse=x + 4, Hc=4, Wc=5), E_ALIGN, b"coarse"),
        "lk too many pairs": (lk(N=70000, pairs=65536), E_UNSUP, b"65535 pairs"),
        "lk too large": (lk(H=1 << 15, W=(1 << 15) + 1), E_UNSUP, b"2^30"),
        "fb null fwd": (fb(fwd=None), E_ARG, b"null"), "fb null bwd": (fb(bwd=None), E_ARG, b"null"),
        "fb null valid": (fb(valid=None), E_ARG, b"null"), "fb pairs": (fb(pairs=0), E_ARG, b"pairs"),
        "fb H": (fb(H=0), E_ARG, b"H (0)"), "fb alpha": (fb(alpha=-0.1), E_ARG, b"tolerance"),
        "fb nan beta": (fb(beta=nan), E_ARG, b"tolerance"),
        "fb fwd misaligned": (fb(fwd=x + 4), E_ALIGN, b"fwd"), "fb bwd misaligned": (fb(bwd=x + 12), E_ALIGN, b"bwd"),
        "estimate null frames": (est(frames=None), E_ARG, b"null"), "estimate null flow": (est(flow=None), E_ARG, b"null"),
        "estimate null workspace": (est(ws=None), E_ARG, b"null"),
        "estimate null flow_bwd": (est(bwd=None), E_ARG, b"null"), "estimate null valid": (est(valid=None), E_ARG, b"null"),
        "estimate N": (est(N=1), E_ARG, b"N (1)"), "estimate H": (est(H=0), E_ARG, b"H (0)"),
        "estimate k 0": (est(k=0), E_ARG, b"frame_step"), "estimate k N": (est(k=3), E_ARG, b"frame_step"),
        "estimate dtype": (est(dtype=4), E_ARG, b"dtype"), "estimate radius": (est(r=8), E_ARG, b"radius"),
        "estimate levels": (est(levels=6), E_ARG, b"levels"), "estimate iterations": (est(it=0), E_ARG, b"iterations"),
        "estimate damping": (est(damping=nan), E_ARG, b"damping"), "estimate alpha": (est(alpha=-1.0), E_ARG, b"tolerance"),
        "estimate workspace misaligned": (est(ws=x + 8), E_ALIGN, b"workspace"),
        "estimate flow misaligned": (est(flow=x + 4), E_ALIGN, b"flow"),
        "estimate flow_bwd misaligned": (est(bwd=x + 4), E_ALIGN, b"flow_bwd"),
        "estimate too many pairs": (est(N=65537), E_UNSUP, b"65535 pairs"),
    }
    wrong = {k: v for k, ((rc, msg), code, word) in cases.items() for v in [(rc, msg)] if rc != code or word not in msg}
    assert not wrong, wrong
