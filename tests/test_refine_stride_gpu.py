"""Strided refine on the device: the three strided averaging kernels (csrc/elementwise.hip over
csrc/refine_index.h) bitwise against f64 sums in torch over the host list
(pipeline.refine_snippet_indice), and RollingDepthPipeline.forward / shard.sharded_forward with
`refine_stride` 1, 2 and 3 on the tiny_refine fixture (9 frames 32², refine at d = 2, then d = 1)."""
import json
import os
import socket

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")
DTYPES = [torch.float16, torch.float32]

# (N, w, d, s): the smallest shapes that reach each branch of the index map
SHAPES = [(11, 3, 2, 2),  # classes of length 6 and 5; an appended last window in class 0
          (14, 4, 3, 3),  # R = 2, lengths 5, 5, 4; one class with a single snippet
          (9, 3, 1, 3),   # every frame covered exactly once
          (10, 3, 1, 3),  # appended window: frames 7 and 8 covered twice
          (7, 3, 3, 2)]   # lengths 3, 2, 2: two classes without a snippet → frames with count 0 → zeros
H, WD, C, LD = 5, 7, 4, 8


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _reference(src, idx, N, dtype):
    """Per frame: f64 sum of the covering predictions ÷ cover count → f32 → dtype (zeros where the count
    is 0); also the f64 sums and the counts.  src [n, w, h, wd, ≥ C] on the host, idx the host list."""
    sums = torch.zeros(N, *src.shape[2:4], C, dtype=torch.float64)
    cnt = torch.zeros(N, dtype=torch.float64)
    for k, sn in enumerate(idx):
        for j, f in enumerate(sn):
            sums[f] += src[k, j, ..., :C].double()
            cnt[f] += 1
    c4 = cnt.view(N, 1, 1, 1)
    mean = torch.where(c4 > 0, sums / c4.clamp_min(1), torch.zeros((), dtype=torch.float64))
    return mean.float().to(dtype), sums, cnt


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_w%d_d%d_s%d" % s)
def test_strided_average_kernels(shape, dtype):
    """snippet_average_strided against the f64 reference, bitwise, pad channels exactly 0;
    snippet_accumulate_strided over the shards (0, 3), (3, 0), (3, rest) of the rows (clipped to the row
    count), summed — exactly the reference sums — then snippet_finish_strided: the bits of the average.  The
    sums of ≤ 4 such terms are exact in f64, so the statement is that of tests/test_glue_gpu.py."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.pipeline import refine_snippet_indice

    N, w, d, s = shape
    idx = refine_snippet_indice(N, w, d, s)
    n = len(idx)
    g = torch.Generator().manual_seed(1000 * N + 100 * w + 10 * d + s)
    src = torch.randn(n, w, H, WD, LD, generator=g).to(dtype)  # padding channels hold junk, never read
    ref, sums, cnt = _reference(src, idx, N, dtype)
    if shape == (7, 3, 3, 2):
        assert n == 1 and sorted(torch.nonzero(cnt == 0).flatten().tolist()) == [1, 2, 4, 5]
    elif shape == (9, 3, 1, 3):
        assert (cnt == 1).all()
    elif shape == (10, 3, 1, 3):
        assert cnt.tolist() == [1.0] * 7 + [2.0, 2.0, 1.0]
    else:
        assert (cnt > 0).all()
    sd = src.to(DEV)
    avg = K.snippet_average_strided(sd, d, s, N)
    assert avg.shape == (N, H, WD, LD) and avg.dtype == dtype
    assert torch.equal(_bits(avg[..., :C].cpu()), _bits(ref))
    assert (avg[..., C:] == 0).all() and (avg[cnt.to(DEV) == 0] == 0).all()
    a = min(3, n)
    total = sum(K.snippet_accumulate_strided(sd[k0:k0 + nloc], k0, d, s, N)
                for k0, nloc in ((0, a), (a, 0), (a, n - a)))
    assert total.dtype == torch.float64 and torch.equal(total.cpu(), sums.view(N, H * WD, C))
    fin = K.snippet_finish_strided(total, n, w, d, s, (H, WD), LD, dtype=dtype)
    assert torch.equal(_bits(fin), _bits(avg))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_w%d_d%d" % s[:3])
def test_strided_average_start_step_1_is_snippet_average(shape, dtype):
    """At start step 1 the class-major list is get_snippet_indice's, permuted: snippet_average_strided on
    the permuted rows gives the bits of rdmi_snippet_average on the rows in start-frame order."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.pipeline import refine_snippet_indice

    N, w, d, _ = shape
    idx = refine_snippet_indice(N, w, d, 1)
    n = len(idx)
    order = sorted(range(n), key=lambda k: idx[k][0])  # order[i]: class-major row of the i-th start frame
    if d <= N // w:
        assert [idx[k][0] for k in order] == list(range(n))  # "snippet k starts at frame k"
    g = torch.Generator().manual_seed(7 + N)
    nat = torch.randn(n, w, H, WD, LD, generator=g).to(dtype).to(DEV)
    cm = torch.empty_like(nat)
    cm[order] = nat
    want = K.snippet_average(nat, d, N)
    got = K.snippet_average_strided(cm, d, 1, N)
    assert torch.equal(_bits(got), _bits(want))


def test_strided_average_rejects_bad_start_step():
    """start_step 0 and w + 1 (and a row count other than the map's) are refused before any launch:
    RdmiError, outputs untouched."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import _native
    from rollingdepth_amd._native import RdmiError

    N, w, d = 11, 3, 2
    src = torch.randn(5, w, H, WD, LD).half().to(DEV)
    sums = torch.full((N, H * WD, C), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((N, H, WD, LD), 7.0, dtype=torch.float16, device=DEV)
    for ss in (0, w + 1):
        with pytest.raises(RdmiError, match=f"start step {ss}"):
            K.snippet_average_strided(src, d, ss, N)
        with pytest.raises(RdmiError, match=f"start step {ss}"):
            K.snippet_accumulate_strided(src, 0, d, ss, N, out=sums)
        with pytest.raises(RdmiError, match=f"start step {ss}"):
            K.snippet_finish_strided(sums, 5, w, d, ss, (H, WD), LD)
        rc = _native.lib.rdmi_snippet_average_strided(src.data_ptr(), 5, w, d, ss, N, H * WD, C, LD, out.data_ptr(),
                                                      _native.RDMI_F16, None)
        assert rc == 1001
    with pytest.raises(RdmiError, match="gives 5"):
        K.snippet_average_strided(src[:4], d, 2, N)
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ pipeline
def _fixture_pipe(snippet_batch=8):
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    t = load_file(os.path.join(G, "tiny_refine.safetensors"))
    meta = json.load(open(os.path.join(G, "tiny_refine.json")))
    pipe = RollingDepthPipeline.from_synthetic(meta["unet"], meta["vae"], meta["scheduler"], device="cuda")
    pipe.empty_text_embed = t["context"]
    pipe.snippet_batch = snippet_batch
    return t, meta, pipe


def _forward(pipe, t, meta, record=None, **kw):
    return pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], [1], None, meta["refine_step"], 3,
                        meta["refine_start_dilation"], None, False, 4, False, init_noise=t["init_noise"], record=record,
                        **kw)


def _refine_frame_steps(pipe, meta, N, w=3):
    """The frame step d of each refine step, from the unchanged dilation schedule."""
    d0 = pipe.cap_max_dilation(N, w, meta["refine_start_dilation"])
    ts = list(range(meta["refine_step"]))
    out = []
    for i in range(len(ts)):
        sn = pipe.get_snippet_indice(i, ts, N, w, d0, 1, 1)[0]
        out.append(sn[1] - sn[0])
    return out


@pytest.fixture(scope="module")
def tiny():
    """The fixture pipeline, its default forward (with record) and the UNet-frame counter."""
    from tests.test_pipeline_gpu import _count_unet_frames

    t, meta, pipe = _fixture_pipe()
    seen = _count_unet_frames(pipe)
    rec = {}
    out = _forward(pipe, t, meta, record=rec)
    base_frames = sum(seen)
    seen.clear()
    return t, meta, pipe, seen, out, rec, base_frames


def test_refine_stride_1_is_the_default(tiny):
    """refine_stride=1 passed explicitly: depth_pred and the refined latents are the default call's bits."""
    t, meta, pipe, seen, out, rec, _ = tiny
    rec1 = {}
    out1 = _forward(pipe, t, meta, record=rec1, refine_stride=1)
    seen.clear()
    assert torch.equal(_bits(out1.depth_pred), _bits(out.depth_pred))
    assert torch.equal(_bits(out1.depth_coaligned), _bits(out.depth_coaligned))
    assert torch.equal(_bits(rec1["refined_latent"]), _bits(rec["refined_latent"]))


@pytest.mark.parametrize("stride", [2, 3])
def test_refine_stride_single_gpu(tiny, stride):
    """refine_stride 2 and 3: finite outputs; the refine UNet calls process Σ_steps
    len(refine_snippet_indice(N, 3, d, stride))·3 frames (d = 2, then 1); each step's averaged latents are,
    bitwise, the f64 average recomputed in torch from that step's predictions and the host list."""
    from rollingdepth_amd.pipeline import refine_snippet_count, refine_snippet_indice

    t, meta, pipe, seen, out, rec, base_frames = tiny
    N, w = t["frames"].shape[0], 3
    steps = _refine_frame_steps(pipe, meta, N)
    assert steps == [2, 1]
    seen.clear()
    rs = {}
    o = _forward(pipe, t, meta, record=rs, refine_stride=stride)
    frames = sum(seen)
    seen.clear()
    assert torch.isfinite(o.depth_pred.float()).all() and torch.isfinite(rs["refined_latent"].float()).all()
    assert torch.equal(_bits(o.depth_coaligned), _bits(out.depth_coaligned))  # the initial stage is untouched
    init_frames = sum(s.shape[0] * s.shape[1] for s in o.snippet_ls)
    lists = [refine_snippet_indice(N, w, d, stride) for d in steps]
    assert frames - init_frames == sum(len(ix) for ix in lists) * w
    assert [len(ix) for ix in lists] == [refine_snippet_count(N, w, d, stride) for d in steps]
    # fewer refine frames than the default run's
    assert frames - init_frames < base_frames - init_frames == sum(refine_snippet_count(N, w, d, 1) for d in steps) * w
    assert len(rs["refine_pred"]) == len(rs["refine_latent"]) == len(steps)
    for ix, pred, lat in zip(lists, rs["refine_pred"], rs["refine_latent"]):
        assert pred.shape[:2] == (len(ix), w) and lat.shape[0] == N
        ref, _, cnt = _reference(pred.cpu(), ix, N, pred.dtype)
        assert (cnt > 0).all()
        assert torch.equal(_bits(lat[..., :C].cpu()), _bits(ref))
        assert (lat[..., C:] == 0).all()
    assert torch.equal(_bits(rs["refine_latent"][-1]), _bits(rs["refined_latent"]))


def test_refine_stride_rejected_before_inference(tiny):
    """refine_stride above refine_snippet_len, 0, a bool and a float raise ValueError before any UNet call."""
    t, meta, pipe, seen, *_ = tiny
    seen.clear()
    for bad in (4, 0, True, 2.0):
        with pytest.raises(ValueError, match="refine_stride"):
            _forward(pipe, t, meta, refine_stride=bad)
    assert not seen


# ------------------------------------------------------------------------------------------------ sharded
def _l1(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().mean().item()


def _worker(rank, world, port, stride, with_pipe, res):
    """One of `world` ranks on the one GPU (gloo).  res: [0] depth L1 sharded_forward(refine_stride) vs the
    single-GPU forward(refine_stride), [1] UNet frames over all ranks − single GPU's, and with_pipe: [2], [3]
    the same for enable_snippet_parallel() + forward."""
    import torch.distributed as dist
    from rollingdepth_amd.shard import sharded_forward
    from tests.test_pipeline_gpu import _count_unet_frames

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t, meta, pipe = _fixture_pipe(3)
    seen = _count_unet_frames(pipe)

    def frames_all_ranks():
        n = torch.tensor([float(sum(seen))])
        dist.all_reduce(n)
        seen.clear()
        return n.item()

    so = sharded_forward(pipe, t["frames"][None].cuda(), list(meta["dilations_in"]), True, 3, None,
                         init_noise=t["init_noise"].cuda(), refine_step=meta["refine_step"],
                         refine_start_dilation=meta["refine_start_dilation"], gather=True, refine_stride=stride)
    torch.cuda.synchronize()
    n_shard = frames_all_ranks()
    po, n_pipe = None, 0.0
    if with_pipe:
        pipe.enable_snippet_parallel()
        po = _forward(pipe, t, meta, refine_stride=stride)
        torch.cuda.synchronize()
        n_pipe = frames_all_ranks()
        pipe._group = None
    dist.barrier()
    if rank == 0:
        pipe.snippet_batch = 8
        out = _forward(pipe, t, meta, refine_stride=stride)
        n_single = sum(seen)
        res[0] = _l1(so.depth_pred_full, out.depth_pred)
        res[1] = n_shard - n_single
        print(f"tiny_refine refine_stride {stride} world {world}: sharded vs single-GPU depth L1 {res[0]:.2e}; "
              f"UNet frames {n_shard:.0f} vs {n_single}")
        if with_pipe:
            res[2] = _l1(po.depth_pred, out.depth_pred)
            res[3] = n_pipe - n_single
            print(f"  enable_snippet_parallel + forward: depth L1 {res[2]:.2e}; UNet frames {n_pipe:.0f}")
    dist.destroy_process_group()


PIPE_CASE = (2, 2)  # (world, stride): its worker also runs enable_snippet_parallel() + forward


@pytest.mark.parametrize("world,stride", [(2, 2), (2, 3), (3, 2), (3, 3)])
def test_sharded_refine_stride_multi_rank_one_gpu(world, stride):
    """sharded_forward(refine_stride=…) over W ranks on the one GPU (collectives over gloo, f16), gathered
    and compared with rank 0's single-GPU forward(refine_stride=…) on the same noise.  Bound: depth L1
    ≤ 1e-5, the bound of test_sharded_forward_multi_rank_one_gpu (the cross-rank sums are exact f64 sums).
    The ranks together run exactly the single-GPU forward's UNet frames.  The first case also runs
    enable_snippet_parallel() + forward(refine_stride=…) to the same bound."""
    import torch.multiprocessing as mp

    with_pipe = (world, stride) == PIPE_CASE
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    res = ctx.Array("d", [1.0, -1.0, 1.0, -1.0])
    procs = [ctx.Process(target=_worker, args=(r, world, port, stride, with_pipe, res)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert res[0] <= 1e-5 and res[1] == 0, list(res)
    if with_pipe:
        assert res[2] <= 1e-5 and res[3] == 0, list(res)
