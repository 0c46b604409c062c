"""Strided snippet jobs (start steps > 1) through the sharded merge kernels and the multi-rank forward:
rdmi_aligner_merge_partial_window_strided / rdmi_aligner_merge_finish_pieces_strided against the
single-GPU rdmi_aligner_merge_strided, and shard.sharded_forward / RollingDepthPipeline.forward under
enable_snippet_parallel() against the single-GPU strided forward.  Layouts as in
tests/test_shard_strided_cpu.py:
  L-on   N = 23, dilations (1, 4, 7), lengths (3, 2, 2), start steps (2, 3, 5): 11 / 7 / 4 snippets
  L-off  the same geometry, start steps (3, 4, 2): 8 / 6 / 9, every last window off the start grid
  L-gap  N = 14, dilation (1), length (3), start step (4): frames 3 and 7 in no snippet"""
import json
import os
import socket

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(__file__), "golden")

LAYOUTS = {"on": (23, (1, 4, 7), (3, 2, 2), (2, 3, 5), (11, 7, 4)),
           "off": (23, (1, 4, 7), (3, 2, 2), (3, 4, 2), (8, 6, 9)),
           "gap": (14, (1,), (3,), (4,), (4,))}
H, W = 24, 20
HW = H * W


def _starts(N, w, dil, ss):
    win = (w - 1) * dil + 1
    st = list(range(0, N - win + 1, ss))
    if st[-1] < N - win:
        st.append(N - win)
    return st


_JOBS = {}


def _job(layout, f32):
    """Snippets, scales, translations, min shift of one layout (device tensors) and the single-GPU
    strided merge of them — computed once per (layout, dtype) and shared, never written to."""
    if (layout, f32) not in _JOBS:
        from rollingdepth_amd import kernels as K

        N, dil, w, ss, counts = LAYOUTS[layout]
        rng = np.random.default_rng(3)
        base = rng.uniform(-1, 1, (N, H, W)).astype(np.float32)
        xf, sc, tr = [], [], []
        for d, wd, s in zip(dil, w, ss):
            st = _starts(N, wd, d, s)
            x = np.stack([np.stack([base[q + j * d] for j in range(wd)]) for q in st])
            x = x * (0.5 + rng.uniform(0, 1, (len(st), 1, 1, 1))) + 0.3 * rng.standard_normal((len(st), 1, 1, 1))
            xf.append(torch.from_numpy(x.astype(np.float32 if f32 else np.float16)).to(DEV))
            sc.append(torch.from_numpy((1 + 0.1 * rng.standard_normal(len(st))).astype(np.float32)).to(DEV))
            tr.append(torch.from_numpy((0.1 * rng.standard_normal(len(st))).astype(np.float32)).to(DEV))
        assert tuple(x.shape[0] for x in xf) == counts
        shift = torch.tensor([min(float(x.min()) for x in xf)], dtype=torch.float32, device=DEV)
        ref = K.aligner_merge(xf, sc, tr, list(dil), N, shift, f32_arith=True, start_steps=list(ss)).reshape(N, HW)
        _JOBS[(layout, f32)] = (xf, sc, tr, shift, ref)
    return _JOBS[(layout, f32)]


def _windowed(n, dil, w, N, world, xf, sc, tr, shift, mode, start_steps, seq_len, plan_steps):
    """W ranks emulated in one process: per-rank window sums, the all-to-all of
    shard.merge_exchange_plan done by slicing, the finish per frame chunk → ([N, HW] f32, per-rank sums)."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.shard import chunk_bounds, merge_exchange_plan, rank_subsets

    kw = {} if start_steps is None else dict(start_steps=start_steps, seq_len=seq_len)
    sent, all_sums = [], []
    for r in range(world):
        sub = rank_subsets(n, world, r)
        k0 = [x[0] if x else 0 for x in sub]
        rows = [xf[d][k0[d]:k0[d] + len(sub[d])] for d in range(len(n))]
        ranges, send, _ = merge_exchange_plan(n, dil, w, N, world, r, plan_steps)
        sums = torch.cat([K.aligner_merge_partial_window([x if x.shape[0] else None for x in rows], k0, n, sc, tr,
                                                         dil, w, a, b - a, HW, shift, mode, **kw)
                          for a, b in ranges]) if ranges else torch.zeros((0, HW), dtype=torch.float64, device=DEV)
        assert sums.shape[0] == sum(send)
        all_sums.append(sums)
        o, per_dst = 0, []
        for m in send:
            per_dst.append(sums[o:o + m])
            o += m
        sent.append(per_dst)
    got = []
    for r in range(world):
        f0, f1 = chunk_bounds(N, world)[r]
        _, _, recv = merge_exchange_plan(n, dil, w, N, world, r, plan_steps)
        rbuf = torch.cat([sent[s][r] for s in range(world)])
        pieces = [pc for src in recv for pc in src]
        got.append(K.aligner_merge_finish_pieces(rbuf.contiguous(), pieces, n, dil, w, f0, f1 - f0, HW, **kw))
    return torch.cat(got), all_sums


@pytest.mark.parametrize("world", [2, 3, 8, 24])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("layout", ["on", "off", "gap"])
def test_strided_merge_windowed_bitwise(layout, f32, world):
    """The sharded merge of a strided job — rdmi_aligner_merge_partial_window_strided per rank,
    shard.merge_exchange_plan(start_steps), rdmi_aligner_merge_finish_pieces_strided — equals the
    single-GPU rdmi_aligner_merge_strided bitwise (f64 sums of f32 terms), for W ranks emulated in one
    process.  24 ranks over 23 / 23 / 4 snippets leave ranks that own nothing; L-off exercises the
    appended last snippet of every dilation; the frames of L-gap that no snippet reaches are 0 on both
    sides (cover count 0)."""
    N, dil, w, ss, counts = LAYOUTS[layout]
    xf, sc, tr, shift, ref = _job(layout, f32)
    got, _ = _windowed(list(counts), list(dil), list(w), N, world, xf, sc, tr, shift, 1 if f32 else 2, list(ss), N,
                       list(ss))
    assert torch.equal(got, ref)
    if layout == "gap":
        assert not ref[[3, 7]].any() and not got[[3, 7]].any()
        assert ref[[2, 4, 6, 8]].abs().sum(1).min().item() > 0


@pytest.mark.parametrize("world", [3, 24])
@pytest.mark.parametrize("f32", [False, True])
def test_start_step_one_through_strided_entry_points(world, f32):
    """All-ones start steps through the _strided entry points (they take the start-step-1 kernels): the
    per-rank window sums and the finished frames are bitwise those of the existing entry points, on the
    layout of tests/test_aligner_gpu.py::test_aligner_merge_windowed_bitwise (N = 23, dilations (1, 4, 7),
    lengths (3, 2, 2), 21 / 19 / 16 snippets)."""
    N, dil, w = 23, [1, 4, 7], [3, 2, 2]
    n = [N - (wd - 1) * d for d, wd in zip(dil, w)]
    rng = np.random.default_rng(5)
    dt = np.float32 if f32 else np.float16
    xf = [torch.from_numpy(rng.uniform(-1, 1, (m, wd, H, W)).astype(dt)).to(DEV) for m, wd in zip(n, w)]
    sc = [torch.from_numpy((1 + 0.1 * rng.standard_normal(m)).astype(np.float32)).to(DEV) for m in n]
    tr = [torch.from_numpy((0.1 * rng.standard_normal(m)).astype(np.float32)).to(DEV) for m in n]
    shift = torch.tensor([min(float(x.min()) for x in xf)], dtype=torch.float32, device=DEV)
    mode = 1 if f32 else 2
    old, old_sums = _windowed(n, dil, w, N, world, xf, sc, tr, shift, mode, None, None, None)
    new, new_sums = _windowed(n, dil, w, N, world, xf, sc, tr, shift, mode, [1, 1, 1], N, [1, 1, 1])
    assert torch.equal(new, old)
    assert all(torch.equal(a, b) for a, b in zip(new_sums, old_sums))
    assert old.abs().sum().item() > 0


def test_strided_entry_points_refuse_a_wrong_count():
    """N = 14, dilation 3, length 3, start step 2: the last window starts at 7, so the starts are
    0 2 4 6 7 — 5 snippets.  With n = 4 both _strided entry points return RDMI_E_ARG before any launch:
    RdmiError naming the count, and the output tensor keeps its contents."""
    from rollingdepth_amd import kernels as K
    from rollingdepth_amd._native import RdmiError

    N, px = 14, 64
    xf = [torch.rand((4, 3, 8, 8), device=DEV)]
    sc, tr = [torch.ones(4, device=DEV)], [torch.zeros(4, device=DEV)]
    shift = torch.zeros(1, device=DEV)
    sums = torch.full((N, px), 7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(RdmiError, match="gives 5"):
        K.aligner_merge_partial_window(xf, [0], [4], sc, tr, [3], [3], 0, N, px, shift, 1, out=sums,
                                       start_steps=[2], seq_len=N)
    out = torch.full((N, px), 7.0, dtype=torch.float32, device=DEV)
    recv = torch.ones((N, px), dtype=torch.float64, device=DEV)
    with pytest.raises(RdmiError, match="gives 5"):
        K.aligner_merge_finish_pieces(recv, [(0, N)], [4], [3], [3], 0, N, px, start_steps=[2], seq_len=N, out=out)
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((out == 7.0).all())
    # the right count passes both (and a frame window past the sequence does not)
    K.aligner_merge_partial_window([torch.rand((5, 3, 8, 8), device=DEV)], [0], [5], [torch.ones(5, device=DEV)],
                                   [torch.zeros(5, device=DEV)], [3], [3], 0, N, px, shift, 1, out=sums,
                                   start_steps=[2], seq_len=N)
    K.aligner_merge_finish_pieces(recv, [(0, N)], [5], [3], [3], 0, N, px, start_steps=[2], seq_len=N, out=out)
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())
    with pytest.raises(RdmiError):
        K.aligner_merge_finish_pieces(recv, [(0, N)], [5], [3], [3], 1, N, px, start_steps=[2], seq_len=N)


# ------------------------------------------------------------------------------------------------ forward
def _fixture_pipe(name, snippet_batch):
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    t = load_file(os.path.join(G, name + ".safetensors"))
    meta = json.load(open(os.path.join(G, name + ".json")))
    pipe = RollingDepthPipeline.from_synthetic(meta["unet"], meta["vae"], meta["scheduler"], device="cuda")
    pipe.empty_text_embed = t["context"]
    pipe.snippet_batch = snippet_batch
    return t, meta, pipe


def _l1(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().mean().item()


def _worker(rank, world, port, name, strides, with_pipe, res):
    """One of `world` ranks on the one GPU (gloo: device tensors staged through the host).  res:
    [0] depth L1 sharded_forward vs single GPU, [1] coaligned L1, [2] UNet frames over all ranks − single
    GPU's, and with_pipe: [3] depth_pred, [4] depth_coaligned, [5] worst snippet_ls L1 of
    enable_snippet_parallel() + forward vs single GPU, [6] that run's UNet frames − single GPU's."""
    import torch.distributed as dist
    from rollingdepth_amd.shard import sharded_forward
    from tests.test_pipeline_gpu import _count_unet_frames

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t, meta, pipe = _fixture_pipe(name, 3)
    rs, rsd = meta.get("refine_step", 0), meta.get("refine_start_dilation", 6)
    seen = _count_unet_frames(pipe)

    def frames_all_ranks():
        n = torch.tensor([float(sum(seen))])
        dist.all_reduce(n)
        seen.clear()
        return n.item()

    so = sharded_forward(pipe, t["frames"][None].cuda(), list(meta["dilations_in"]), True, 3, None,
                         init_noise=t["init_noise"].cuda(), refine_step=rs, refine_start_dilation=rsd, gather=True,
                         strides=list(strides))
    torch.cuda.synchronize()
    n_shard = frames_all_ranks()
    po, n_pipe = None, 0.0
    if with_pipe:
        pipe.enable_snippet_parallel()
        po = pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], list(strides), None, rs, 3,
                          rsd, None, False, 4, False, init_noise=t["init_noise"])
        torch.cuda.synchronize()
        n_pipe = frames_all_ranks()
        pipe._group = None
    dist.barrier()
    if rank == 0:
        pipe.snippet_batch = 8
        out = pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], list(strides), None, rs, 3,
                           rsd, None, False, 4, False, init_noise=t["init_noise"])
        n_single = sum(seen)
        res[0] = _l1(so.depth_pred_full, out.depth_pred)
        res[1] = _l1(so.depth_coaligned_full, out.depth_coaligned)
        res[2] = n_shard - n_single
        print(f"{name} strides {list(strides)} world {world}: snippets {so.snippet_counts}, sharded vs single-GPU "
              f"depth L1 {res[0]:.2e}, coaligned {res[1]:.2e}; UNet frames {n_shard:.0f} vs {n_single}")
        if with_pipe:
            assert [s.shape for s in po.snippet_ls] == [s.shape for s in out.snippet_ls]
            res[3] = _l1(po.depth_pred, out.depth_pred)
            res[4] = _l1(po.depth_coaligned, out.depth_coaligned)
            res[5] = max(_l1(a, b) for a, b in zip(po.snippet_ls, out.snippet_ls))
            res[6] = n_pipe - n_single
            print(f"  enable_snippet_parallel + forward: depth {res[3]:.2e}, coaligned {res[4]:.2e}, snippets "
                  f"{res[5]:.2e}; UNet frames {n_pipe:.0f}")
    dist.destroy_process_group()


_RUNS = {}


def _run(name, strides, world, with_pipe=False):
    """Spawn the ranks of one case once; the tests that read the same case share its result."""
    key = (name, tuple(strides), world)
    if key not in _RUNS:
        import torch.multiprocessing as mp

        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        ctx = mp.get_context("spawn")
        res = ctx.Array("d", [1.0, 1.0, -1.0, 1.0, 1.0, 1.0, -1.0])
        procs = [ctx.Process(target=_worker, args=(r, world, port, name, list(strides), with_pipe, res))
                 for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(240)
        _RUNS[key] = ([p.exitcode for p in procs], list(res))
    return _RUNS[key]


# the case the pipeline-level test shares: its worker also runs enable_snippet_parallel() + forward
PIPE_CASE = ("tiny_pipeline", (2, 2), 2)


@pytest.mark.parametrize("name,strides,world", [PIPE_CASE, ("tiny_pipeline", (1, 3), 2), ("tiny_pipeline", (3, 1), 2),
                                                ("tiny_pipeline", (2, 2), 3), ("tiny_refine", (2, 2), 2)])
def test_sharded_forward_strided_multi_rank_one_gpu(name, strides, world):
    """sharded_forward(strides=…) over W ranks on the one GPU (collectives over gloo), gathered and
    compared with rank 0's single-GPU pipe.forward(strides=…) on the same noise: 9 frames 32², dilations
    [1, 2] → 4 + 3, 7 + 3 and 3 + 5 snippets; tiny_refine runs the sharded refine after a strided merge.
    Bound: depth L1 ≤ 1e-5, the bound of test_sharded_forward_multi_rank_one_gpu (the cross-rank sums are
    exact f64 sums; at these sizes the two agree bitwise).  The ranks together run exactly the single-GPU
    forward's UNet frames."""
    codes, res = _run(name, strides, world, with_pipe=(name, strides, world) == PIPE_CASE)
    assert all(c == 0 for c in codes), codes
    assert res[0] <= 1e-5 and res[1] <= 1e-5 and res[2] == 0, res


def test_pipeline_forward_strided_snippet_parallel():
    """pipe.enable_snippet_parallel() + pipe.forward(..., strides=[2, 2]) on 2 ranks (the worker of the
    first case above): depth_pred, depth_coaligned and every snippet_ls[d] match the single-GPU
    forward to the same bound, and the ranks ran its UNet frames once."""
    codes, res = _run(*PIPE_CASE, with_pipe=True)
    assert all(c == 0 for c in codes), codes
    assert res[3] <= 1e-5 and res[4] <= 1e-5 and res[5] <= 1e-5 and res[6] == 0, res


def test_sharded_forward_strided_world1_equals_forward():
    """sharded_forward(strides=[2, 2]) over a 1-rank RCCL group — strided window sums, all-to-all with
    itself, strided cover-count finish — reproduces pipe.forward(strides=[2, 2]) bitwise."""
    from rollingdepth_amd.shard import sharded_forward
    from tests.test_pipeline_gpu import _rccl_world1

    t, meta, pipe = _fixture_pipe("tiny_pipeline", 8)
    out = pipe.forward(t["frames"][None], list(meta["dilations_in"]), True, [3], [1], [2, 2], None, 0, 3, 6, None,
                       False, 4, False, init_noise=t["init_noise"])
    dist = _rccl_world1()
    try:
        so = sharded_forward(pipe, t["frames"][None].cuda(), list(meta["dilations_in"]), True, 3, None,
                             init_noise=t["init_noise"].cuda(), gather=True, strides=[2, 2])
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert so.snippet_counts == [4, 3]
    for a, b in zip(so.snippet_rows, out.snippet_ls):
        assert torch.equal(a.to(b.dtype).cpu(), b.view(a.shape))
    assert torch.equal(so.depth_coaligned_full.cpu(), out.depth_coaligned)
    assert torch.equal(so.depth_pred_full.cpu(), out.depth_pred)
