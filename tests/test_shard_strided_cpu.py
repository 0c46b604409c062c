"""Strided snippet jobs (start steps > 1: a dilation's snippets start every `ss` frames, plus the last
window) through the multi-rank plan of rollingdepth_amd/shard.py, host side: the cover count the
finish kernel divides by (csrc/aligner_index.h, under sanitizers), the frame windows and the all-to-all
plan for strided layouts, the whole windowed merge over gloo ranks with a CPU restatement of the two
kernels, and sharded_forward's validation of `strides`.

Layouts (N, dilations, lengths, start steps → snippet counts):
  L-on   23, (1, 4, 7), (3, 2, 2), (2, 3, 5) → 11 / 7 / 4: every last window (20, 18, 15) on the start grid
  L-off  23, (1, 4, 7), (3, 2, 2), (3, 4, 2) →  8 / 6 / 9: every last window off the grid (appended snippet)
  L-gap  14, (1,), (3,), (4,)                →  4: frames 3 and 7 in no snippet (cover count 0)
and the fast-preset geometry, N = 100, dilations (1, 25): strides (1, 5) → 98 + 11, (2, 5) → 50 + 11."""
import os
import shutil
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L_ON = (23, (1, 4, 7), (3, 2, 2), (2, 3, 5), (11, 7, 4))
L_OFF = (23, (1, 4, 7), (3, 2, 2), (3, 4, 2), (8, 6, 9))
L_GAP = (14, (1,), (3,), (4,), (4,))
FAST_15 = (100, (1, 25), (3, 3), (1, 5), (98, 11))
FAST_25 = (100, (1, 25), (3, 3), (2, 5), (50, 11))
WORLDS = (1, 2, 3, 8, 24)


def _starts(N, w, dil, ss):
    """The reference's snippet starts (get_snippet_indice): range(0, N − win + 1, ss) plus the last window."""
    win = (w - 1) * dil + 1
    st = list(range(0, N - win + 1, ss))
    if st[-1] < N - win:
        st.append(N - win)
    return st


def _cover(N, dil, w, ss):
    """Per frame, the number of (dilation, snippet, slot) triples on it, from the snippet lists."""
    c = [0] * N
    for d, wd, s in zip(dil, w, ss):
        for q in _starts(N, wd, d, s):
            for j in range(wd):
                c[q + j * d] += 1
    return c


def test_cover_count_header_under_sanitizers(tmp_path):
    """rdmi_cover_count (csrc/aligner_index.h — the function merge_finish_pieces_k<true> calls) in a
    stand-alone program built with AddressSanitizer + UBSan, runtimes linked statically: against
    brute-force enumeration of the snippet lists for every N ≤ 40, length ≤ 4, dilation ≤ 6, start step
    ≤ 8 with N ≥ window, one- and two-dilation jobs, every frame."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/cover_count_check.cpp"
    exe = str(tmp_path / "cover_count_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "cover_count_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    per_n = [sum(1 for w in range(1, 5) for d in range(1, 7) for _ in range(1, 9) if N >= (w - 1) * d + 1)
             for N in range(1, 41)]
    assert sum(per_n) == 6672  # the range of tests/test_strided_cpu.py's index-map check
    want = f"{sum(per_n)} one-dilation cases, {sum(c * c for c in per_n)} two-dilation cases, 0 failures"
    assert want in r.stdout, r.stdout


@pytest.mark.parametrize("layout", [L_ON, L_OFF, L_GAP, FAST_15, FAST_25], ids=["on", "off", "gap", "fast15", "fast25"])
def test_strided_merge_plan(layout):
    """merge_exchange_plan / frame_ranges with start steps, planned independently per rank for W = 1, 2,
    3, 8, 24: every frame a rank's own snippets touch lies in its frame ranges (disjoint, sorted); the
    rows rank r sends to rank s are the rows s expects from r, piece by piece inside s's chunk and r's
    ranges; no frame is touched by more than 64 pieces (the finish kernel's table)."""
    from rollingdepth_amd.aligner import snippet_count
    from rollingdepth_amd.shard import chunk_bounds, frame_ranges, merge_exchange_plan, rank_subsets

    N, dil, w, ss, counts = layout
    assert tuple(snippet_count(N, wd, d, s) for d, wd, s in zip(dil, w, ss)) == counts
    assert tuple(len(_starts(N, wd, d, s)) for d, wd, s in zip(dil, w, ss)) == counts
    starts = [_starts(N, wd, d, s) for d, wd, s in zip(dil, w, ss)]
    for W in WORLDS:
        plans = [merge_exchange_plan(counts, dil, w, N, W, r, ss) for r in range(W)]
        chunks = chunk_bounds(N, W)
        touching = [0] * N
        for r in range(W):
            ranges, send, recv = plans[r]
            sub = rank_subsets(counts, W, r)
            assert ranges == frame_ranges(sub, dil, w, ss, N)
            assert all(a < b for a, b in ranges) and all(b1 < a2 for (_, b1), (a2, _) in zip(ranges, ranges[1:]))
            assert all(0 <= a and b <= N for a, b in ranges)
            own = {starts[d][k] + j * dil[d] for d in range(len(dil)) for k in sub[d] for j in range(w[d])}
            assert own <= {f for a, b in ranges for f in range(a, b)}, (W, r)
            assert sum(send) == sum(b - a for a, b in ranges)
            for s in range(W):
                pieces = plans[s][2][r]  # what s expects from r
                assert send[s] == sum(m for _, m in pieces), (W, r, s)
                f0, f1 = chunks[s]
                for a, m in pieces:
                    assert m > 0 and f0 <= a and a + m <= f1
                    assert any(lo <= a and a + m <= hi for lo, hi in ranges)
                    for f in range(a, a + m):
                        touching[f] += 1
                assert {f for f in own if f0 <= f < f1} <= {f for a, m in pieces for f in range(a, a + m)}
            assert len(recv) == W
        assert max(touching) <= 64, (W, max(touching))
        cover = _cover(N, dil, w, ss)
        assert all(touching[f] >= 1 for f in range(N) if cover[f]), W  # a covered frame reaches its owner


def test_start_step_one_plans_are_the_positional_calls():
    """start_steps=None or all ones: frame_ranges and merge_exchange_plan return what the positional
    (start-step-1) calls return — those calls are the ones the stride-1 sharded forward makes."""
    from rollingdepth_amd.shard import frame_ranges, merge_exchange_plan, rank_subsets

    for N, dil, w in ((23, (1, 4, 7), (3, 2, 2)), (14, (1,), (3,)), (100, (1, 25), (3, 3)), (30, (1, 10), (3, 2))):
        counts = [N - (wd - 1) * d for d, wd in zip(dil, w)]
        ones = [1] * len(dil)
        for W in WORLDS:
            for r in range(W):
                want = merge_exchange_plan(counts, dil, w, N, W, r)
                assert merge_exchange_plan(counts, dil, w, N, W, r, None) == want
                assert merge_exchange_plan(counts, dil, w, N, W, r, ones) == want
                assert merge_exchange_plan(counts, dil, w, N, W, r, start_steps=tuple(ones)) == want
                sub = rank_subsets(counts, W, r)
                assert frame_ranges(sub, dil, w, None, None) == frame_ranges(sub, dil, w, ones) == \
                    frame_ranges(sub, dil, w, ones, N) == frame_ranges(sub, dil, w) == want[0]
    with pytest.raises(ValueError):  # start steps > 1 need the sequence length
        frame_ranges([[0, 1]], [1], [3], [2])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _window_sums_cpu(rows, k0, starts, dil, w, sc, tr, N, HW):
    """CPU restatement of rdmi_aligner_merge_partial_window_strided over all N frames (f32 snippets): per
    frame the f64 sum, over this rank's (dilation, local snippet, slot) on it, of the f32 term s·x + t."""
    out = torch.zeros((N, HW), dtype=torch.float64)
    for d, r in enumerate(rows):
        for i in range(r.shape[0]):
            k = k0[d] + i
            for j in range(w[d]):
                term = r[i, j].reshape(-1) * sc[d][k] + tr[d][k]  # f32 arithmetic
                assert term.dtype == torch.float32
                out[starts[d][k] + j * dil[d]] += term.double()
    return out


def _gloo_worker(rank, world, port, res):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rollingdepth_amd.shard import (_all_gather_rows, chunk_bounds, exchange_window_rows, merge_exchange_plan,
                                        rank_subsets)

    N, dil, w, ss, counts = L_OFF
    H, W = 4, 5
    HW = H * W
    g = torch.Generator().manual_seed(11)
    full = [torch.rand((n, wd, H, W), generator=g) for n, wd in zip(counts, w)]
    sc = [0.5 + torch.rand(n, generator=g) for n in counts]
    tr = [0.1 * torch.randn(n, generator=g) for n in counts]
    starts = [_starts(N, wd, d, s) for d, wd, s in zip(dil, w, ss)]
    sub = rank_subsets(counts, world, rank)
    k0 = [s[0] if s else 0 for s in sub]
    rows = [full[d][k0[d]:k0[d] + len(sub[d])] for d in range(len(dil))]
    sums = _window_sums_cpu(rows, k0, starts, dil, w, sc, tr, N, HW)
    ranges, send, recv = merge_exchange_plan(counts, dil, w, N, world, rank, ss)
    ok = bool((sums[[f for f in range(N) if not any(a <= f < b for a, b in ranges)]] == 0).all())
    wsum = torch.cat([sums[a:b] for a, b in ranges]) if ranges else torch.zeros((0, HW), dtype=torch.float64)
    ok &= sum(send) == wsum.shape[0]
    rbuf = exchange_window_rows(wsum, send, [sum(m for _, m in pc) for pc in recv], None)
    f0, f1 = chunk_bounds(N, world)[rank]
    acc = torch.zeros((f1 - f0, HW), dtype=torch.float64)
    o = 0
    for src in recv:  # pieces added per frame in source-rank order (merge_finish_pieces_k)
        for a, m in src:
            acc[a - f0:a - f0 + m] += rbuf[o:o + m]
            o += m
    ok &= o == rbuf.shape[0]
    cover = _cover(N, dil, w, ss)
    ok &= min(cover) >= 1
    mine = torch.stack([acc[i] / cover[f0 + i] for i in range(f1 - f0)]) if f1 > f0 else \
        torch.zeros((0, HW), dtype=torch.float64)
    merged = _all_gather_rows(mine, N, world)
    # direct: per frame the mean over all covering slots, f64 sum of the same f32 terms
    want = _window_sums_cpu(full, [0] * len(dil), starts, dil, w, sc, tr, N, HW) / \
        torch.tensor(cover, dtype=torch.float64)[:, None]
    ok &= torch.equal(merged, want)
    res[rank] = int(ok)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_strided_windowed_merge_gloo(world):
    """L-off over 2 and 3 gloo ranks: window sums of each rank's own snippets (CPU restatement), the real
    merge_exchange_plan(start_steps) and exchange_window_rows, pieces added in source-rank order ÷ the
    cover count == the direct per-frame mean over all covering slots, exactly (f64 sums of f32-valued
    terms in [−1, 3]: at most 7 terms of 24 significant bits within a few binades, exact in any order)."""
    ctx = mp.get_context("spawn")
    res = ctx.Array("i", [0] * world)
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, res)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert list(res) == [1] * world


def _plan_pipe():
    """tests/test_shard_gloo.py's host-only pipeline stand-in, also recording the start steps that reach
    init_snippet_infer."""
    from tests.test_shard_gloo import _PlanPipe

    class _StridedPlanPipe(_PlanPipe):
        def init_snippet_infer(self, rgb_latent, noise, dilations, snippet_lengths, init_infer_steps, strides,
                               snippet_subset=None, record=None):
            self.start_steps = list(strides)
            return super().init_snippet_infer(rgb_latent, noise, dilations, snippet_lengths, init_infer_steps,
                                              strides, snippet_subset=snippet_subset, record=record)

    return _StridedPlanPipe()


def test_sharded_forward_validates_strides():
    """sharded_forward(strides=…) rejects what forward() rejects, before the snippet stage: a layout that
    leaves frames in no snippet (L-gap: the error names frame 3, the first), and strides that are not ints
    ≥ 1.  A valid strided job reaches init_snippet_infer with its start steps and the rank's subset of
    the strided snippet counts."""
    from tests.test_shard_gloo import _StopAtSnippets
    from rollingdepth_amd.shard import SliceGroup, rank_subsets, sharded_forward

    frames = torch.zeros((1, 14, 3, 16, 16))
    noise = torch.zeros(1, 4, 2, 2)
    grp = SliceGroup(1, 2)
    pipe = _plan_pipe()
    with pytest.raises(ValueError, match=r"frame 3 \(2 of 14 frames\)"):
        sharded_forward(pipe, frames, [1], True, 3, None, init_noise=noise, group=grp, strides=(4,))
    for bad in ([0], [1.5], [True], [2, 2], 0, -1):
        with pytest.raises(ValueError, match="strides"):
            sharded_forward(pipe, frames, [1], True, 3, None, init_noise=noise, group=grp, strides=bad)
    assert pipe.calls == []  # nothing reached the snippet stage
    for strides, want_ss, counts in ((2, [2, 2], [7, 5]), ([3, 2], [3, 2], [5, 5]), ([1], [1, 1], [12, 8]), (1, [1, 1], [12, 8])):
        pipe = _plan_pipe()
        with pytest.raises(_StopAtSnippets):  # N = 14, dilations (1, 3), length 3: last windows 11 and 7
            sharded_forward(pipe, frames, [1, 3], True, 3, None, init_noise=noise, group=grp, strides=strides)
        assert pipe.start_steps == want_ss
        assert pipe.calls[0]["subset"] == rank_subsets(counts, 2, 1)
