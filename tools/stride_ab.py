"""What snippet strides > 1 buy and cost at the fast-preset geometry (one GPU).

    python tools/stride_ab.py [--rounds 3] [--frames 100] [--res 768] [--aligner-iters 2000]

pipe.forward on bench.py's fast-preset workload (100 synthetic 768² frames, dilations [1, 25], f16, no
refine, synthetic weights) with strides [1, 1], [1, 5] and [2, 5], interleaved: one warm-up of each
variant, then `rounds` rounds of the three in turn.  Per variant: the snippet counts, the median depth
frames/s, the run-to-run spread, the aligner time (device time of DepthAligner.run) and — as information
only — the mean |Δ depth_pred| against the [1, 1] run of the same process (the quality cost of the knob
on synthetic weights: no bound), plain and after one least-squares scale and shift of the variant onto the
[1, 1] run (rollingdepth_amd.metrics.depth_metrics, align="video": the plain mean is mostly the offset that
depth_pred's renormalisation moves).  The time base is the [1, 1] run of the same interleave.

    python tools/stride_ab.py --slice-world 8 [--rounds 2]

times instead each rank's share of a W-rank step of the three variants on this one GPU, under
shard.SliceGroup (shard.sharded_forward(strides=…): the rank's encode chunk, its snippets, the replicated
aligner, its strided window sums and finish; every collective a local no-op — what bench.py --slice-world
does for stride 1).  Per variant: every rank's median step and phases, the slowest rank, and the
single-GPU step of the same variant.  A rank-slice prediction, not a scaling result: nothing ran on W
GPUs and the collectives' time is left out.

    python tools/stride_ab.py --refine [--rounds 3] [--frames 100] [--res 512]

measures instead the refine stage's knob, `refine_stride`, on the full preset's structure (dilations
[1, 10, 25], refine_step 10 from dilation 6, f16, synthetic weights; 512² by default so that the twelve
forwards finish in a few minutes): refine_stride 1, 2 and 3 interleaved, one warm-up of each, then `rounds`
rounds.  Per variant: depth frames/s (median, min .. max), the UNet frames of the refine stage and of the
whole forward, the speed-up the UNet-frame counts alone predict (all UNet frames of the stride-1 forward ÷
this variant's: the VAE, the aligner and the glue do not shrink), the measured one, the device time of the
refine stage and — as information only, on random-init weights — the mean |Δ depth_pred| against the
stride-1 run of the same process, plain and after the video-level fit.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ([1, 1], [1, 5], [2, 5])


def fitted_mean_abs(variant, base):
    """mean |s·variant + t − base| with one least-squares (s, t) for the video: the difference that is left
    when the offset of depth_pred's renormalisation is taken out (every pixel counts: no valid range)."""
    from rollingdepth_amd.metrics import depth_metrics

    inf = float("inf")
    return depth_metrics(variant, base, align="video", valid_range=(-inf, inf)).mae


def slice_world(a, pipe, frames, noise, coalign, one):
    """--slice-world W: per variant, each rank's share of the W-rank step timed alone on this GPU."""
    from rollingdepth_amd.shard import SliceGroup, chunk_bounds, rank_subsets, sharded_forward

    Wd, N = a.slice_world, a.frames
    rows = []
    for v in VARIANTS:
        one(v)  # warm-up, then the single-GPU step of this variant
        single = statistics.median(one(v)[0] for _ in range(a.rounds))
        ranks = []
        for r in range(Wd):
            lo, hi = chunk_bounds(N, Wd)[r]
            fr = frames[0, lo:hi]
            g = SliceGroup(r, Wd)

            def step(timing=None):
                return sharded_forward(pipe, fr, [1, 25], True, 3, coalign, init_noise=noise, num_frames=N,
                                       to_host=True, group=g, timing=timing, strides=list(v))

            so = step()
            torch.cuda.synchronize()
            walls, phases = [], {}
            for _ in range(a.rounds):
                tm = []
                t0 = time.perf_counter()
                step(tm)
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
                for (_, e0), (n1, e1) in zip(tm, tm[1:]):
                    phases[n1] = phases.get(n1, 0.0) + e0.elapsed_time(e1) / a.rounds
            ranks.append({"rank": r, "ms": round(statistics.median(walls) * 1e3, 1), "frames": hi - lo,
                          "snippets": [len(x) for x in rank_subsets(so.snippet_counts, Wd, r)],
                          "phases_ms": {k: round(x, 1) for k, x in phases.items()}})
            print(f"strides {v} W={Wd} rank {r}: {ranks[-1]['ms']} ms, snippets {ranks[-1]['snippets']}, "
                  f"{ranks[-1]['phases_ms']}", flush=True)
        slow = max(ranks, key=lambda x: x["ms"])
        rows.append({"strides": v, "snippets": so.snippet_counts, "single_gpu_ms": round(single * 1e3, 1),
                     "slowest_rank": slow["rank"], "slowest_rank_ms": slow["ms"],
                     "fastest_rank_ms": min(x["ms"] for x in ranks), "ranks": ranks})
    print(f"| strides | snippets | single GPU ms | slowest of {Wd} rank slices ms | its phases ms |")
    print("|---|---|---|---|---|")
    for row in rows:
        ph = row["ranks"][row["slowest_rank"]]["phases_ms"]
        print(f"| {row['strides']} | {' + '.join(map(str, row['snippets']))} | {row['single_gpu_ms']:.1f} | "
              f"{row['slowest_rank_ms']:.1f} (rank {row['slowest_rank']}) | "
              f"{', '.join(f'{k} {x:.1f}' for k, x in ph.items())} |")
    print(json.dumps({"tool": "stride_ab", "mode": "rank-slice", "note": "each rank's share of a W-rank step timed "
                      "alone on one GPU, collectives left out: a prediction, not a scaling result",
                      "world": Wd, "frames": N, "res": a.res, "rounds": a.rounds, "rows": rows}))


REFINE_VARIANTS = (1, 2, 3)


def refine_ab(a, pipe, frames, noise, coalign):
    """--refine: refine_stride 1, 2, 3 on the full preset's structure, interleaved."""
    seen = {"all": 0, "refine": 0}
    events = []
    unet0, refine0 = pipe.unet.forward, pipe.refine
    inside = [False]

    def unet(x, *args, **kw):
        seen["all"] += x.shape[0]
        if inside[0]:
            seen["refine"] += x.shape[0]
        return unet0(x, *args, **kw)

    def refine(*args, **kw):  # device time and UNet frames of the refine stage
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        inside[0] = True
        e0.record()
        out = refine0(*args, **kw)
        e1.record()
        inside[0] = False
        events.append((e0, e1))
        return out

    pipe.unet.forward, pipe.refine = unet, refine

    def one(s):
        seen.update(all=0, refine=0)
        events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.forward(frames, [1, 10, 25], True, [3], [1], [1], coalign, 10, 3, 6, None, False, 4, False,
                           init_noise=noise, refine_stride=s)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, events[0][0].elapsed_time(events[0][1]), out

    res = {s: {"s": [], "refine_ms": []} for s in REFINE_VARIANTS}
    for s in REFINE_VARIANTS:  # warm-up (and the outputs: every run of a variant computes the same values)
        _, _, out = one(s)
        res[s].update(unet_all=seen["all"], unet_refine=seen["refine"], depth=out.depth_pred.float())
    for r in range(a.rounds):
        for s in REFINE_VARIANTS:
            dt, ms, _ = one(s)
            res[s]["s"].append(dt)
            res[s]["refine_ms"].append(ms)
            print(f"round {r} refine_stride {s}: {dt:.3f} s ({a.frames / dt:.2f} depth frames/s), refine stage "
                  f"{ms:.0f} ms", flush=True)
    base = res[REFINE_VARIANTS[0]]
    bmed = statistics.median(base["s"])
    print("| refine_stride | depth frames/s (median) | min .. max | refine UNet frames | all UNet frames | predicted "
          "from UNet frames | measured | refine stage ms | mean abs Δ depth_pred | after video fit |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    rows = []
    for s in REFINE_VARIANTS:
        x = res[s]
        med = statistics.median(x["s"])
        fps = [a.frames / t for t in x["s"]]
        dd = (x["depth"] - base["depth"]).abs().mean().item()
        df = fitted_mean_abs(x["depth"], base["depth"])
        row = {"refine_stride": s, "frames_per_s": round(a.frames / med, 2), "frames_per_s_min": round(min(fps), 2),
               "frames_per_s_max": round(max(fps), 2), "unet_frames_refine": x["unet_refine"],
               "unet_frames_all": x["unet_all"], "predicted_speedup": round(base["unet_all"] / x["unet_all"], 3),
               "speedup": round(bmed / med, 3), "refine_ms": round(statistics.median(x["refine_ms"]), 1),
               "mean_abs_ddepth": dd, "mean_abs_ddepth_fitted": df}
        rows.append(row)
        print(f"| {s} | {row['frames_per_s']:.2f} | {row['frames_per_s_min']:.2f} .. {row['frames_per_s_max']:.2f} | "
              f"{row['unet_frames_refine']} | {row['unet_frames_all']} | {row['predicted_speedup']:.3f}x | "
              f"{row['speedup']:.3f}x | {row['refine_ms']:.0f} | {dd:.2e} | {df:.2e} |")
    print(json.dumps({"tool": "stride_ab", "mode": "refine", "frames": a.frames, "res": a.res, "rounds": a.rounds,
                      "dilations": [1, 10, 25], "refine_step": 10, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--res", type=int, default=None, help="default 768 (512 with --refine)")
    ap.add_argument("--refine", action="store_true",
                    help="A/B refine_stride 1, 2, 3 on the full preset's structure instead of the snippet strides")
    ap.add_argument("--aligner-iters", type=int, default=2000)
    ap.add_argument("--slice-world", type=int, default=0,
                    help="W: time each rank's share of a strided W-rank step on this GPU (shard.SliceGroup)")
    a = ap.parse_args()
    if a.res is None:
        a.res = 512 if a.refine else 768

    from rollingdepth_amd import aligner as A
    from rollingdepth_amd import config as C
    from rollingdepth_amd import weights as W
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    dev = torch.device("cuda", 0)
    pipe = RollingDepthPipeline.from_synthetic(C.SD2_UNET, C.SD2_VAE, C.RD_SCHEDULER, device=dev,
                                               torch_dtype=torch.float16)
    frames = W.synth_frames(a.frames, a.res, a.res, seed=0)[None].to(dev, torch.float16)
    noise = W.synth_noise(a.res // 8, a.res // 8).to(dev)
    coalign = {"num_iterations": a.aligner_iters}
    if a.refine:
        return refine_ab(a, pipe, frames, noise, coalign)

    events = []
    run0 = A.DepthAligner.run

    def timed_run(self, *args, **kw):  # device time of the co-alignment (prepare, Adam loop, merge)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run0(self, *args, **kw)
        e1.record()
        events.append((e0, e1))
        return out

    A.DepthAligner.run = timed_run

    def one(strides):
        events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe.forward(frames, [1, 25], True, [3], [1], list(strides), coalign, 0, 3, 6, None, False, 4, False,
                           init_noise=noise)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, events[0][0].elapsed_time(events[0][1]), out

    if a.slice_world:
        return slice_world(a, pipe, frames, noise, coalign, one)

    res = {tuple(v): {"s": [], "aligner_ms": []} for v in VARIANTS}
    for v in VARIANTS:  # warm-up (and the outputs: every run of a variant computes the same values)
        _, _, out = one(v)
        res[tuple(v)]["counts"] = [s.shape[0] for s in out.snippet_ls]
        res[tuple(v)]["depth"] = out.depth_pred.float()
    for r in range(a.rounds):
        for v in VARIANTS:
            dt, al, _ = one(v)
            res[tuple(v)]["s"].append(dt)
            res[tuple(v)]["aligner_ms"].append(al)
            print(f"round {r} strides {v}: {dt:.3f} s ({a.frames / dt:.2f} depth frames/s), aligner {al:.1f} ms",
                  flush=True)
    base = res[tuple(VARIANTS[0])]
    bmed = statistics.median(base["s"])
    print("| strides | snippets | depth frames/s (median) | min .. max | vs [1, 1] | aligner ms | mean abs Δ depth_pred | "
          "after video fit |")
    print("|---|---|---|---|---|---|---|---|")
    rows = []
    for v in VARIANTS:
        x = res[tuple(v)]
        med = statistics.median(x["s"])
        fps = [a.frames / s for s in x["s"]]
        dd = (x["depth"] - base["depth"]).abs().mean().item()
        df = fitted_mean_abs(x["depth"], base["depth"])
        row = {"strides": v, "snippets": x["counts"], "frames_per_s": round(a.frames / med, 2),
               "frames_per_s_min": round(min(fps), 2), "frames_per_s_max": round(max(fps), 2),
               "speedup": round(bmed / med, 3), "aligner_ms": round(statistics.median(x["aligner_ms"]), 1),
               "mean_abs_ddepth": dd, "mean_abs_ddepth_fitted": df}
        rows.append(row)
        print(f"| {v} | {' + '.join(map(str, x['counts']))} = {sum(x['counts'])} | {row['frames_per_s']:.2f} | "
              f"{row['frames_per_s_min']:.2f} .. {row['frames_per_s_max']:.2f} | {row['speedup']:.3f}x | "
              f"{row['aligner_ms']:.1f} | {dd:.2e} | {df:.2e} |")
    print(json.dumps({"tool": "stride_ab", "frames": a.frames, "res": a.res, "rounds": a.rounds, "rows": rows}))


if __name__ == "__main__":
    main()
