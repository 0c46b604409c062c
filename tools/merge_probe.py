"""Time the merge with and without the per-pixel spread on the same inputs (one GPU).

    python tools/merge_probe.py [--call merge|moments|both] [--frames 100] [--res 768] [--dilations 1 25]
                                [--f16] [--reps 10] [--warmup 3]

The fast preset's geometry by default: 100 frames 768², dilations [1, 25], snippets of 3 → 98 + 50 snippets,
f32 (the decoded snippets' dtype there), seeded so that every run sees the same data.  HIP events, the median
of `reps` after `warmup` calls, for
  * rdmi_aligner_merge         (kernels.aligner_merge: the mean alone),
  * rdmi_aligner_merge_moments (kernels.aligner_merge_moments: the mean and the spread in one pass).
--call picks one of them, so that a job script can run each under its own `timeout`.
Bytes are algorithmic: every snippet slot is read once (Σ n_d · w · HW elements) and each output map written
once (N · HW · 4 B: one map for the merge, two for the fused call).  The two means are compared bitwise.
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--call", choices=["merge", "moments", "both"], default="both")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--dilations", type=int, nargs="+", default=[1, 25])
    ap.add_argument("--f16", action="store_true", help="f16 snippets merged in f32 arithmetic (x_f32 = 2)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    from rollingdepth_amd import kernels as K

    dev = torch.device("cuda", 0)
    N, HW, w = a.frames, a.res * a.res, 3
    g = torch.Generator(device=dev).manual_seed(0)
    counts = [N - (w - 1) * d for d in a.dilations]
    dt = torch.float16 if a.f16 else torch.float32
    xf = [torch.rand((n, w, a.res, a.res), generator=g, device=dev).to(dt) for n in counts]
    sc = [1 + 0.1 * torch.randn(n, generator=g, device=dev) for n in counts]
    tr = [0.1 * torch.randn(n, generator=g, device=dev) for n in counts]
    shift = K.minmax(torch.stack([K.minmax(x) for x in xf]).reshape(-1))
    esz = 2 if a.f16 else 4
    reads = sum(counts) * w * HW * esz
    runs = {
        "merge": ("rdmi_aligner_merge", reads + N * HW * 4,
                  lambda: K.aligner_merge(xf, sc, tr, a.dilations, N, shift, f32_arith=True)),
        "moments": ("rdmi_aligner_merge_moments", reads + 2 * N * HW * 4,
                    lambda: K.aligner_merge_moments(xf, sc, tr, a.dilations, N, shift, f32_arith=True)),
    }
    mean = K.aligner_merge(xf, sc, tr, a.dilations, N, shift, f32_arith=True)
    mean2, std = K.aligner_merge_moments(xf, sc, tr, a.dilations, N, shift, f32_arith=True)
    print(f"{N} x {a.res}^2, dilations {a.dilations}, {' + '.join(map(str, counts))} snippets of {w}, "
          f"{'f16' if a.f16 else 'f32'} snippets; means bitwise equal {torch.equal(mean, mean2)}; "
          f"std mean {std.mean().item():.6f} max {std.max().item():.6f}")
    del mean, mean2, std
    print("| call | ms (median) | min .. max | bytes | TB/s |")
    print("|---|---|---|---|---|")
    rows = []
    for key, (name, nbytes, fn) in runs.items():
        if a.call not in (key, "both"):
            continue
        med, lo, hi = timed(fn, a.reps, a.warmup)
        rows.append({"call": name, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                     "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e9, 3)})
        print(f"| {name} | {med:.3f} | {lo:.3f} .. {hi:.3f} | {nbytes} | {nbytes / med / 1e9:.2f} |", flush=True)
    print(json.dumps({"tool": "merge_probe", "frames": N, "res": a.res, "dilations": a.dilations,
                      "snippets": counts, "f16": a.f16, "reps": a.reps, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
