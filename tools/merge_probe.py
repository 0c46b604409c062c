"""Time the merge with and without the per-pixel spread on the same inputs (one GPU).

    python tools/merge_probe.py [--call merge|moments|both|median] [--frames 100] [--res 768] [--dilations 1 25]
                                [--snippet-len 3] [--f16] [--reps 10] [--warmup 3]

The fast preset's geometry by default: 100 frames 768², dilations [1, 25], snippets of 3 → 98 + 50 snippets,
f32 (the decoded snippets' dtype there), seeded so that every run sees the same data.  HIP events, the median
of `reps` after `warmup` calls, for
  * rdmi_aligner_merge         (kernels.aligner_merge: the mean alone),
  * rdmi_aligner_merge_moments (kernels.aligner_merge_moments: the mean and the spread in one pass),
  * rdmi_aligner_merge_median  (kernels.aligner_merge_median: the per-pixel median, without and with the MAD;
    --call median, which also times rdmi_aligner_merge_moments — it reads the same snippet bytes — as the
    yardstick and prints the ratios).
--call picks one of them, so that a job script can run each under its own `timeout`.  --dilations may repeat
a value and --snippet-len sets the snippets' length: eight dilations of 1 at length 8 put 64 terms on a pixel.
Bytes are algorithmic: every snippet slot is read once (Σ n_d · w · HW elements) and each output map written
once (N · HW · 4 B: one map for the merge and the median alone, two for the fused calls).  The two means are
compared bitwise.
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
    ap.add_argument("--call", choices=["merge", "moments", "both", "median"], default="both")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--dilations", type=int, nargs="+", default=[1, 25])
    ap.add_argument("--snippet-len", type=int, default=3)
    ap.add_argument("--f16", action="store_true", help="f16 snippets merged in f32 arithmetic (x_f32 = 2)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    from rollingdepth_amd import kernels as K

    dev = torch.device("cuda", 0)
    N, HW, w = a.frames, a.res * a.res, a.snippet_len
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
        "median": ("rdmi_aligner_merge_median", reads + N * HW * 4,
                   lambda: K.aligner_merge_median(xf, sc, tr, a.dilations, N, shift, f32_arith=True)),
        "median_mad": ("rdmi_aligner_merge_median + MAD", reads + 2 * N * HW * 4,
                       lambda: K.aligner_merge_median(xf, sc, tr, a.dilations, N, shift, f32_arith=True, mad=True)),
    }
    picked = {"merge": ["merge"], "moments": ["moments"], "both": ["merge", "moments"],
              "median": ["moments", "median", "median_mad"]}[a.call]
    mean = K.aligner_merge(xf, sc, tr, a.dilations, N, shift, f32_arith=True)
    mean2, std = K.aligner_merge_moments(xf, sc, tr, a.dilations, N, shift, f32_arith=True)
    print(f"{N} x {a.res}^2, dilations {a.dilations}, {' + '.join(map(str, counts))} snippets of {w}, "
          f"{'f16' if a.f16 else 'f32'} snippets; means bitwise equal {torch.equal(mean, mean2)}; "
          f"std mean {std.mean().item():.6f} max {std.max().item():.6f}")
    if a.call == "median":
        med, mad = K.aligner_merge_median(xf, sc, tr, a.dilations, N, shift, f32_arith=True, mad=True)
        print(f"median differs from the mean at {(med != mean).float().mean().item():.3f} of the pixels; "
              f"MAD mean {mad.mean().item():.6f} max {mad.max().item():.6f}")
        del med, mad
    del mean, mean2, std
    print("| call | ms (median) | min .. max | bytes | TB/s |")
    print("|---|---|---|---|---|")
    rows = []
    for key in picked:
        name, nbytes, fn = runs[key]
        med, lo, hi = timed(fn, a.reps, a.warmup)
        rows.append({"call": name, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                     "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e9, 3)})
        print(f"| {name} | {med:.3f} | {lo:.3f} .. {hi:.3f} | {nbytes} | {nbytes / med / 1e9:.2f} |", flush=True)
    if a.call == "median":
        base = rows[0]["ms"]
        print("against rdmi_aligner_merge_moments: " +
              ", ".join(f"{r['call']} {r['ms'] / base:.2f}x" for r in rows[1:]))
    print(json.dumps({"tool": "merge_probe", "frames": N, "res": a.res, "dilations": a.dilations,
                      "snippets": counts, "snippet_len": w,
                      "f16": a.f16, "reps": a.reps, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
