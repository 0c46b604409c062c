"""Time the device quantiles against the streaming floor they replace and against a full sort (one GPU).

    python tools/quantile_probe.py [--frames 100] [--res 768] [--reps 10] [--warmup 3]

An f32 map [frames, res, res] (the fast preset's merged video by default) with two contents:
  * pipeline-like: a smooth depth ramp in about [0.1, 1.9] with pixel noise and a few hundred stray pixels far
    outside — in pass 0 of the radix select nearly every element falls into two exponent bins;
  * constant: every element 1.0, the worst case for the counting atomics (one bin in every pass).
HIP events, the median of `reps` after `warmup` calls, for
  * kernels.quantiles(x, [0.02, 0.98]): zero + select_passes() × (count + pick), no host sync,
  * kernels.minmax(x): the one-pass streaming reduction the percentile range replaces,
  * torch.sort of the flattened map: the only stock way to the same numbers at this size (torch.quantile refuses
    more than 16 M elements).
Bytes are algorithmic: select_passes() · 4 B per element for the quantiles, 4 B per element for minmax, 8 B (read +
write of the values alone) for the sort.  Then each counting pass (select_hist) and each pick (select_pick, less the
state copy that restores its input) alone, through the split form.  The two values are checked against the sorted map at the ranks
floor(q · (n − 1)) before anything is timed.  One JSON line at the end.
"""
import argparse
import json
import math
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
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    from rollingdepth_amd import kernels as K

    dev = torch.device("cuda", 0)
    N, R = a.frames, a.res
    n = N * R * R
    g = torch.Generator(device=dev).manual_seed(0)
    ramp = torch.linspace(0.1, 1.8, R, device=dev).view(1, R, 1).expand(N, R, R)
    like = (ramp + 0.1 * torch.rand((N, R, R), generator=g, device=dev)).contiguous()
    stray = torch.randint(0, n, (300,), generator=g, device=dev)
    like.view(-1)[stray] = torch.where(torch.arange(300, device=dev) % 2 == 0, -40.0, 55.0)
    inputs = {"pipeline-like": like, "constant": torch.full((N, R, R), 1.0, device=dev)}
    q = [0.02, 0.98]
    passes = K.select_passes()
    rows = []
    print(f"{N} x {R}^2 f32 = {n} elements; {passes} passes of {K.select_bins()} bins")
    print("| input | call | us (median) | min .. max | bytes | TB/s |")
    print("|---|---|---|---|---|---|")
    for name, x in inputs.items():
        got = K.quantiles(x, q).tolist()
        srt = torch.sort(x.view(-1)).values
        want = [srt[int(math.floor(f * (n - 1)))].item() for f in q]
        del srt
        assert got == want, (name, got, want)
        mm = K.minmax(x).tolist()
        print(f"{name}: min / max {mm[0]:.4f} / {mm[1]:.4f}, percentiles 2 / 98 {got[0]:.6f} / {got[1]:.6f} "
              "(equal to the sorted map's)")
        runs = {
            "quantiles k=2": (lambda: K.quantiles(x, q), passes * 4 * n),
            "minmax": (lambda: K.minmax(x), 4 * n),
            "torch.sort": (lambda: torch.sort(x.view(-1)), 8 * n),
        }
        for call, (fn, nbytes) in runs.items():
            med, lo, hi = timed(fn, a.reps, a.warmup)
            rows.append({"input": name, "call": call, "us": round(med * 1e3, 1), "us_min": round(lo * 1e3, 1),
                         "us_max": round(hi * 1e3, 1), "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e9, 3)})
            print(f"| {name} | {call} | {med * 1e3:.1f} | {lo * 1e3:.1f} .. {hi * 1e3:.1f} | {nbytes} | "
                  f"{nbytes / med / 1e9:.2f} |", flush=True)
        # where the time goes: each counting pass and each pick alone, through the split form (the state a pass
        # reads is the one the passes before it left; a timed pick runs on a restored copy of the state)
        k, qd, state = len(q), K.select_q(q, dev), K.select_state(dev)
        out = torch.empty(k, device=dev)
        scratch = torch.zeros((k, K.select_bins()), dtype=torch.int64, device=dev)
        for p in range(passes):
            med, lo, hi = timed(lambda: K.select_hist(x, state, p, k, scratch), a.reps, a.warmup)
            hist = torch.zeros_like(scratch)
            K.select_hist(x, state, p, k, hist)
            saved = state.clone()
            pm, _, _ = timed(lambda: (state.copy_(saved), K.select_pick(hist, qd, p, k, state, out)), a.reps, 1)
            cm, _, _ = timed(lambda: state.copy_(saved), a.reps, 1)
            state.copy_(saved)
            K.select_pick(hist, qd, p, k, state, out)
            rows.append({"input": name, "call": f"select_hist pass {p}", "us": round(med * 1e3, 1),
                         "us_min": round(lo * 1e3, 1), "us_max": round(hi * 1e3, 1), "bytes": 4 * n,
                         "tb_per_s": round(4 * n / med / 1e9, 3), "pick_us": round((pm - cm) * 1e3, 1)})
            print(f"| {name} | select_hist pass {p} | {med * 1e3:.1f} | {lo * 1e3:.1f} .. {hi * 1e3:.1f} | {4 * n} | "
                  f"{4 * n / med / 1e9:.2f} | + select_pick {(pm - cm) * 1e3:.1f} us", flush=True)
        assert out.tolist() == got
    t = {(r["input"], r["call"]): r["us"] for r in rows}
    for name in inputs:
        print(f"{name}: quantiles / ({passes} x minmax) = {t[name, 'quantiles k=2'] / (passes * t[name, 'minmax']):.2f}, "
              f"torch.sort / quantiles = {t[name, 'torch.sort'] / t[name, 'quantiles k=2']:.1f}")
    print(f"constant / pipeline-like quantiles = {t['constant', 'quantiles k=2'] / t['pipeline-like', 'quantiles k=2']:.2f}")
    print(json.dumps({"tool": "quantile_probe", "frames": N, "res": R, "reps": a.reps, "warmup": a.warmup,
                      "passes": passes, "rows": rows}))


if __name__ == "__main__":
    main()
