"""Time the optical-flow chain (one GPU) and set it next to one fast-preset pipeline step.

    python tools/flow_probe.py [--res 768 1024] [--pairs 1 8 32] [--reps 5] [--warmup 2] [--log profiles/flow_probe.log]

For each resolution and pair count, on f16 frames [pairs + 1, 3, res, res] of a moving plane-wave texture (a smooth
flow of a few pixels, zoom included): HIP events, the median of `reps` after `warmup` calls, for
  * kernels.flow_estimate with the defaults (radius 5, 3 iterations, the level rule, both directions and the
    forward–backward check): luma + pyramid, two Lucas–Kanade launches per level, one check;
  * the same without the backward flow;
  * the pyramid alone, and the level-0 Lucas–Kanade launch alone (one direction) — where the time goes.
Taps: the level-0 launch reads (2r + 1)² · 4 taps of the moving image per pixel and iteration through the caches;
"Gtap/s" is that count over the launch's time.  The comparison figure is ms_per_step of the newest BENCH_*.json in the
repository root (bench.py's fast preset: 100 frames of 768²), if there is one.  Everything printed also goes to --log;
one JSON line at the end.
"""
import argparse
import glob
import json
import math
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def texture_video(n, res, dev):
    """n frames [n, 3, res, res] f16: 12 plane waves, frame i shifted by i·(1.5, 1.0) px and zoomed by 1.01^-i."""
    g = torch.Generator().manual_seed(1)
    fx, fy = ((torch.rand(12, generator=g, dtype=torch.float64) * 2 - 1) * 0.6 for _ in range(2))
    ph = torch.rand(12, generator=g, dtype=torch.float64) * 2 * math.pi
    fx, fy, ph = (t.to(dev).float() for t in (fx, fy, ph))
    ys, xs = torch.meshgrid(torch.arange(res, device=dev).float(), torch.arange(res, device=dev).float(), indexing="ij")
    c = (res - 1) / 2
    out = torch.empty((n, 3, res, res), dtype=torch.float16, device=dev)
    for i in range(n):
        z = 1.01 ** -i
        X, Y = (xs - c) * z + c - 1.5 * i, (ys - c) * z + c - 1.0 * i
        t = torch.zeros_like(X)
        for k in range(12):
            t += torch.sin(X * fx[k] + Y * fy[k] + ph[k])
        t /= 6
        for ch, gain in enumerate((1.0, 0.8, 0.6)):
            out[i, ch] = (gain * t).half()
    return out


def bench_step_ms():
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "BENCH_*.json"))):
        try:
            m = re.findall(r'"ms_per_step":\s*([0-9.]+)', open(path).read().replace('\\"', '"'))
        except OSError:
            continue
        if m:
            best = (os.path.basename(path), float(m[-1]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[768, 1024])
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "flow_probe.log"))
    a = ap.parse_args()

    from rollingdepth_amd import kernels as K

    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda", 0)
    r, its = 5, 3
    step = bench_step_ms()
    rows = []
    say(f"optical-flow chain, radius {r}, {its} iterations, f16 frames; median of {a.reps} after {a.warmup} warm-up calls")
    say("| res | pairs | levels | call | ms (median) | min .. max | ms / pair | Gtap/s |")
    say("|---|---|---|---|---|---|---|---|")
    for res in a.res:
        lv = K.flow_levels(res, res, r)
        for pairs in a.pairs:
            x = texture_video(pairs + 1, res, dev)
            flow, _, valid = K.flow_estimate(x)
            torch.cuda.synchronize()
            share = valid.float().mean().item()
            pyr = K.flow_pyramid(x, lv)
            coarse = None
            for l in range(lv - 1, 0, -1):
                coarse = K.flow_lk_level(pyr[l], 0, 1, pairs, coarse, r, its)
            taps = pairs * res * res * (2 * r + 1) ** 2 * 4 * its
            runs = {
                "estimate, both directions + check": (lambda: K.flow_estimate(x), None),
                "estimate, forward only": (lambda: K.flow_estimate(x, backward=False), None),
                "pyramid": (lambda: K.flow_pyramid(x, lv), None),
                "lk level 0, one direction": (lambda: K.flow_lk_level(pyr[0], 0, 1, pairs, coarse, r, its), taps),
            }
            for call, (fn, ntaps) in runs.items():
                med, lo, hi = timed(fn, a.reps, a.warmup)
                rate = "" if ntaps is None else f"{ntaps / med / 1e6:.0f}"
                rows.append({"res": res, "pairs": pairs, "levels": lv, "call": call, "ms": round(med, 3),
                             "ms_min": round(lo, 3), "ms_max": round(hi, 3), "valid_share": round(share, 4)})
                say(f"| {res} | {pairs} | {lv} | {call} | {med:.3f} | {lo:.3f} .. {hi:.3f} | {med / pairs:.3f} | {rate} |")
            say(f"{res}^2, {pairs} pairs: mean |flow| {flow.norm(dim=-1).mean().item():.2f} px, valid share {share:.3f}")
            del x, flow, valid, pyr, coarse
    if step:
        t = {(w["res"], w["pairs"]): w["ms"] for w in rows if w["call"].startswith("estimate, both")}
        say(f"one fast-preset step ({step[0]}): {step[1]:.1f} ms for 100 frames of 768^2")
        for (res, pairs), ms in t.items():
            say(f"{res}^2: flow + mask for 99 pairs at the {pairs}-pair rate = {99 * ms / pairs:.1f} ms = "
                f"{99 * ms / pairs / step[1]:.3f} of that step")
    else:
        say("no BENCH_*.json found: no pipeline step to compare with")
    line = json.dumps({"tool": "flow_probe", "radius": r, "iterations": its, "reps": a.reps, "warmup": a.warmup,
                       "bench_step": step, "rows": rows})
    say(line)
    log.close()


if __name__ == "__main__":
    main()
