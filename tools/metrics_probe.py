"""Time the depth-metric passes against the existing streaming reduction (one GPU).

    python tools/metrics_probe.py [--frames 100] [--res 768] [--reps 10] [--warmup 3] [--temporal]

f32 pred and target [frames, res, res] with a u8 mask, all on the device.  HIP events, the median of `reps`
after `warmup` calls, for
  * depth_metrics(align="video") as a user calls it (workspace allocation, the three launches, the copies of
    [N, 2] + [N, 8] doubles to the host and their synchronisation included),
  * its device work alone: rdmi_depth_moments → rdmi_depth_fit → rdmi_depth_errors enqueued back to back,
    and each of the two streaming passes alone,
  * kernels.minmax over pred, the streaming reduction the project already had.
Bytes are algorithmic: each metric pass reads pred + target + mask once (9 B per pixel), minmax reads 4 B per
pixel.  --temporal adds rdmi_depth_temporal (frame_step 1, the fit above) without a flow and with a smooth
synthetic one (values on the ¼-pixel grid, |dx|, |dy| ≤ 3): both frames' pred, target and mask per pixel pair
(18 B), plus 8 B of flow.  rdmi_depth_errors in the same run on the same inputs is its yardstick.  One JSON line
at the end.
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
    ap.add_argument("--temporal", action="store_true", help="add the rdmi_depth_temporal rows")
    a = ap.parse_args()

    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.metrics import depth_metrics

    dev = torch.device("cuda", 0)
    N, P = a.frames, a.res * a.res
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.rand((N, a.res, a.res), generator=g, device=dev)
    target = (1.5 * pred + 0.25) * (0.5 + torch.rand((N, a.res, a.res), generator=g, device=dev))
    mask = (torch.rand((N, a.res, a.res), generator=g, device=dev) < 0.75).to(torch.uint8)
    p2, g2, m2 = pred.view(N, P), target.view(N, P), mask.view(N, P)
    ws = K.depth_metrics_workspace(N, P, dev)
    video = K.DEPTH_FIT_MODES["video"]
    _, st = K.depth_fit(K.depth_moments(p2, g2, m2, 1e-3, math.inf, ws), N, P, video)

    def passes():
        K.depth_moments(p2, g2, m2, 1e-3, math.inf, ws)
        _, s = K.depth_fit(ws, N, P, video)
        K.depth_errors(p2, g2, m2, s, 1e-3, math.inf, ws=ws)

    runs = {
        "depth_metrics(align='video')": (lambda: depth_metrics(pred, target, mask, align="video"), 18 * N * P),
        "moments + fit + errors, device only": (passes, 18 * N * P),
        "rdmi_depth_moments": (lambda: K.depth_moments(p2, g2, m2, 1e-3, math.inf, ws), 9 * N * P),
        "rdmi_depth_errors": (lambda: K.depth_errors(p2, g2, m2, st, 1e-3, math.inf, ws=ws), 9 * N * P),
        "minmax (f32 pred)": (lambda: K.minmax(pred), 4 * N * P),
    }
    if a.temporal:
        # a smooth flow: a slow wave over the frame, drifting from pair to pair, rounded to quarter pixels
        y, x = torch.meshgrid(torch.arange(a.res, device=dev) / a.res, torch.arange(a.res, device=dev) / a.res,
                              indexing="ij")
        ph = torch.arange(N - 1, device=dev).view(-1, 1, 1) * 0.1
        dx = 3 * torch.sin(2 * math.pi * y + ph) * torch.cos(2 * math.pi * x)
        dy = 3 * torch.cos(2 * math.pi * y) * torch.sin(2 * math.pi * x + ph)
        flow = (torch.stack([dx, dy], -1) * 4).round() / 4
        assert flow.abs().max() <= 3 and flow.shape == (N - 1, a.res, a.res, 2)
        flow = flow.float().contiguous()

        def temporal(fl):
            return K.depth_temporal(p2, g2, m2, fl, None, st, a.res, a.res, 1, 1e-3, math.inf, ws=ws)

        kept = [float(temporal(fl)[:, 0].sum().item()) / ((N - 1) * P) for fl in (None, flow)]
        print(f"rdmi_depth_temporal keeps {kept[0]:.4f} of the pixel pairs without a flow, {kept[1]:.4f} with it")
        runs["rdmi_depth_temporal, no flow"] = (lambda: temporal(None), 18 * (N - 1) * P)
        runs["rdmi_depth_temporal, smooth flow"] = (lambda: temporal(flow), 26 * (N - 1) * P)
    out = depth_metrics(pred, target, mask, align="video")
    print(f"{N} x {a.res}^2 f32 pred / target, u8 mask; n_valid {out.n_valid}, scale {out.scale[0].item():.6f}, "
          f"shift {out.shift[0].item():.6f}, abs_rel {out.abs_rel:.6f}, delta1 {out.delta1:.6f}")
    print("| call | ms (median) | min .. max | bytes | TB/s |")
    print("|---|---|---|---|---|")
    rows = []
    for name, (fn, nbytes) in runs.items():
        med, lo, hi = timed(fn, a.reps, a.warmup)
        rows.append({"call": name, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                     "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e9, 3)})
        print(f"| {name} | {med:.3f} | {lo:.3f} .. {hi:.3f} | {nbytes} | {nbytes / med / 1e9:.2f} |", flush=True)
    print(json.dumps({"tool": "metrics_probe", "frames": N, "res": a.res, "reps": a.reps, "warmup": a.warmup,
                      "rows": rows}))


if __name__ == "__main__":
    main()
