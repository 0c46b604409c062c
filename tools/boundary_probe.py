"""Time boundary_metrics beside depth_metrics, and score the plain resize against the edge-aware restore (one GPU).

    python tools/boundary_probe.py [--frames 16] [--reps 20] [--warmup 3] [--timeout 240] [--log profiles/boundary_probe.log]

Per shape one child process under its own `timeout`, started by a parent that never opens the GPU and stops at the
first child that fails.

(a) Timing, 768 × 768 and 1080 × 1920, `frames` frames, f16 pred, f32 target, with and without a u8 mask; the scene is
    a smooth field with steps, the prediction the same scene with 3 % noise, whose neighbours often differ by more
    than the lowest thresholds, so the kernel meets edges at every threshold; one more row times the kernel on the
    same scene with 0.3 % noise, where only the steps are edges.  Each call is warmed up, then HIP events around every
    call and the median of `reps`:
      * boundary_metrics(align="video") and depth_metrics(align="video") as a user calls them (allocation, the
        launches, the copies of the small results to the host and their synchronisation included), in the same run on
        the same inputs.  Both read the operands twice — the moments pass and their own pass — so depth_metrics is the
        yardstick, and the GB/s of both are 2 · (2 + 4 [+ 1]) bytes per pixel over the time;
      * their own passes alone, enqueued on the device: rdmi_depth_boundary (with and without the edge map, which
        adds one byte written per pixel) and rdmi_depth_errors, each reading the operands once.
(b) First use, 576 × 1024 → 1080 × 1920 and 432 × 768 → 1080 × 1920 (the upsample probe's shapes), 4 frames: the truth
    is a full-resolution depth — a step scene, and smooth fields plus steps — the input its bilinear downsample, the
    guide an image that follows the depth plus texture and 8-bit noise.  boundary_metrics(align="none") of the plain
    bilinear resize and of guided_upsample at its defaults, each against the truth.  Synthetic scenes: no real video
    and no trained weights have run.

Everything printed also goes to --log; one JSON line at the end."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIME_SHAPES = [(768, 768), (1080, 1920)]
UP_SHAPES = [(576, 1024, 1080, 1920), (432, 768, 1080, 1920)]
UP_FRAMES = 4


def timed(fn, reps, warmup):
    import torch

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


def depth_video(n, H, W, dev, smooth=True):
    """f32 [n, H, W] in about [1, 4]: a vertical and a slanted step that drift from frame to frame, on a constant or
    (smooth) on a slowly varying field."""
    import torch

    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None] / H
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :] / W
    out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    for i in range(n):
        d = torch.full((H, W), 1.5, device=dev)
        if smooth:
            d = d + 0.4 * torch.sin(2 * math.pi * (1.5 * xs + 0.05 * i)) * torch.cos(2 * math.pi * ys) + 0.5 * ys
        d = d * (1.0 + 0.6 * (xs >= 0.4 + 0.01 * i).float()) * (1.0 + 0.3 * ((xs + 0.5 * ys) >= 0.9).float())
        out[i] = d
    return out


def child_time(a):
    import torch

    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.metrics import DEFAULT_BOUNDARY_THRESHOLDS, boundary_metrics, depth_metrics

    H, W = a.shape
    n, dev = a.frames, torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(3)
    target = depth_video(n, H, W, dev)
    pred = (0.25 + 0.5 * target * torch.exp(0.03 * torch.randn((n, H, W), generator=gen, device=dev))).half()
    mask = (torch.rand((n, H, W), generator=gen, device=dev) < 0.8).to(torch.uint8)
    calm = (0.25 + 0.5 * target * torch.exp(0.003 * torch.randn((n, H, W), generator=gen, device=dev))).half()
    P = H * W
    p2, g2, c2 = pred.view(n, P), target.view(n, P), calm.view(n, P)
    tau = list(DEFAULT_BOUNDARY_THRESHOLDS)
    rows = []
    for m in (None, mask):
        m2 = None if m is None else m.view(n, P)
        px_bytes = 6 + (m is not None)
        ws = K.depth_metrics_workspace(n, P, dev)
        _, st = K.depth_fit(K.depth_moments(p2, g2, m2, 1e-3, math.inf, ws), n, P, K.DEPTH_FIT_MODES["video"])
        got = boundary_metrics(pred, target, m)
        runs = [
            ("boundary_metrics(align='video')", lambda: boundary_metrics(pred, target, m), 2 * px_bytes),
            ("depth_metrics(align='video')", lambda: depth_metrics(pred, target, m), 2 * px_bytes),
            ("rdmi_depth_boundary", lambda: K.depth_boundary(p2, g2, m2, st, H, W, tau), px_bytes),
            ("rdmi_depth_boundary + edge map", lambda: K.depth_boundary(p2, g2, m2, st, H, W, tau, edge_index=5),
             px_bytes + 1),
            ("rdmi_depth_errors", lambda: K.depth_errors(p2, g2, m2, st, 1e-3, math.inf, ws=ws), px_bytes),
            ("rdmi_depth_boundary, 0.3 % noise", lambda: K.depth_boundary(c2, g2, m2, st, H, W, tau), px_bytes),
        ]
        for name, fn, b in runs:
            med, lo, hi = timed(fn, a.reps, a.warmup)
            rows.append({"H": H, "W": W, "frames": n, "mask": m is not None, "call": name, "ms": round(med, 4),
                         "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": b * n * P, "f1": got.f1,
                         "edge_share": float(got.counts[:, 0, :, 2].sum()) / max(got.n_pairs, 1)})
    print("ROWS " + json.dumps(rows), flush=True)


def child_up(a):
    import torch

    from rollingdepth_amd import kernels as K
    from rollingdepth_amd.metrics import boundary_metrics
    from rollingdepth_amd.upsample import guided_upsample

    h, w, H, W = a.shape
    n, dev = UP_FRAMES, torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = []
    for scene, smooth in (("step", False), ("smooth + step", True)):
        truth = depth_video(n, H, W, dev, smooth)[:, None].contiguous()
        ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None] / H
        xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :] / W
        frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        for c in range(3):  # an image that follows the depth: brighter where nearer, plus texture and ±2 levels of noise
            f = 0.85 - 0.2 * truth[:, 0] + 0.03 * torch.sin(2 * math.pi * (7 * xs + 5 * ys + 0.3 * c))
            f = f * 255 + (torch.rand((n, H, W), generator=gen, device=dev) * 4 - 2)
            frames[..., c] = f.clamp(0, 255).round().to(torch.uint8)
        low = K.resize(truth, (h, w), "BILINEAR")
        for method, up in (("resize", K.resize(low, (H, W), "BILINEAR")), ("joint_bilateral", guided_upsample(low, frames))):
            m = boundary_metrics(up, truth, align="none")
            rows.append({"h": h, "w": w, "H": H, "W": W, "frames": n, "scene": scene, "method": method, "f1": m.f1,
                         "precision": m.precision, "recall": m.recall, "n_pairs": m.n_pairs,
                         "f1_per_threshold": [round(v, 4) for v in m.f1_per_threshold.tolist()]})
        best = boundary_metrics(truth, truth, align="none")
        rows.append({"h": h, "w": w, "H": H, "W": W, "frames": n, "scene": scene, "method": "truth against itself",
                     "f1": best.f1, "precision": best.precision, "recall": best.recall, "n_pairs": best.n_pairs,
                     "f1_per_threshold": [round(v, 4) for v in best.f1_per_threshold.tolist()]})
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "boundary_probe.log"))
    ap.add_argument("--shape", type=int, nargs="+", default=None, help="child mode: H W (timing) or h w H W (first use)")
    a = ap.parse_args()
    if a.shape is not None:
        return child_time(a) if len(a.shape) == 2 else child_up(a)

    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def run_child(shape):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--frames",
               str(a.frames), "--reps", str(a.reps), "--warmup", str(a.warmup), "--shape", *map(str, shape)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [l for l in p.stdout.splitlines() if l.startswith("ROWS ")]
        if p.returncode != 0 or not got:
            say(f"{' x '.join(map(str, shape))}: child ended with status {p.returncode}; nothing more is started")
            say(p.stdout[-2000:] + p.stderr[-2000:])
            return None, p.returncode or 1
        return json.loads(got[-1][5:]), 0

    say(f"(a) boundary_metrics beside depth_metrics: {a.frames} frames, f16 pred, f32 target, 10 thresholds; median of "
        f"{a.reps} after {a.warmup} warm-up calls, HIP events; GB/s from the algorithmic bytes")
    say("| H x W | mask | call | ms (median) | min .. max | GB/s | x depth_metrics | x rdmi_depth_errors |")
    say("|---|---|---|---|---|---|---|---|")
    timing, scores, rc = [], [], 0
    for shape in TIME_SHAPES:
        rows, rc = run_child(shape)
        if rows is None:
            break
        for q in rows:
            same = [r for r in rows if r["mask"] == q["mask"]]
            dm = next(r for r in same if r["call"].startswith("depth_metrics"))["ms"]
            de = next(r for r in same if r["call"] == "rdmi_depth_errors")["ms"]
            q.update(gbs=round(q["bytes"] / q["ms"] / 1e6, 1), x_depth_metrics=round(q["ms"] / dm, 3),
                     x_depth_errors=round(q["ms"] / de, 3))
            timing.append(q)
            say(f"| {q['H']} x {q['W']} | {'u8' if q['mask'] else 'none'} | {q['call']} | {q['ms']:.3f} | {q['ms_min']:.3f} .. "
                f"{q['ms_max']:.3f} | {q['gbs']:.0f} | {q['x_depth_metrics']:.2f} | {q['x_depth_errors']:.2f} |")
        say(f"  ({shape[0]} x {shape[1]}: target edges at the lowest threshold on {rows[0]['edge_share']:.4f} of the "
            f"directed pairs without a mask; f1 of the noisy prediction {rows[0]['f1']:.4f})")
    if rc == 0:
        say()
        say(f"(b) first use, synthetic scenes, {UP_FRAMES} frames: the bilinear downsample of a full-resolution truth "
            "brought back by the plain resize and by guided_upsample (defaults), scored against the truth, align none")
        say("| h x w -> H x W | scene | method | f1 | precision | recall | f1 at 1.05 .. 1.25 |")
        say("|---|---|---|---|---|---|---|")
        for shape in UP_SHAPES:
            rows, rc = run_child(shape)
            if rows is None:
                break
            for q in rows:
                scores.append(q)
                say(f"| {q['h']} x {q['w']} -> {q['H']} x {q['W']} | {q['scene']} | {q['method']} | {q['f1']:.4f} | "
                    f"{q['precision']:.4f} | {q['recall']:.4f} | {q['f1_per_threshold'][0]:.3f} .. "
                    f"{q['f1_per_threshold'][-1]:.3f} |")
    say(json.dumps({"tool": "boundary_probe", "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
                    "timing": timing, "scores": scores}))
    log.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
