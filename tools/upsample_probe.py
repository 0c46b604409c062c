"""Time joint bilateral upsampling against the bilinear resize of the same maps (one GPU).

    python tools/upsample_probe.py [--frames 16] [--reps 20] [--warmup 3] [--timeout 240] [--log profiles/upsample_probe.log]

Shapes: 576 × 1024 → 1080 × 1920 and 432 × 768 → 1080 × 1920, `frames` frames, uint8 [N, H, W, 3] guide, f32 values;
radius 1, 2, 3 and C = 1, 2.  Per shape one child process under its own `timeout`, started by a parent that never
opens the GPU and stops at the first child that fails.  In a child, in one run: kernels.joint_bilateral_upsample and
kernels.resize(values, (H, W), "BILINEAR") on the same values, each warmed up, then HIP events around every call and
the median of `reps`.  The guide is a smooth field plus steps and 8-bit noise (so the weights are neither all 1 nor
all 0), guide_lo the device's bilinear resize of it in [0, 1] — built outside the timed calls, as is the guide.

Columns: ms per call; ns per output pixel (all C channels); the ratio to the bilinear resize of the same C maps;
Gtap/s = N·H·W·(2r)² taps over the time; GB/s = the algorithmic HBM bytes (3 guide bytes read and 4·C written per
output pixel, (3·4 + C·4) bytes read per low-resolution pixel) over the time.  Everything printed also goes to --log;
one JSON line at the end."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(576, 1024, 1080, 1920), (432, 768, 1080, 1920)]


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


def guide_video(n, H, W, dev):
    """uint8 [n, H, W, 3]: a smooth field, two steps (one vertical, one slanted) and ±2 levels of noise."""
    import torch

    g = torch.Generator(device=dev).manual_seed(7)
    ys = torch.arange(H, device=dev, dtype=torch.float32)[:, None] / H
    xs = torch.arange(W, device=dev, dtype=torch.float32)[None, :] / W
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    for i in range(n):
        for c in range(3):
            f = 0.35 + 0.12 * torch.sin(2 * math.pi * (3 * xs + 0.1 * i + 0.3 * c)) * torch.cos(2 * math.pi * 2 * ys)
            f = f + 0.3 * (xs >= 0.4 + 0.01 * i).float() + 0.2 * ((xs + 0.5 * ys) >= 0.9).float()
            f = f * 255 + (torch.rand((H, W), generator=g, device=dev) * 4 - 2)
            out[i, :, :, c] = f.clamp(0, 255).round().to(torch.uint8)
    return out


def child(a):
    import torch

    from rollingdepth_amd import kernels as K

    h, w, H, W = a.shape
    n = a.frames
    dev = torch.device("cuda", 0)
    guide = guide_video(n, H, W, dev)
    guide_lo = K.resize(guide, (h, w), "BILINEAR", channels_last=True).mul_(1.0 / 255.0)
    gen = torch.Generator(device=dev).manual_seed(11)
    rows = []
    for C in (1, 2):
        values = torch.rand((n, C, h, w), generator=gen, device=dev) * 2 - 1
        out = torch.empty((n, C, H, W), dtype=torch.float32, device=dev)
        res = torch.empty((n, C, H, W), dtype=torch.float32, device=dev)
        bil = timed(lambda: K.resize(values, (H, W), "BILINEAR", out=res), a.reps, a.warmup)
        for r in (1, 2, 3):
            jbu = timed(lambda: K.joint_bilateral_upsample(values, guide_lo, guide, r, 1.0, 0.1, out=out), a.reps,
                        a.warmup)
            bil2 = timed(lambda: K.resize(values, (H, W), "BILINEAR", out=res), a.reps, a.warmup)
            rows.append({"h": h, "w": w, "H": H, "W": W, "frames": n, "C": C, "radius": r, "jbu_ms": round(jbu[0], 4),
                         "jbu_min": round(jbu[1], 4), "jbu_max": round(jbu[2], 4),
                         "bilinear_ms": round(min(bil[0], bil2[0]), 4), "bilinear_ms_before": round(bil[0], 4),
                         "bilinear_ms_after": round(bil2[0], 4)})
            bil = bil2
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "upsample_probe.log"))
    ap.add_argument("--shape", type=int, nargs=4, default=None, help="child mode: h w H W")
    a = ap.parse_args()
    if a.shape is not None:
        return child(a)

    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say(f"joint bilateral upsampling vs the bilinear resize, {a.frames} frames, u8 guide, f32 values, sigma_spatial 1, "
        f"sigma_range 0.1; median of {a.reps} after {a.warmup} warm-up calls, HIP events")
    say("| h x w -> H x W | C | r | jbu ms (median) | min .. max | ns / output px | bilinear ms | jbu / bilinear | Gtap/s | GB/s |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    rows, rc = [], 0
    for h, w, H, W in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--frames",
               str(a.frames), "--reps", str(a.reps), "--warmup", str(a.warmup), "--shape", str(h), str(w), str(H), str(W)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [l for l in p.stdout.splitlines() if l.startswith("ROWS ")]
        if p.returncode != 0 or not got:
            rc = p.returncode or 1
            say(f"{h} x {w} -> {H} x {W}: child ended with status {p.returncode}; nothing more is started")
            say(p.stdout[-2000:] + p.stderr[-2000:])
            break
        for q in json.loads(got[-1][5:]):
            px = q["frames"] * H * W
            taps = px * (2 * q["radius"]) ** 2
            nbytes = px * (3 + 4 * q["C"]) + q["frames"] * h * w * (12 + 4 * q["C"])
            q.update(ns_per_px=round(q["jbu_ms"] * 1e6 / px, 4), ratio=round(q["jbu_ms"] / q["bilinear_ms"], 3),
                     gtaps=round(taps / q["jbu_ms"] / 1e6, 1), gbs=round(nbytes / q["jbu_ms"] / 1e6, 1))
            rows.append(q)
            say(f"| {h} x {w} -> {H} x {W} | {q['C']} | {q['radius']} | {q['jbu_ms']:.3f} | {q['jbu_min']:.3f} .. "
                f"{q['jbu_max']:.3f} | {q['ns_per_px']:.4f} | {q['bilinear_ms']:.3f} | {q['ratio']:.2f} | {q['gtaps']:.0f} | "
                f"{q['gbs']:.0f} |")
    say(json.dumps({"tool": "upsample_probe", "frames": a.frames, "reps": a.reps, "warmup": a.warmup, "rows": rows}))
    log.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
