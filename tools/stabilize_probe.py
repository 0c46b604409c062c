"""What the temporal filter buys and costs, and what it takes (one GPU).

    python tools/stabilize_probe.py [--frames 100] [--size 768] [--timeout 300] [--log profiles/stabilize_probe.log]

Two child processes, each under its own `timeout`, started by a parent that never opens the GPU and stops at the first
child that fails.

quality: a seeded synthetic video of 16 frames of 192 × 256.  A texture and a depth (smooth, plus a step of +1 along a
slanted line) translate together by (1.5, 1.0) px per frame; the prediction is the true depth under a per-frame affine
jitter (scale and shift, σ = 0.01 each) plus pixel noise of σ = 0.02.  Before, and after temporal_filter(pred, frames)
at radius 1, 2, 3 (sigma_time 1, --sigma-depth): flicker and tge of temporal_metrics along the TRUE flow, the f1 of
boundary_metrics and the AbsRel of depth_metrics against the true depth, and the share of valid slots.

timing: `frames` frames of `size`², f32 depth, f32 frames.  Per radius, in chunks as temporal_filter takes them
(stabilize._CHUNK_ELEMS): the flow chain (stabilize.chunk_flow: pyramid, both directions per offset, both checks, the
packing) and rdmi_temporal_filter on the flows so built, each warmed up and then repeated until a window of
--window ms is filled, HIP events around every repetition, the median.  GB/s = the kernel's algorithmic bytes — per
pixel 4 B of d0 (2 B for f16) and 4 B of out, and 8 + 1 + 4 B (flow, valid, one depth sample) per neighbour present
in the video — over its time, beside the 6.3 TB/s HBM rate the part can reach.  No threshold: there is no earlier
version to compare with.  Everything printed also goes to --log; one JSON line at the end."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 6300.0
MOTION = (1.5, 1.0)


def timed(fn, window_ms, warmup=2, min_reps=3, max_reps=200):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    while len(ms) < min_reps or (sum(ms) < window_ms and len(ms) < max_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), len(ms)


def scene(N, H, W, dev, seed=5):
    """frames f32 [N, 3, H, W] in about [−1, 1], the true depth f32 [N, H, W] (> 1) and the true flow [N − 1, H, W, 2]:
    everything is a function of (x − n·dx, y − n·dy)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    fx = ((torch.rand(16, generator=g) * 2 - 1) * 0.6).to(dev)
    fy = ((torch.rand(16, generator=g) * 2 - 1) * 0.6).to(dev)
    ph = (torch.rand(16, generator=g) * 2 * math.pi).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev),
                            torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    frames = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    for n in range(N):
        X, Y = xs - n * MOTION[0], ys - n * MOTION[1]
        tex = torch.sin(X[..., None] * fx + Y[..., None] * fy + ph).sum(-1) / 8
        for c, gain in enumerate((1.0, 0.8, 0.6)):
            frames[n, c] = gain * tex
        smooth = 2.0 + 0.4 * torch.sin(X * 0.031 + 0.5) * torch.cos(Y * 0.023) + 0.2 * torch.sin((X + Y) * 0.017)
        depth[n] = smooth + (X + 0.3 * Y >= 0.55 * W).float()
    flow = torch.empty((N - 1, H, W, 2), dtype=torch.float32, device=dev)
    flow[..., 0], flow[..., 1] = MOTION
    return frames, depth, flow


def quality(a):
    import torch

    import rollingdepth_amd as RD

    dev = torch.device("cuda", 0)
    N, H, W = 16, 192, 256
    frames, truth, flow = scene(N, H, W, dev)
    g = torch.Generator().manual_seed(9)
    s = 1.0 + 0.01 * torch.randn(N, generator=g)
    t = 0.01 * torch.randn(N, generator=g)
    noise = 0.02 * torch.randn((N, H, W), generator=g)
    pred = truth * s.to(dev)[:, None, None] + t.to(dev)[:, None, None] + noise.to(dev)

    def score(p):
        tm = RD.temporal_metrics(p, truth, flow=flow)
        return dict(flicker=tm.flicker, tge=tm.tge, f1=RD.boundary_metrics(p, truth).f1,
                    abs_rel=RD.depth_metrics(p, truth).abs_rel)

    rows = [dict(radius=0, valid=None, **score(pred))]
    for R in (1, 2, 3):
        out, _, valid = RD.temporal_filter(pred, frames, radius=R, sigma_time=1.0, sigma_depth=a.sigma_depth,
                                           return_flow=True)
        rows.append(dict(radius=R, valid=valid.float().mean().item(), **score(out)))
    print("ROWS " + json.dumps(rows), flush=True)


def timing(a):
    import torch

    from rollingdepth_amd import kernels as K
    from rollingdepth_amd import stabilize as S

    dev = torch.device("cuda", 0)
    N, H, W = a.frames, a.size, a.size
    frames, depth, _ = scene(N, H, W, dev)
    depth = depth + 0.02 * torch.randn((N, H, W), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    out = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    rows = []
    for R in (1, 2, 3):
        step = max(1, S._CHUNK_ELEMS // (2 * R * H * W))
        chunks = [(lo, min(lo + step, N)) for lo in range(0, N, step)]
        packs = {}

        def chain():
            for lo, hi in chunks:
                packs[lo] = S.chunk_flow(frames, lo, hi, R)

        def kernel(d):
            for lo, hi in chunks:
                K.temporal_filter(d, packs[lo][0], packs[lo][1], R, 1.0, a.sigma_depth, f0=lo, n=hi - lo,
                                  out=out[lo:hi])

        fl = timed(chain, a.window, warmup=1, min_reps=3)
        k32 = timed(lambda: kernel(depth), a.window, warmup=3, min_reps=10)
        d16 = depth.half()
        k16 = timed(lambda: kernel(d16), a.window, warmup=3, min_reps=10)
        valid = sum(p[1].sum().item() for p in packs.values()) / sum(p[1].numel() for p in packs.values())
        rows.append(dict(radius=R, chunks=len(chunks), flow_ms=fl[0], flow_min=fl[1], flow_max=fl[2], flow_reps=fl[3],
                         f32_ms=k32[0], f32_min=k32[1], f32_max=k32[2], f32_reps=k32[3],
                         f16_ms=k16[0], f16_min=k16[1], f16_max=k16[2], f16_reps=k16[3], valid=valid))
    print("ROWS " + json.dumps(rows), flush=True)


def algorithmic_bytes(N, H, W, R, depth_bytes):
    present = 2 * sum(max(N - k, 0) for k in range(1, R + 1))  # (frame, neighbour) pairs inside the video
    return H * W * (N * (depth_bytes + 4) + present * (8 + 1 + 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--sigma-depth", type=float, default=0.1)
    ap.add_argument("--window", type=float, default=300.0, help="timed window per measurement, ms")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "stabilize_probe.log"))
    ap.add_argument("--part", choices=("quality", "timing"), default=None, help="child mode")
    a = ap.parse_args()
    if a.part is not None:
        return {"quality": quality, "timing": timing}[a.part](a)

    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "w")

    def say(line=""):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def run(part):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--part", part,
               "--frames", str(a.frames), "--size", str(a.size), "--sigma-depth", str(a.sigma_depth), "--window",
               str(a.window)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [l for l in p.stdout.splitlines() if l.startswith("ROWS ")]
        if p.returncode != 0 or not got:
            say(f"{part}: child ended with status {p.returncode}; nothing more is started")
            say(p.stdout[-2000:] + p.stderr[-2000:])
            return p.returncode or 1, None
        return 0, json.loads(got[-1][5:])

    result = {"tool": "stabilize_probe", "frames": a.frames, "size": a.size, "sigma_depth": a.sigma_depth}
    say(f"temporal filter on a synthetic video: 16 frames of 192 x 256, texture and depth move by {MOTION} px per frame, "
        f"a depth step of +1, per-frame affine jitter 0.01 / 0.01, pixel noise 0.02; sigma_time 1, sigma_depth "
        f"{a.sigma_depth}; flicker and tge along the true flow")
    rc, rows = run("quality")
    if rc == 0:
        say("| radius | flicker | tge | boundary f1 | AbsRel | valid slots |")
        say("|---|---|---|---|---|---|")
        for q in rows:
            name = "unfiltered" if q["radius"] == 0 else str(q["radius"])
            share = "" if q["valid"] is None else f"{q['valid']:.3f}"
            say(f"| {name} | {q['flicker']:.5f} | {q['tge']:.5f} | {q['f1']:.4f} | {q['abs_rel']:.5f} | {share} |")
        result["quality"] = rows
        say()
        say(f"{a.frames} frames of {a.size} x {a.size}, f32 frames, chunks of stabilize._CHUNK_ELEMS; median over a window of "
            f"{a.window:.0f} ms of HIP-event timings after warm-up; {HBM_GBS / 1000:.1f} TB/s is the HBM rate the part can reach")
        rc, rows = run("timing")
    if rc == 0:
        say("| radius | launches | flow chain ms (min .. max, reps) | filter f32 ms (min .. max, reps) | GB/s | of HBM | "
            "filter f16 ms | GB/s | valid slots |")
        say("|---|---|---|---|---|---|---|---|---|")
        for q in rows:
            b32 = algorithmic_bytes(a.frames, a.size, a.size, q["radius"], 4)
            b16 = algorithmic_bytes(a.frames, a.size, a.size, q["radius"], 2)
            q.update(f32_bytes=b32, f16_bytes=b16, f32_gbs=b32 / q["f32_ms"] / 1e6, f16_gbs=b16 / q["f16_ms"] / 1e6)
            say(f"| {q['radius']} | {q['chunks']} | {q['flow_ms']:.2f} ({q['flow_min']:.2f} .. {q['flow_max']:.2f}, "
                f"{q['flow_reps']}) | {q['f32_ms']:.3f} ({q['f32_min']:.3f} .. {q['f32_max']:.3f}, {q['f32_reps']}) | "
                f"{q['f32_gbs']:.0f} | {q['f32_gbs'] / HBM_GBS:.2f} | {q['f16_ms']:.3f} | {q['f16_gbs']:.0f} | "
                f"{q['valid']:.3f} |")
        result["timing"] = rows
    say(json.dumps(result))
    log.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
