"""Reference fixtures for snippet strides > 1 (generation needs the read-only reference, see _refload.py).

    python tests/golden/make_golden_strided.py [--only idx,aligner]

  snippet_indices_strided.json        the reference's static get_snippet_indice for the strided
                                      aligner layouts of tests/test_strided_*.py and the fast-preset
                                      geometry (N = 100, dilations [1, 25], strides [1, 5] and [2, 5])
  aligner_strided.safetensors (+ .json)
                                      the reference's DepthAligner.optimize + merge_scaled_triplets called
                                      with strided index tensors (its run() only builds stride-1 ones):
                                      N = 20, 64², dilations (1, 4), lengths (3, 3), strides (2, 3),
                                      2000 iterations — the preparation of run() (min shift, border
                                      crop, subsample, depth_aligner.py:78-92) is restated here
                                      (snippets stored as f16, exactly: they are rounded to f16 values
                                      before the f32 run; load them with .float())
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from safetensors.torch import save_file  # noqa: E402

import _refload  # noqa: E402

# (N, dilations, snippet lengths, strides)
LAYOUTS = [
    (14, (1, 3), (3, 3), (2, 2)),
    (14, (1, 3), (3, 3), (1, 3)),
    (14, (1, 3), (3, 3), (3, 1)),
    (15, (1, 3), (3, 3), (2, 5)),
    (14, (1, 3), (3, 2), (2, 3)),
    (14, (1, 3, 2), (4, 2, 2), (1, 2, 3)),
    (9, (1, 2), (3, 3), (2, 2)),
    (9, (1, 2), (3, 3), (1, 3)),
    (9, (1, 2), (3, 3), (3, 1)),
    (14, (1, 3), (3, 3), (1, 20)),
    (100, (1, 25), (3, 3), (1, 5)),
    (100, (1, 25), (3, 3), (2, 5)),
]


def _c(t):
    return t.detach().to(torch.float32).contiguous().clone()


def index_fixture(P):
    RDP = P.RollingDepthPipeline
    res = []
    for N, dil, lens, steps in LAYOUTS:
        idx = [RDP.get_snippet_indice(0, torch.tensor([999]), N, w, d, d, s) for d, w, s in zip(dil, lens, steps)]
        res.append({"N": N, "dilations": list(dil), "snippet_lengths": list(lens), "strides": list(steps),
                    "indices": idx})
    json.dump(res, open(os.path.join(HERE, "snippet_indices_strided.json"), "w"))
    print("strided indices:", [[len(i) for i in r["indices"]] for r in res])


def aligner_fixture(P, A, name="aligner_strided", N=20, H=64, Wd=64, dil=(1, 4), lengths=(3, 3), steps=(2, 3), seed=3,
                    iters=2000):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((N, 1, H, Wd), generator=g) * 2 - 1
    RDP = P.RollingDepthPipeline
    idx = [torch.tensor(RDP.get_snippet_indice(0, torch.tensor([999]), N, w, d, d, s))
           for d, w, s in zip(dil, lengths, steps)]
    snips = []
    for ix in idx:
        n = ix.shape[0]
        s = base[ix]  # [n, w, 1, H, W]
        sc = 0.5 + torch.rand((n, 1, 1, 1, 1), generator=g)
        sh = 0.3 * torch.randn((n, 1, 1, 1, 1), generator=g)
        # f16-representable values, stored as f16 and run in f32: the file stays under 1 MiB
        snips.append((s * sc + sh + 0.01 * torch.randn(s.shape, generator=g)).half().float())
    al = A.DepthAligner(device=torch.device("cpu"), num_iterations=iters)
    mn = min(s.min() for s in snips)
    shifted = [s - mn for s in snips]
    sub = [s[:, :, :, al.border:-al.border, al.border:-al.border][:, :, :, ::al.factor, ::al.factor] for s in shifted]
    with contextlib.redirect_stdout(io.StringIO()):  # the reference's optimize prints its shapes
        sc, tr, hist = al.optimize(snippet_ls=sub, indices_list=idx, sequence_length=N)
    merged = al.merge_scaled_triplets(snippet_ls=shifted, indices_list=idx, s_list=sc, t_list=tr, sequence_length=N,
                                      device=torch.device("cpu"))
    out = {f"snippet_{i}": x.half() for i, x in enumerate(snips)}
    out["merged"] = _c(merged)
    for i, (a, b) in enumerate(zip(sc, tr)):
        out[f"scale_{i}"] = _c(a)
        out[f"trans_{i}"] = _c(b)
    out["loss_hist"] = torch.tensor(np.array(hist, dtype=np.float64))
    save_file(out, os.path.join(HERE, name + ".safetensors"))
    json.dump({"dilations": list(dil), "N": N, "H": H, "W": Wd, "iterations": iters, "snippet_lengths": list(lengths),
               "strides": list(steps), "seed": seed, "indices": [ix.tolist() for ix in idx]},
              open(os.path.join(HERE, name + ".json"), "w"))
    print(name, merged.shape, [ix.shape[0] for ix in idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    todo = a.only.split(",") if a.only else ["idx", "aligner"]
    P, A = _refload.load_reference()
    if "idx" in todo:
        index_fixture(P)
    if "aligner" in todo:
        aligner_fixture(P, A, seed=a.seed)


if __name__ == "__main__":
    main()
