"""Snippet strides > 1 (get_snippet_indice's `stride`: snippets start every `stride` frames, plus the
last window), host side: the index map against the reference's own indices, the numpy oracle against
a strided run of the reference's DepthAligner, the shared index header under sanitizers, and the
C-ABI validation, which precedes every HIP call."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from safetensors.torch import load_file

from oracle import rd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_snippet_indices_strided_vs_reference():
    """tests/golden/snippet_indices_strided.json holds the reference's static get_snippet_indice for
    the ten strided aligner layouts and the fast-preset geometry.  The pipeline's get_snippet_indice,
    the oracle's, the Python index map (count, start of snippet k) and create_triplet_indices agree with
    it.  (N = 100, dilations [1, 25]: strides [1, 5] give 98 + 11 snippets, [2, 5] give 50 + 11 — the
    last window, start 97, is appended to range(0, 98, 2).)"""
    import torch
    from rollingdepth_amd.aligner import DepthAligner, snippet_count, snippet_last, snippet_start
    from rollingdepth_amd.pipeline import RollingDepthPipeline as RDP

    cases = json.load(open(os.path.join(G, "snippet_indices_strided.json")))
    assert len(cases) == 12
    counts = {}
    al = DepthAligner(device=torch.device("cpu"))
    for c in cases:
        N = c["N"]
        for d, w, s, ref in zip(c["dilations"], c["snippet_lengths"], c["strides"], c["indices"]):
            assert RDP.get_snippet_indice(0, [999], N, w, d, d, s) == ref
            assert O.snippet_indices(0, 1, N, w, d, d, s) == ref
            assert snippet_count(N, w, d, s) == len(ref)
            assert [snippet_start(k, N, w, d, s) for k in range(len(ref))] == [r[0] for r in ref]
            assert ref[-1][0] == snippet_last(N, w, d) and ref[-1][-1] == N - 1
            assert al.create_triplet_indices(N, d - 1, w, s).tolist() == ref
        counts[(N, tuple(c["strides"]))] = [len(r) for r in c["indices"]]
    assert counts[(100, (1, 5))] == [98, 11]
    assert counts[(100, (2, 5))] == [50, 11]
    assert counts[(14, (1, 20))] == [12, 2]


def _prepared(snips, border=2, factor=10):
    """DepthAligner.run's preparation (depth_aligner.py:78-92): min shift, border crop, subsample."""
    mn = min(float(s.min()) for s in snips)
    shifted = [(s - np.float32(mn)).astype(np.float32) for s in snips]
    sub = [s[:, :, :, border:-border, border:-border][..., ::factor, ::factor] for s in shifted]
    return shifted, [s.reshape(s.shape[0], s.shape[1], -1).astype(np.float32) for s in sub]


def test_aligner_strided_oracle_vs_reference():
    """The oracle with strided index arrays against the reference's DepthAligner.optimize +
    merge_scaled_triplets called with the same strided index tensors (aligner_strided fixture: N = 20,
    64², dilations (1, 4), lengths (3, 3), strides (2, 3), 2000 iterations), with the comparison of
    tests/test_oracle_golden.py::test_aligner_oracle_vs_reference.

    Oracle vs reference when the fixture was made (seed 3): max |Δs| 2.9e-3, max |Δt| 4.9e-4, merged
    mean 1.5e-4 / max 1.4e-3 of the range, loss history 1.3e-7 relative over the first 50 rows, 7.2e-7
    over the first 200 (first row beyond 1e-5: 632) and 3.4e-4 overall — each within half of the bound
    the device test (tests/test_strided_gpu.py) holds against the same fixture."""
    t = load_file(os.path.join(G, "aligner_strided.safetensors"))
    meta = json.load(open(os.path.join(G, "aligner_strided.json")))
    dil, N = meta["dilations"], meta["N"]
    snips = [t[f"snippet_{i}"].float().numpy() for i in range(len(dil))]
    idx = [np.array(O.snippet_indices(0, 1, N, w, d, d, s), np.int64)
           for d, w, s in zip(dil, meta["snippet_lengths"], meta["strides"])]
    assert [ix.tolist() for ix in idx] == meta["indices"]
    shifted, xs = _prepared(snips)
    sc, tr, hist = O.aligner_optimize(xs, idx, N, iters=meta["iterations"])
    merged = O.aligner_merge(shifted, idx, sc, tr, N)
    ref_hist = t["loss_hist"].numpy()
    np.testing.assert_allclose(np.array(hist)[:5], ref_hist[:5], rtol=1e-5)
    np.testing.assert_allclose(np.array(hist)[:200, 0], ref_hist[:200, 0], rtol=1e-5)
    for i in range(len(dil)):
        np.testing.assert_allclose(sc[i], t[f"scale_{i}"].numpy().ravel(), atol=1e-2)
        np.testing.assert_allclose(tr[i], t[f"trans_{i}"].numpy().ravel(), atol=1e-2)
    ref_m = t["merged"].numpy()
    rng = ref_m.max() - ref_m.min()
    assert np.abs(merged - ref_m).mean() <= 1e-3 * rng
    assert np.abs(merged - ref_m).max() <= 5e-3 * rng


def test_aligner_index_header_under_sanitizers(tmp_path):
    """csrc/aligner_index.h (the map the kernels and the host validation share) in a stand-alone
    program built with AddressSanitizer + UBSan: closed form vs brute-force enumeration for every
    N ≤ 40, length ≤ 4, dilation ≤ 6, start step ≤ 8 with N ≥ window.  The sanitizer runtimes are
    linked statically, so the program does not depend on what else the environment preloads."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/aligner_index_check.cpp"
    exe = str(tmp_path / "aligner_index_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "aligner_index_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and "6672 cases" in r.stdout, r.stdout


def test_aligner_workspace_layout_under_sanitizers(tmp_path):
    """csrc/aligner_ws.h (the workspace layout rdmi_aligner_workspace and rdmi_aligner_optimize share) in
    a stand-alone program built with AddressSanitizer + UBSan, sanitizer runtimes linked statically: for
    N ≤ 40, P in {1, 9, 5929}, ntot in {1, 2, 12, 148, 1024}, iters in {0, 1, 20, 128, 129, 2000}, with
    and without a history, every region lies inside the total, the regions are disjoint and in the
    documented order, f64 regions start at even float offsets, m / v / counters are contiguous and the
    total is the closed formula."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/aligner_ws_check.cpp"
    exe = str(tmp_path / "aligner_ws_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "aligner_ws_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and "7200 cases" in r.stdout, r.stdout


def _args(n, start_step, N=14, stride=(1, 3), w=(3, 3), P=9):
    """Aligner arguments with host buffers behind every pointer (never read: the calls below are
    rejected before any launch)."""
    from rollingdepth_amd import _native

    a = _native.AlignerArgs()
    keep = []
    a.n_dil, a.seq_len, a.P, a.iters = len(n), N, P, 1
    for d in range(len(n)):
        bufs = [(C.c_float * 64)() for _ in range(3)]
        keep += bufs
        a.x[d], a.s[d], a.t[d] = (C.addressof(b) for b in bufs)
        a.n[d], a.stride[d], a.w[d] = n[d], stride[d], w[d]
        if start_step is not None:
            a.start_step[d] = start_step[d]
    ws = (C.c_double * 4096)()
    keep.append(ws)
    a.workspace = C.addressof(ws)
    return a, keep


def test_start_step_validation_without_gpu():
    """With a start step > 1, rdmi_aligner_optimize checks the layout against the index map before
    any HIP call: an n[d] other than the map's count, a negative start step and a window longer than
    the sequence are RDMI_E_ARG with a message (N = 14, dilations (1, 3), length 3, start steps (2, 2):
    7 and 5 snippets)."""
    from rollingdepth_amd import _native

    lib = _native.lib
    assert lib.rdmi_version() >= 2
    a, keep = _args([7, 4], [2, 2])  # dilation 3: last = 7 → starts 0 2 4 6 7 = 5 snippets
    assert lib.rdmi_aligner_optimize(C.byref(a), None) == 1001
    msg = lib.rdmi_last_error().decode()
    assert "dilation 1" in msg and "4 snippets" in msg and "gives 5" in msg, msg
    with pytest.raises(_native.RdmiError):
        _native.check(1001, "rdmi_aligner_optimize")
    a, keep = _args([6, 5], [2, 2])
    assert lib.rdmi_aligner_optimize(C.byref(a), None) == 1001
    assert "dilation 0" in lib.rdmi_last_error().decode()
    a, keep = _args([7, 5], [2, -1])
    assert lib.rdmi_aligner_optimize(C.byref(a), None) == 1001
    assert "start step -1" in lib.rdmi_last_error().decode()
    a, keep = _args([2, 1], [2, 2], N=4)  # dilation 3, length 3: a window of 7 frames in 4
    assert lib.rdmi_aligner_optimize(C.byref(a), None) == 1001
    assert "does not fit" in lib.rdmi_last_error().decode()


def test_start_step_workspace(monkeypatch):
    """A zero-initialised start_step (callers built against version 1) and explicit ones leave
    rdmi_aligner_workspace at its value, and the size depends on the arguments alone: the same with
    RDMI_ALIGNER_FUSED unset, 0, 1 and 2 (a caller may size the workspace once and run under another
    setting)."""
    from rollingdepth_amd import _native

    lib = _native.lib
    N, P, PS = 14, 9, 8

    def size(n, ss, hist):
        a, keep = _args(n, ss, N=N, P=P)
        a.iters = 20
        a.history = C.addressof(keep[-1]) if hist else None
        return lib.rdmi_aligner_workspace(C.byref(a))

    def formula(ntot, hist):  # csrc/aligner_ws.h
        f = 8 * ntot * PS + 8 * N * PS + 2 * N * P + 4 * ntot + ((ntot + 1) & ~1) + 4 * 21
        if hist:
            f += 20 * (4 * ntot * PS + 2 * N * PS + 2 * ntot) + 2
        return f + 64

    for mode in (None, "0", "1", "2"):
        if mode is None:
            monkeypatch.delenv("RDMI_ALIGNER_FUSED", raising=False)
        else:
            monkeypatch.setenv("RDMI_ALIGNER_FUSED", mode)
        for hist in (False, True):
            assert size([12, 8], None, hist) == size([12, 8], [1, 1], hist) == formula(20, hist), mode
            assert size([7, 5], [2, 2], hist) == formula(12, hist), mode
