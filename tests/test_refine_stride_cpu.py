"""Strided refine (`refine_stride`: the refine snippets start several positions apart inside each residue
class mod the step's dilation), host side: the snippet list's properties, the knob's validation, the
shared index header (csrc/refine_index.h) under sanitizers, and the C-ABI validation of the three
strided averaging calls, which precedes every HIP call."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid():
    for N in range(3, 41):
        for w in range(1, 5):
            for d in range(1, N // w + 1):
                for s in range(1, w + 1):
                    yield N, w, d, s


N_CASES = sum(1 for _ in _grid())


def test_refine_snippet_indice_properties():
    """For N 3…40, w 1…4, d 1…N//w, s 1…w: at s = 1 the list sorted by start frame is
    get_snippet_indice(..., stride=1); every snippet is w in-range frames d apart; every frame is
    covered; the order is class-major (class ascending, then position ascending, positions s apart but
    for an appended last window); the count is the closed form."""
    from rollingdepth_amd.pipeline import RollingDepthPipeline as RDP
    from rollingdepth_amd.pipeline import refine_snippet_count, refine_snippet_indice

    for N, w, d, s in _grid():
        idx = refine_snippet_indice(N, w, d, s)
        key = (N, w, d, s)
        if s == 1:
            assert sorted(idx) == RDP.get_snippet_indice(0, [0], N, w, d, d, 1), key
        for sn in idx:
            assert len(sn) == w and 0 <= sn[0] and sn[-1] < N, key
            assert all(b - a == d for a, b in zip(sn, sn[1:])), key
        assert {f for sn in idx for f in sn} == set(range(N)), key
        order = [(sn[0] % d, sn[0] // d) for sn in idx]
        assert order == sorted(set(order)), key
        for r in range(d):
            pos = [m for c, m in order if c == r]
            last = len(range(r, N, d)) - w
            want = list(range(0, last + 1, s))
            assert pos == want + ([last] if want[-1] < last else []), key
        assert len(idx) == refine_snippet_count(N, w, d, s), key
    # the issue's example of what get_snippet_indice's own stride leaves out, covered here
    assert {f for sn in RDP.get_snippet_indice(0, [0], 20, 3, 4, 4, 2) for f in sn} != set(range(20))
    assert {f for sn in refine_snippet_indice(20, 3, 4, 2) for f in sn} == set(range(20))
    # a class too short for a window has no snippet (N = 7, w = 3, d = 3: lengths 3, 2, 2)
    assert refine_snippet_indice(7, 3, 3, 2) == [[0, 3, 6]] and refine_snippet_count(7, 3, 3, 2) == 1
    assert refine_snippet_indice(11, 3, 2, 2) == [[0, 2, 4], [4, 6, 8], [6, 8, 10], [1, 3, 5], [5, 7, 9]]


def test_refine_stride_validation():
    """check_refine_stride accepts 1 … refine_snippet_len and raises ValueError for 0, w + 1, a bool and a
    float; forward / __call__ / sharded_forward take the knob as a trailing keyword defaulting to 1."""
    from rollingdepth_amd.pipeline import RollingDepthPipeline as RDP
    from rollingdepth_amd.pipeline import check_refine_stride
    from rollingdepth_amd.shard import sharded_forward

    w = 3
    assert [check_refine_stride(s, w) for s in (1, 2, 3)] == [1, 2, 3]
    for bad in (0, w + 1, True, 2.0, -1, None, "2"):
        with pytest.raises(ValueError):
            check_refine_stride(bad, w)
    for fn in (RDP.__call__, RDP.forward, RDP._forward_sharded, sharded_forward):
        p = inspect.signature(fn).parameters["refine_stride"]
        assert p.default == 1, fn
    assert inspect.signature(RDP.refine).parameters["start_step"].default == 1
    # the positional order that mirrors the reference is untouched
    names = list(inspect.signature(RDP.forward).parameters)
    assert names[1:15] == ["input_frames", "dilations", "cap_dilation", "snippet_lengths", "init_infer_steps", "strides",
                           "coalign_kwargs", "refine_step", "refine_snippet_len", "refine_start_dilation", "generator",
                           "verbose", "max_vae_bs", "unload_snippet"]


def test_refine_index_header_under_sanitizers(tmp_path):
    """csrc/refine_index.h (the map the strided averaging kernels and their host validation share) in a
    stand-alone program built with AddressSanitizer + UBSan, the sanitizer runtimes linked statically:
    over the grid above, the closed-form start → index lookup (frames outside the sequence included) and
    the closed-form index → start lookup against brute-force enumeration, and the kernels' cover count."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/refine_index_check.cpp"
    exe = str(tmp_path / "refine_index_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "refine_index_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and f"{N_CASES} cases" in r.stdout, r.stdout


def test_strided_average_validation_without_gpu():
    """The three strided calls check start_step (1 … w) and the row count against the index map before
    any HIP call: RDMI_E_ARG with a message (host buffers behind the pointers, never read)."""
    from rollingdepth_amd import _native

    lib = _native.lib
    assert lib.rdmi_version() >= 4
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    N, w, d, P, c, ld = 11, 3, 2, 1, 4, 8  # start step 2: 3 + 2 snippets
    for ss in (0, w + 1, -2):
        assert lib.rdmi_snippet_average_strided(p, 5, w, d, ss, N, P, c, ld, p, 0, None) == 1001
        assert f"start step {ss}" in lib.rdmi_last_error().decode()
        assert lib.rdmi_snippet_accumulate_strided(p, 0, 0, 5, w, d, ss, N, P, c, ld, p, None) == 1001
        assert f"start step {ss}" in lib.rdmi_last_error().decode()
        assert lib.rdmi_snippet_finish_strided(p, 5, w, d, ss, N, P, c, ld, p, 0, None) == 1001
        assert f"start step {ss}" in lib.rdmi_last_error().decode()
    assert lib.rdmi_snippet_average_strided(p, 6, w, d, 2, N, P, c, ld, p, 0, None) == 1001
    assert "gives 5" in lib.rdmi_last_error().decode()
    assert lib.rdmi_snippet_finish_strided(p, 4, w, d, 2, N, P, c, ld, p, 0, None) == 1001
    assert "gives 5" in lib.rdmi_last_error().decode()
    assert lib.rdmi_snippet_accumulate_strided(p, 0, 3, 3, w, d, 2, N, P, c, ld, p, None) == 1001
    assert "gives 5" in lib.rdmi_last_error().decode()
    with pytest.raises(_native.RdmiError):
        _native.check(1001, "rdmi_snippet_average_strided")
