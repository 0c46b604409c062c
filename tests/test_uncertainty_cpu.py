"""CPU side of the merge's per-pixel spread (depth_uncertainty): the new library symbols and their checks,
which return before any launch, the Python argument checks that run before any device work, and the
reference of tests/uncertainty_util.py on a hand-worked example."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

NEW = ("rdmi_aligner_merge_moments", "rdmi_aligner_merge_partial_window_moments",
       "rdmi_aligner_merge_finish_pieces_moments", "rdmi_scale_spread_f32")


def test_new_symbols_load_and_version():
    from rollingdepth_amd import _native as N_

    for name in NEW:
        assert name in N_.EXPORTED and callable(getattr(N_.lib, name))
    assert N_.lib.rdmi_version() >= 6


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def test_library_checks_run_before_any_launch():
    """N = 14, dilation 3, length 3, start step 2 → starts 0 2 4 6 7, 5 snippets.  A wrong count, a zero start
    step and a null output are RDMI_E_ARG in all three merge calls — on a machine without a GPU, so nothing
    can have been launched.  The pointers are never dereferenced."""
    from rollingdepth_amd import _native as N_

    lib, x = N_.lib, 4096  # x: a non-null, 16-byte aligned pointer value
    xp, n5, n4, st, ss2, ss0, w, z = _ptrs(x), _ints(5), _ints(4), _ints(3), _ints(2), _ints(0), _ints(3), _ints(0)
    fused = lambda n, ss, mean, std: lib.rdmi_aligner_merge_moments(  # noqa: E731
        1, xp, 1, xp, xp, n, st, ss, w, 14, 64, x, mean, std, None)
    part = lambda n, ss, nloc, mom: lib.rdmi_aligner_merge_partial_window_moments(  # noqa: E731
        1, xp, 1, xp, xp, n, st, ss, z, nloc, w, 14, 0, 14, 64, x, mom, None)
    fin = lambda n, ss, mean, std, nf=14: lib.rdmi_aligner_merge_finish_pieces_moments(  # noqa: E731
        1, n, st, ss, w, 14, 0, nf, 64, 1, _ints(0), _ints(nf), x, mean, std, None)
    bad = {
        "fused count": fused(n4, ss2, x, x),
        "fused zero step": fused(n5, ss0, x, x),
        "fused null mean": fused(n5, ss2, None, x),
        "fused null std": fused(n5, ss2, x, None),
        "fused null steps": fused(n5, None, x, x),
        "partial count": part(n4, ss2, n4, x),
        "partial zero step": part(n5, ss0, n5, x),
        "partial null out": part(n5, ss2, n5, None),
        "partial window past the sequence": lib.rdmi_aligner_merge_partial_window_moments(
            1, xp, 1, xp, xp, n5, st, ss2, z, n5, w, 14, 1, 14, 64, x, x, None),
        "finish count": fin(n4, ss2, x, x),
        "finish zero step": fin(n5, ss0, x, x),
        "finish null mean": fin(n5, ss2, None, x),
        "finish null std": fin(n5, ss2, x, None),
        "finish empty chunk, wrong count": fin(n4, ss2, None, None, 0),
        "scale null x": lib.rdmi_scale_spread_f32(None, 4, x, None),
        "scale null minmax": lib.rdmi_scale_spread_f32(x, 4, None, None),
        "scale n": lib.rdmi_scale_spread_f32(x, 0, x, None),
    }
    assert all(rc == 1001 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc != 1001}
    assert fused(n4, ss2, x, x) == 1001 and b"gives 5" in lib.rdmi_last_error()
    # the start-step-1 layout is checked too (N = 14, dilation 3, length 3: 8 snippets)
    assert fused(n5, _ints(1), x, x) == 1001 and b"gives 8" in lib.rdmi_last_error()
    # an empty frame chunk with a right layout needs no outputs and launches nothing
    assert fin(n5, ss2, None, None, 0) == 0


def test_kernels_wrappers_check_their_arguments():
    from rollingdepth_amd import kernels as K

    x = [torch.zeros((5, 3, 2, 2))]
    one = [torch.ones(5)]
    sh = torch.zeros(1)
    with pytest.raises(ValueError, match="start steps"):
        K.aligner_merge_moments(x, one, one, [3], 14, sh, start_steps=[2, 2])
    with pytest.raises(ValueError, match="start steps"):
        K.aligner_merge_partial_window_moments(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, start_steps=[])
    with pytest.raises(ValueError, match=r"\[nf, 2, HW\]"):
        K.aligner_merge_partial_window_moments(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14,
                                               out=torch.zeros((14, 4), dtype=torch.float64))
    with pytest.raises(TypeError, match="f64"):
        K.aligner_merge_finish_pieces_moments(torch.zeros((14, 2, 4)), [(0, 14)], [5], [3], [3], 0, 14, 4, 14)
    with pytest.raises(ValueError, match="device tensor"):
        K.scale_spread_(torch.zeros(4), torch.zeros(2))


def test_run_and_forward_argument_checks():
    """uncertainty / output_uncertainty are keywords defaulting to False and must be bools: TypeError before
    any device work (the aligner's device here is the CPU; forward's `self` is never touched)."""
    from rollingdepth_amd.aligner import DepthAligner
    from rollingdepth_amd.pipeline import RollingDepthOutput, RollingDepthPipeline, check_output_uncertainty
    from rollingdepth_amd.shard import _merge_windowed, sharded_forward

    assert inspect.signature(DepthAligner.run).parameters["uncertainty"].default is False
    for fn in (RollingDepthPipeline.forward, RollingDepthPipeline.__call__, sharded_forward):
        assert inspect.signature(fn).parameters["output_uncertainty"].default is False
    assert inspect.signature(_merge_windowed).parameters["moments"].default is False
    assert RollingDepthOutput(None, None, None, None).depth_uncertainty is None
    for bad in (1, 0, None, "yes", torch.ones(1)):
        with pytest.raises(TypeError, match="output_uncertainty"):
            check_output_uncertainty(bad)
        with pytest.raises(TypeError, match="uncertainty"):
            DepthAligner(device="cpu").run([torch.zeros((3, 3, 1, 4, 4))], [1], uncertainty=bad)
        with pytest.raises(TypeError, match="output_uncertainty"):
            RollingDepthPipeline.forward(None, torch.zeros((1, 5, 3, 8, 8)), [1], True, [3], [1], [1], None, 0, 3, 6,
                                         None, False, 4, False, output_uncertainty=bad)
        with pytest.raises(TypeError, match="output_uncertainty"):
            RollingDepthPipeline.__call__(None, torch.zeros((5, 3, 8, 8)), output_uncertainty=bad)
        with pytest.raises(TypeError, match="output_uncertainty"):
            sharded_forward(None, torch.zeros((5, 3, 8, 8)), [1], output_uncertainty=bad)
    assert check_output_uncertainty(True) is True and check_output_uncertainty(False) is False


def test_reference_on_a_hand_worked_example():
    """N = 5, dilation 1, length 3 → 3 snippets; frame 2 is covered by (k 0, slot 2), (k 1, slot 1) and
    (k 2, slot 0).  With shift 0:  2·0.5 + 0 = 1,  1·1.5 + 0.5 = 2,  0.5·5 + 0.5 = 3  →  mean 2, population
    std √(2/3).  Frame 0 has the one term 2·0.5 + 0 = 1 (std 0), frame 1 the two terms 2·7 + 0 = 14 and
    1·3 + 0.5 = 3.5 → std 5.25."""
    from tests import uncertainty_util as U

    x = np.zeros((3, 3, 1), np.float32)
    x[0, 2], x[1, 1], x[2, 0] = 0.5, 1.5, 5.0
    x[0, 1], x[1, 0], x[0, 0] = 7.0, 3.0, 0.5
    s = [np.array([2.0, 1.0, 0.5], np.float32)]
    t = [np.array([0.0, 0.5, 0.5], np.float32)]
    assert U.starts(5, 3, 1, 1) == [0, 1, 2] and U.starts(14, 3, 3, 2) == [0, 2, 4, 6, 7]
    fr = U.frame_terms([x], s, t, [1], [1], 5, 0.0, 1)
    assert [a.shape[0] for a in fr] == [1, 2, 3, 2, 1]
    assert fr[2][:, 0].tolist() == [1.0, 2.0, 3.0]  # slot descending = snippet ascending
    assert fr[1][:, 0].tolist() == [14.0, 3.5]
    ref, tol, cnt = U.spread_reference(fr)
    assert cnt.tolist() == [1, 2, 3, 2, 1]
    assert ref[0, 0] == 0 and ref[1, 0] == 5.25
    assert abs(float(ref[2, 0]) - math.sqrt(2.0 / 3.0)) < 1e-15
    # tol = 2⁻²²·ref + E / ref with E = 7·2⁻⁵²·9 at frame 2; √E where ref = 0
    E = 7 * 2.0 ** -52 * 9.0
    assert abs(float(tol[2, 0]) - (2.0 ** -22 * math.sqrt(2 / 3) + E / math.sqrt(2 / 3))) < 1e-20
    assert abs(float(tol[0, 0]) - math.sqrt(5 * 2.0 ** -52 * 1.0)) < 1e-20
    # the f16 chain of mode 0 rounds every step through f16: 0.1·3 + 0.2 in f16
    a = U.terms(np.array([3.0], np.float16), np.float32(0.1), np.float32(0.2), 0.0, 0)
    h = np.float16
    assert a.dtype == np.float32 and a[0] == np.float32(h(np.float32(h(np.float32(3.0) * np.float32(h(0.1))))
                                                          + np.float32(h(0.2))))
    # the one-pass f64 formula of the kernel stays inside tol here, a sample std does not
    al = fr[2][:, 0].astype(np.float64)
    one_pass = math.sqrt(max(0.0, (al * al).sum() / 3 - (al.sum() / 3) ** 2))
    assert U.worst_ratio(np.array([[np.float32(one_pass)]]), ref[2:3, :1], tol[2:3, :1])[0] <= 1.0
    assert U.worst_ratio(np.array([[np.float32(1.0)]]), ref[2:3, :1], tol[2:3, :1])[0] > 1.0  # ÷ (c − 1)
