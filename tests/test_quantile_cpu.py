"""CPU side of the device quantiles (percentile renormalisation): the shared key / rank / pick header under
sanitizers, the new library symbols and their checks, which return before any launch, the Python argument checks
that run before any device work, and the reference of tests/quantile_util.py against numpy."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdmi_select_hist", "rdmi_select_pick", "rdmi_quantiles", "rdmi_renormalize_clip_f32", "rdmi_select_bins",
       "rdmi_select_passes", "rdmi_select_state_bytes", "rdmi_quantiles_workspace")


def test_select_key_header_under_sanitizers(tmp_path):
    """csrc/select_key.h in a stand-alone program built with AddressSanitizer + UBSan (linked statically, nothing
    preloaded): key order and inverse on the edge values, the shared zero key, the digits, the histogram walk
    (first / last bin, boundaries, one bin, counts above 2^32), the rank rule at cnt = 1 and 2^40, and a whole
    digit-by-digit select."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/select_key_check.cpp"
    exe = str(tmp_path / "select_key_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "select_key_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and " cases" in r.stdout, r.stdout


def test_new_symbols_load_and_version():
    from rollingdepth_amd import _native as N_
    from rollingdepth_amd import kernels as K

    for name in NEW:
        assert name in N_.EXPORTED and callable(getattr(N_.lib, name))
    assert N_.lib.rdmi_version() >= 9
    bins, passes = K.select_bins(), K.select_passes()
    assert bins >= 2 and bins & (bins - 1) == 0 and bins ** passes == 1 << 32  # the digits tile the 32-bit key
    assert N_.lib.rdmi_select_state_bytes() % 8 == 0
    assert N_.lib.rdmi_quantiles_workspace() >= N_.lib.rdmi_select_state_bytes() + passes * 4 * bins * 8
    hdr = open(os.path.join(ROOT, "include", "rdmi.h")).read()
    assert "#define RDMI_SELECT_MAX 4" in hdr and K.SELECT_MAX == 4


def test_library_checks_run_before_any_launch():
    """Null pointers, n ≤ 0, k outside 1 … 4 and a pass outside its range are RDMI_E_ARG in all four entry points —
    on a machine without a GPU, so nothing can have been launched.  The pointers are never dereferenced."""
    from rollingdepth_amd import _native as N_

    lib, x = N_.lib, 4096  # x: a non-null, 16-byte aligned pointer value
    P = lib.rdmi_select_passes()
    hist = lambda x_=x, n=8, st=x, p=0, k=2, h=x: lib.rdmi_select_hist(x_, 1, None, n, st, p, k, h, None)  # noqa: E731
    pick = lambda h=x, q=x, p=0, k=2, st=x, o=x: lib.rdmi_select_pick(h, q, p, k, st, o, None)  # noqa: E731
    quant = lambda x_=x, n=8, q=x, k=2, o=x, ws=x: lib.rdmi_quantiles(x_, 0, None, n, q, k, o, ws, None)  # noqa: E731
    bad = {
        "hist null x": hist(x_=None), "hist null state": hist(st=None), "hist null hist": hist(h=None),
        "hist n 0": hist(n=0), "hist n < 0": hist(n=-3), "hist k 0": hist(k=0), "hist k 5": hist(k=5),
        "hist pass -1": hist(p=-1), "hist pass P": hist(p=P),
        "pick null hist": pick(h=None), "pick null q": pick(q=None), "pick null state": pick(st=None),
        "pick null out": pick(o=None), "pick k 0": pick(k=0), "pick k 5": pick(k=5), "pick pass -1": pick(p=-1),
        "pick pass P": pick(p=P),
        "quantiles null x": quant(x_=None), "quantiles null q": quant(q=None), "quantiles null out": quant(o=None),
        "quantiles null workspace": quant(ws=None), "quantiles n 0": quant(n=0), "quantiles k 0": quant(k=0),
        "quantiles k 5": quant(k=5),
        "clip null x": lib.rdmi_renormalize_clip_f32(None, 4, x, None),
        "clip null lohi": lib.rdmi_renormalize_clip_f32(x, 4, None, None),
        "clip n 0": lib.rdmi_renormalize_clip_f32(x, 0, x, None),
    }
    assert all(rc == 1001 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc != 1001}
    assert hist(k=5) == 1001 and b"k 5" in lib.rdmi_last_error()
    assert pick(p=P) == 1001 and f"pass {P}".encode() in lib.rdmi_last_error()


@pytest.mark.parametrize("bad", [(2,), (98, 2), (-1, 50), (0, 100.5), (True, 50), "2,98", (50, 50), (2, 98, 99),
                                 (float("nan"), 50), 5, (2, "98")])
def test_check_renorm_percentiles_rejects(bad):
    from rollingdepth_amd.colorize import colorize_depth_multi_thread
    from rollingdepth_amd.pipeline import RollingDepthPipeline, check_renorm_percentiles
    from rollingdepth_amd.shard import sharded_forward

    with pytest.raises(ValueError, match="renorm_percentiles"):
        check_renorm_percentiles(bad)
    # before any device work: forward's `self` is never touched, the frames stay on the host
    with pytest.raises(ValueError, match="renorm_percentiles"):
        RollingDepthPipeline.forward(None, torch.zeros((1, 5, 3, 8, 8)), [1], True, [3], [1], [1], None, 0, 3, 6, None,
                                     False, 4, False, renorm_percentiles=bad)
    with pytest.raises(ValueError, match="renorm_percentiles"):
        RollingDepthPipeline.__call__(None, torch.zeros((5, 3, 8, 8)), renorm_percentiles=bad)
    with pytest.raises(ValueError, match="renorm_percentiles"):
        sharded_forward(None, torch.zeros((5, 3, 8, 8)), [1], renorm_percentiles=bad)
    with pytest.raises(ValueError, match="renorm_percentiles"):
        colorize_depth_multi_thread(np.zeros((2, 1, 4, 4), np.float32), percentiles=bad, device="cpu")


def test_check_renorm_percentiles_accepts_and_defaults():
    from rollingdepth_amd.colorize import colorize_depth_multi_thread
    from rollingdepth_amd.pipeline import RollingDepthPipeline, check_renorm_percentiles
    from rollingdepth_amd.shard import sharded_forward

    assert check_renorm_percentiles(None) is None
    assert check_renorm_percentiles((2, 98)) == (2.0, 98.0) and check_renorm_percentiles([0.0, 100.0]) == (0.0, 100.0)
    assert check_renorm_percentiles((np.float32(0.5), 99)) == (0.5, 99.0)
    for fn in (RollingDepthPipeline.forward, RollingDepthPipeline.__call__, RollingDepthPipeline._forward_sharded,
               sharded_forward):
        assert inspect.signature(fn).parameters["renorm_percentiles"].default is None, fn
    assert inspect.signature(colorize_depth_multi_thread).parameters["percentiles"].default is None


def test_call_forwards_the_argument_only_when_set():
    """__call__ hands renorm_percentiles to forward only when it is not None, so a subclass or spy whose forward
    predates the keyword keeps working."""
    from rollingdepth_amd.pipeline import RollingDepthPipeline

    seen = []

    class Stop(Exception):
        pass

    class Spy(RollingDepthPipeline):
        def __init__(self):
            pass

        def forward(self, *a, **kw):
            seen.append(kw)
            raise Stop  # before any output handling

    for val, want in ((None, False), ((2.0, 98.0), True)):
        with pytest.raises(Stop):
            Spy()(torch.zeros((5, 3, 8, 8)), renorm_percentiles=val)
        assert ("renorm_percentiles" in seen[-1]) is want
    assert seen[-1]["renorm_percentiles"] == (2.0, 98.0)


def test_quantiles_wrapper_checks_before_device_work():
    import rollingdepth_amd
    from rollingdepth_amd import kernels as K

    assert rollingdepth_amd.quantiles is K.quantiles
    x = torch.zeros(8)
    for q in ([], [0.1] * 5, [-0.1], [1.5], [True], ["0.5"], [float("nan")]):
        with pytest.raises(ValueError, match="quantile"):
            K.quantiles(x, q)
    for q in (0.5, "0.5", torch.tensor([0.5])):
        with pytest.raises(TypeError, match="sequence"):
            K.quantiles(x, q)
    for dt in (torch.float64, torch.int32, torch.bfloat16):
        with pytest.raises(TypeError, match="f16/f32"):
            K.quantiles(x.to(dt), [0.5])
    with pytest.raises(ValueError, match="device tensor"):
        K.quantiles(x, [0.5])
    with pytest.raises(ValueError, match="device tensor"):
        K.select_hist(x, x, 0, 1, torch.zeros((1, K.select_bins()), dtype=torch.int64))
    with pytest.raises(ValueError, match="device tensor"):
        K.renormalize_clip_(x, torch.zeros(2))
    x2 = torch.zeros((2, 4))
    with pytest.raises(TypeError, match="mask must be bool or uint8"):
        K.quantiles(x2, [0.5], mask=torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="mask shape"):
        K.quantiles(x2, [0.5], mask=torch.zeros((4, 2), dtype=torch.bool))
    with pytest.raises(ValueError, match="mask on"):
        K.quantiles(x2, [0.5], mask=torch.zeros((2, 4), dtype=torch.bool, device="meta"))


@pytest.mark.parametrize("n", [1, 5, 101, 4097])
def test_reference_against_numpy_lower(n):
    """Where n − 1 is divisible by 4 the percentiles 0, 25, 50, 100 have exact ranks in both formulas: the
    reference is numpy's method="lower"."""
    from tests import quantile_util as Q

    rng = np.random.default_rng(n)
    for dt in (np.float32, np.float16):
        x = (rng.standard_normal(n) * 3).astype(dt)
        got = Q.select(x, [0.0, 0.25, 0.5, 1.0])
        want = np.percentile(x.astype(np.float32), [0, 25, 50, 100], method="lower").astype(np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert [Q.rank(q, n) for q in (0.0, 0.25, 0.5, 1.0)] == [0, (n - 1) // 4, (n - 1) // 2, n - 1]


def test_reference_edges():
    from tests import quantile_util as Q

    inf = np.float32(np.inf)
    v = np.array([np.nan, -inf, -1.0, -0.0, 0.0, 1e-45, 1.0, inf, np.nan], np.float32)
    k = Q.keys(v[1:-1])
    assert np.all(np.diff(k.astype(np.int64)) >= 0) and k[2] == k[3] == 0x80000000
    assert np.array_equal(Q.values(k)[[0, 1, 4, 5, 6]], v[[1, 2, 5, 6, 7]])
    # NaNs are skipped: 7 values remain, ranks 0, 3, 6
    got = Q.select(v, [0.0, 0.5, 1.0])
    assert got[0] == -inf and got[2] == inf and got[1] == 0 and not np.signbit(got[1])
    assert np.isnan(Q.select(v, [0.5], mask=np.zeros(9, bool))).all()
    assert Q.select(v, [0.0, 1.0], mask=np.arange(9) == 6).tolist() == [1.0, 1.0]
    x = np.array([0.0, 1.0, 2.0, 3.0, 10.0], np.float32)
    assert Q.renorm_clip(x, 1.0, 3.0).tolist() == [-1.0, -1.0, 0.0, 1.0, 1.0]
