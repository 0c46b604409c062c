"""CPU side of the median merge (merge="median"): the new library symbols and their checks, which return
before any launch, the Python argument checks that run before any device work, shard.terms_exchange_plan
against brute-force enumeration, and the reference of tests/median_util.py on a hand-worked example."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

NEW = ("rdmi_aligner_merge_median", "rdmi_aligner_merge_partial_window_terms", "rdmi_aligner_median_rows")

# (N, dilations, lengths, start steps): tests/test_uncertainty_gpu.py's four, and the two of test_median_gpu.py
LAYOUTS = {"on": (23, (1, 4, 7), (3, 2, 2), (2, 3, 5)),
           "off": (23, (1, 4, 7), (3, 2, 2), (3, 4, 2)),
           "gap": (14, (1,), (3,), (4,)),
           "one": (23, (1, 4, 7), (3, 2, 2), (1, 1, 1)),
           "wide": (23, tuple(range(1, 9)), (3,) * 8, (1,) * 8),
           "full": (23, (1,) * 8, (8,) * 8, (1,) * 8)}


def test_new_symbols_load_and_version():
    from rollingdepth_amd import _native as N_

    for name in NEW:
        assert name in N_.EXPORTED and callable(getattr(N_.lib, name))
    assert N_.lib.rdmi_version() >= 7


def _ints(*v):
    return (C.c_int * len(v))(*v)


def _ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def test_library_checks_run_before_any_launch():
    """N = 14, dilation 3, length 3, start step 2 → starts 0 2 4 6 7, 5 snippets of 3 slots: 15 terms over
    the 14 frames.  Every bad argument is RDMI_E_ARG (1001) — on a machine without a GPU, so nothing can have
    been launched.  The pointers are never dereferenced."""
    from rollingdepth_amd import _native as N_

    lib, x = N_.lib, 4096  # x: a non-null, 16-byte aligned pointer value
    xp, n5, n4, st, ss2, ss0, w, z = _ptrs(x), _ints(5), _ints(4), _ints(3), _ints(2), _ints(0), _ints(3), _ints(0)
    fused = lambda n, ss, med, mad: lib.rdmi_aligner_merge_median(  # noqa: E731
        1, xp, 1, xp, xp, n, st, ss, w, 14, 64, x, med, mad, None)
    terms = lambda n, ss, nloc, rows, nf=14, k0=z: lib.rdmi_aligner_merge_partial_window_terms(  # noqa: E731
        1, xp, 1, xp, xp, n, st, ss, k0, nloc, w, 14, 0, nf, 64, x, x, rows, x, None)
    sel = lambda nf, mc, med=x: lib.rdmi_aligner_median_rows(x, 4, x, x, nf, 64, mc, med, x, None)  # noqa: E731
    bad = {
        "fused count": fused(n4, ss2, x, x),
        "fused zero step": fused(n5, ss0, x, x),
        "fused null steps": fused(n5, None, x, x),
        "fused null med": fused(n5, ss2, None, x),
        "fused null med, no mad": fused(n5, ss2, None, None),
        "terms count": terms(n4, ss2, n4, 12),
        "terms zero step": terms(n5, ss0, n5, 15),
        "terms null steps": terms(n5, None, n5, 15),
        "terms null k0": terms(n5, ss2, n5, 15, k0=None),
        "terms one row short": terms(n5, ss2, n5, 14),
        "terms one row long": terms(n5, ss2, n5, 16),
        "terms rows of all snippets for two of them": terms(n5, ss2, _ints(2), 15),
        "terms rows for an empty window": terms(n5, ss2, n5, 1, nf=0),
        "terms window past the sequence": lib.rdmi_aligner_merge_partial_window_terms(
            1, xp, 1, xp, xp, n5, st, ss2, z, n5, w, 14, 1, 14, 64, x, x, 15, x, None),
        "rows max_count 0": sel(3, 0),
        "rows max_count 65": sel(3, 65),
        "rows negative nf": sel(-1, 8),
        "rows null med": sel(3, 8, None),
        "rows max_count 0, no frames": sel(0, 0),
    }
    assert all(rc == 1001 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc != 1001}
    assert fused(n4, ss2, x, x) == 1001 and b"gives 5" in lib.rdmi_last_error()
    # the start-step-1 layout is checked too (N = 14, dilation 3, length 3: 8 snippets)
    assert fused(n5, _ints(1), x, x) == 1001 and b"gives 8" in lib.rdmi_last_error()
    assert terms(n4, ss2, n4, 12) == 1001 and b"gives 5" in lib.rdmi_last_error()
    assert terms(n5, ss2, n5, 14) == 1001 and b"hold 15 terms" in lib.rdmi_last_error()
    # snippets 0 and 1 alone (starts 0, 2) hold 6 terms
    assert terms(n5, ss2, _ints(2), 5) == 1001 and b"hold 6 terms" in lib.rdmi_last_error()
    # nothing to do: an empty window with no rows, a rank without snippets, no frames — no launch, no outputs
    assert terms(n5, ss2, n5, 0, nf=0) == 0
    assert terms(n5, ss2, z, 0) == 0
    assert lib.rdmi_aligner_median_rows(None, 0, None, None, 0, 64, 8, None, None, None) == 0


def test_kernels_wrappers_check_their_arguments():
    from rollingdepth_amd import kernels as K

    x = [torch.zeros((5, 3, 2, 2))]
    one = [torch.ones(5)]
    sh = torch.zeros(1)
    off = torch.zeros(15, dtype=torch.int32)
    out = torch.zeros((15, 4))
    with pytest.raises(ValueError, match="start steps"):
        K.aligner_merge_median(x, one, one, [3], 14, sh, start_steps=[2, 2])
    for bad in (1, None, "yes"):
        with pytest.raises(TypeError, match="mad"):
            K.aligner_merge_median(x, one, one, [3], 14, sh, mad=bad)
        with pytest.raises(TypeError, match="mad"):
            K.aligner_median_rows(out, off, off, 14, 8, mad=bad)
    with pytest.raises(ValueError, match="start steps"):
        K.aligner_merge_partial_window_terms(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, off, out,
                                             start_steps=[])
    with pytest.raises(ValueError, match=r"\[rows, HW\]"):
        K.aligner_merge_partial_window_terms(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, off,
                                             torch.zeros((15, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[rows, HW\]"):
        K.aligner_merge_partial_window_terms(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, off,
                                             torch.zeros((15, 5)))
    with pytest.raises(ValueError, match=r"\[nf \+ 1\]"):
        K.aligner_merge_partial_window_terms(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, off[:14], out)
    with pytest.raises(ValueError, match=r"\[nf \+ 1\]"):
        K.aligner_merge_partial_window_terms(x, [0], [5], one, one, [3], [3], 0, 14, 4, sh, 1, 14, off.long(), out)
    with pytest.raises(ValueError, match=r"\[n_rows, HW\]"):
        K.aligner_median_rows(out.double(), off, off, 14, 8)
    with pytest.raises(ValueError, match="row_idx"):
        K.aligner_median_rows(out, off, off.long(), 14, 8)
    with pytest.raises(ValueError, match="frame_off holds"):
        K.aligner_median_rows(out, off, off, 13, 8)
    for mc in (0, 65, -1):
        with pytest.raises(ValueError, match="max_count"):
            K.aligner_median_rows(out, off, off, 14, mc)


def test_merge_keyword_checks():
    """merge is a keyword defaulting to "mean"; anything but "mean" / "median" is a ValueError before any device
    work (the aligner's device here is the CPU; forward's `self` is never touched)."""
    from rollingdepth_amd.aligner import DepthAligner
    from rollingdepth_amd.pipeline import RollingDepthPipeline, check_merge
    from rollingdepth_amd.shard import _merge_windowed, sharded_forward

    for fn in (DepthAligner.run, RollingDepthPipeline.forward, RollingDepthPipeline.__call__, sharded_forward,
               RollingDepthPipeline._forward_sharded):
        assert inspect.signature(fn).parameters["merge"].default == "mean"
    for name in ("median", "mad"):
        assert inspect.signature(_merge_windowed).parameters[name].default is False
    for bad in ("Median", None, True, 1, "", b"median", ["median"]):
        with pytest.raises(ValueError, match="merge must be"):
            check_merge(bad)
        with pytest.raises(ValueError, match="merge must be"):
            DepthAligner(device="cpu").run([torch.zeros((3, 3, 1, 4, 4))], [1], merge=bad)
        with pytest.raises(ValueError, match="merge must be"):
            RollingDepthPipeline.forward(None, torch.zeros((1, 5, 3, 8, 8)), [1], True, [3], [1], [1], None, 0, 3, 6,
                                         None, False, 4, False, merge=bad)
        with pytest.raises(ValueError, match="merge must be"):
            RollingDepthPipeline.__call__(None, torch.zeros((5, 3, 8, 8)), merge=bad)
        with pytest.raises(ValueError, match="merge must be"):
            sharded_forward(None, torch.zeros((5, 3, 8, 8)), [1], merge=bad)
    assert check_merge("mean") == "mean" and check_merge("median") == "median"


def _brute(N, dil, w, ss, world):
    """Per rank the (frame, dilation, slot) of every row it holds, in its storage order (frames ascending, then
    dilation ascending, slot descending), by enumerating its snippets; and per frame the full set of (d, j)."""
    from rollingdepth_amd.shard import rank_subsets
    from tests.uncertainty_util import starts

    st = [starts(N, wd, d, s) for d, wd, s in zip(dil, w, ss)]
    counts = [len(x) for x in st]
    held = []
    for r in range(world):
        sub = rank_subsets(counts, world, r)
        rows = [(st[d][k] + j * dil[d], d, j) for d in range(len(dil)) for k in sub[d] for j in range(w[d])]
        held.append(sorted(rows, key=lambda t: (t[0], t[1], -t[2])))
    full = {f: {(d, j) for r in held for (g, d, j) in r if g == f} for f in range(N)}
    return counts, held, full


@pytest.mark.parametrize("world", [1, 2, 3, 8, 24])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_terms_exchange_plan_against_enumeration(layout, world):
    """Every rank's plan against brute force: its local row counts are those of its snippets, the send and
    receive counts match pairwise, and after the exchange (done here on (frame, d, j) labels) every frame's
    owner finds exactly the frame's full term set at row_idx[frame_off[i] : frame_off[i + 1]]."""
    from rollingdepth_amd.shard import chunk_bounds, merge_exchange_plan, terms_exchange_plan

    N, dil, w, ss = LAYOUTS[layout]
    counts, held, full = _brute(N, dil, w, ss, world)
    plans = [terms_exchange_plan(counts, dil, w, N, world, r, ss) for r in range(world)]
    sent = []
    for r, p in enumerate(plans):
        assert p.ranges == merge_exchange_plan(counts, dil, w, N, world, r, ss)[0]
        frames = [f for a, b in p.ranges for f in range(a, b)]
        assert p.row_counts == [sum(1 for t in held[r] if t[0] == f) for f in frames]
        assert p.row_off[0] == 0 and [b - a for a, b in zip(p.row_off, p.row_off[1:])] == p.row_counts
        assert sum(p.send) == len(held[r]) == p.row_off[-1]  # every row goes to exactly one owner
        o, per_dst = 0, []
        for m in p.send:
            per_dst.append(held[r][o:o + m])
            o += m
        sent.append(per_dst)
    assert all(plans[s].send[q] == plans[q].recv[s] for s in range(world) for q in range(world))
    seen = 0
    for q, p in enumerate(plans):
        f0, f1 = chunk_bounds(N, world)[q]
        rbuf = [t for s in range(world) for t in sent[s][q]]
        assert len(rbuf) == sum(p.recv) == len(p.row_idx) and len(p.frame_off) == f1 - f0 + 1
        assert sorted(p.row_idx) == list(range(len(rbuf)))  # every received row is used exactly once
        for i, f in enumerate(range(f0, f1)):
            got = [rbuf[k] for k in p.row_idx[p.frame_off[i]:p.frame_off[i + 1]]]
            assert all(t[0] == f for t in got)
            assert len(got) == len(full[f]) and {(d, j) for _, d, j in got} == full[f]
            seen += 1
        assert p.max_count == max([len(full[f]) for f in range(f0, f1)], default=0)
    assert seen == N
    if world == 24:  # a rank with an empty frame chunk, and ranks without a snippet
        assert chunk_bounds(N, world)[-1][0] == chunk_bounds(N, world)[-1][1] and not held[-1]
    with pytest.raises(ValueError, match="gives"):
        terms_exchange_plan([c + 1 for c in counts], dil, w, N, world, 0, ss)


def test_layout_cover_counts():
    """The cover counts the GPU tests rely on: `wide` 8 … 19 with both parities on both sides of 16, `full`
    8, 16, …, 64 with frames 7 … 15 at 64 — by enumeration and from the one-rank plan."""
    from rollingdepth_amd.shard import terms_exchange_plan

    cover = {}
    for name in ("wide", "full"):
        N, dil, w, ss = LAYOUTS[name]
        counts, _, full = _brute(N, dil, w, ss, 1)
        cover[name] = (counts, [len(full[f]) for f in range(N)])
        off = terms_exchange_plan(counts, dil, w, N, 1, 0, ss).frame_off  # one rank owns every frame
        assert [b - a for a, b in zip(off, off[1:])] == cover[name][1]
    assert cover["wide"][0] == [21, 19, 17, 15, 13, 11, 9, 7]
    cw = set(cover["wide"][1])
    assert min(cw) == 8 and max(cw) == 19 and {c % 2 for c in cw if c < 16} == {0, 1} == {c % 2 for c in cw if c > 16}
    assert cover["full"][0] == [16] * 8
    assert cover["full"][1] == [8 * min(f + 1, 8, 23 - f) for f in range(23)]
    assert all(cover["full"][1][f] == 64 for f in range(7, 16))


def test_reference_on_a_hand_worked_example():
    """c = 1, 2, 3, 4 (the last with a tie), two pixels each."""
    from tests import median_util as M

    f = np.float32
    med, mad = M.median_mad(np.array([[2.5, -1.0]], f))
    assert med.tolist() == [2.5, -1.0] and mad.tolist() == [0.0, 0.0]
    med, mad = M.median_mad(np.array([[4.0, 1.0], [1.0, 2.0]], f))
    assert med.tolist() == [2.5, 1.5] and mad.tolist() == [1.5, 0.5]
    # 3, 1, 2 → 2; deviations 1, 1, 0 → 1.   −1, 5, 0 → 0; deviations 1, 5, 0 → 1
    med, mad = M.median_mad(np.array([[3.0, -1.0], [1.0, 5.0], [2.0, 0.0]], f))
    assert med.tolist() == [2.0, 0.0] and mad.tolist() == [1.0, 1.0]
    # 7, 2, 2, 1 → sorted 1 2 2 7, median 2 (a tie in the middle); deviations 5 0 0 1 → sorted 0 0 1 5 → 0.5
    # 0, 10, 4, 1 → sorted 0 1 4 10, median 2.5; deviations 2.5 7.5 1.5 1.5 → sorted 1.5 1.5 2.5 7.5 → 2
    med, mad = M.median_mad(np.array([[7.0, 0.0], [2.0, 10.0], [2.0, 4.0], [1.0, 1.0]], f))
    assert med.tolist() == [2.0, 2.5] and mad.tolist() == [0.5, 2.0]
    assert med.dtype == f and mad.dtype == f
    # the even rule rounds once, from f64: 1 and 1 + 2⁻²³ average to the tie 1 + 2⁻²⁴ → even → 1
    a = np.array([[1.0], [np.nextafter(f(1), f(2))]], f)
    assert M.median_rule(a)[0] == f(1.0)
    # no terms: 0 and 0
    med, mad = M.median_mad(np.zeros((0, 2), f))
    assert med.tolist() == [0.0, 0.0] and mad.tolist() == [0.0, 0.0]
    ref = M.median_reference([np.zeros((0, 1), f), np.array([[1.0], [3.0]], f)])
    assert ref[0].tolist() == [[0.0], [2.0]] and ref[1].tolist() == [[0.0], [1.0]] and ref[2].tolist() == [0, 2]
