"""The dyadic attention cases of tests/attention_util.py on the CPU: the inputs keep a faithful flash
loop inside the derived bound, every modelled defect leaves it by a wide margin, and the suite's older
absolute tolerance does not (tests/test_attention_exact_gpu.py holds the kernels to the same bound)."""
import os
import re

import pytest
import torch

from tests import attention_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KBS = {64: (U.KB_D64, U.TK_PIPE), 512: (U.KT_D512,)}  # the kernel tiles each case is run with
CASE_KB = [(n, kb) for n, c in U.CASES.items() for kb in KBS[c["D"]]]

_cache = {}


def _case(name):
    """The case with its f64 reference, computed once and shared (read-only)."""
    if name not in _cache:
        c = U.dyadic_case(name)
        c["ref"], c["A"] = U.reference(c)
        _cache[name] = c
    return _cache[name]


def _excess(name, KB, defect=None):
    c = _case(name)
    y = U.flash_restatement(c, KB, defect)
    return U.excess(y, c["ref"], U.bound(c["ref"], c["A"], U.tiles(c["Sk"], KB))), y


def test_scale_and_exp2_are_exact():
    """scale = ln 2: the kernels' f32 scale·log2(e) is exactly 1; torch's exp2 is exact on integers."""
    sl2 = torch.tensor(U.SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    assert sl2.item() == 1.0
    e = torch.arange(-60, 61, dtype=torch.float32)
    assert torch.equal(torch.exp2(e), torch.ldexp(torch.ones(121), e.int()))


def test_tile_constants_match_the_sources():
    src = {f: open(os.path.join(ROOT, "rollingdepth_amd", "csrc", f), encoding="utf-8").read()
           for f in ("attention.hip", "attention_d512.hip")}

    def const(f, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src[f]).group(1))

    assert const("attention.hip", "KB") == U.KB_D64 and const("attention.hip", "NSLOT") == U.NSLOT_D64
    assert const("attention.hip", "TK") == U.TK_PIPE and const("attention.hip", "NSL") == U.NSL_PIPE
    assert const("attention_d512.hip", "KT5") == U.KT_D512


def test_inputs_are_dyadic():
    for name in U.CASES:
        c = _case(name)
        assert all(torch.equal(c[n], c[n].round()) for n in "qkv") and c["v"].abs().max() <= 8
        k = c["k"].view(c["B"], c["Sk"], c["H"], c["D"]).float()
        for t in range(0, c["Sk"], c["ot"]):  # one offset tile spans at most 5 units per dimension
            kt = k[:, t:t + c["ot"]]
            assert (kt.amax(1) - kt.amin(1)).max() <= 4
        if not c["uniform"]:  # every dimension is some query's dimension (once Sq ≥ D)
            hot = c["q"].view(c["B"], c["Sq"], c["H"], c["D"]).sum(1)
            assert (hot > 0).sum(-1).min() == min(c["Sq"], c["D"])


@pytest.mark.parametrize("name,KB", CASE_KB)
def test_restatement_inside_bound(name, KB):
    e, _ = _excess(name, KB)
    print(f"{name} KB={KB}: excess {e:.3f}")
    assert e <= 1.0


# defect → named cases (and tiles) on which it must leave the bound by 4× or more
REJECTED_ON = {
    "drop_last_key": [("sk129_last_jump", 128), ("sk769_wrap", 64), ("sk3073_uniform", 128), ("d512_sq15_sk31", 32)],
    "duplicate_last_key": [("sk5", 128), ("sk641_jump30", 128), ("sk3073_uniform", 64), ("d512_sq33_sk65_drop20", 32)],
    "unmasked_padding": [("sk127", 128), ("sk641_jump30", 64), ("sk3073_uniform", 128), ("d512_sq127_sk95_rise", 32)],
    "skip_l_rescale": [("sk257_partial", 128), ("sk385_jump12", 64), ("sk769_wrap", 128),
                       ("d512_sq513_sk129_odd_blocks", 32)],
    "skip_o_rescale": [("sk257_partial", 64), ("sk641_jump30", 128), ("sk769_wrap", 64),
                       ("d512_sq129_sk97_jump30", 32)],
    "stale_tile_after_ring_wrap": [("sk641_jump30", 128), ("sk769_wrap", 128), ("sk385_drop20", 64),
                                   ("sk3073_uniform", 128), ("d512_sq33_sk65_drop20", 32)],
    "swap_two_heads": [("sk1", 128), ("sk257_rise", 64), ("sk3073_uniform", 128)],
}


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_defect_leaves_the_bound(defect):
    assert set(REJECTED_ON) == set(U.DEFECTS)
    for name, KB in REJECTED_ON[defect]:
        e, _ = _excess(name, KB, defect)
        print(f"{defect} on {name} KB={KB}: excess {e:.3g}")
        assert e >= 4.0, (name, KB, e)


@pytest.mark.parametrize("defect", ["drop_last_key", "duplicate_last_key", "unmasked_padding"])
def test_key_count_defects_on_every_ragged_case(defect):
    """A dropped, doubled or unmasked key is rejected on every case whose last tile is ragged.  (Sk = 1
    is left out for the doubled key alone: a softmax over one key does not change when it is doubled.)"""
    low = float("inf")
    for name, KB in CASE_KB:
        Sk = U.CASES[name]["Sk"]
        if Sk % KB == 0 or (defect == "duplicate_last_key" and Sk == 1):
            continue
        e, _ = _excess(name, KB, defect)
        low = min(low, e)
        assert e >= 4.0, (name, KB, e)
    print(f"{defect}: smallest excess over the ragged cases {low:.3g}")


@pytest.mark.parametrize("name", [n for n, c in U.CASES.items() if c["Sk"] >= 641])
def test_old_absolute_tolerance_accepts_a_dropped_key(name):
    """The gap this file closes: max |Δ| < 5e-3, the assertion of the first-generation attention tests,
    accepts an output with the last key missing once Sk reaches a few hundred; the bound rejects it."""
    for KB in KBS[U.CASES[name]["D"]]:
        e, y = _excess(name, KB, "drop_last_key")
        err = (y.double() - _case(name)["ref"]).abs().max().item()
        print(f"{name} KB={KB}: dropped key max |d| {err:.2e}, excess {e:.3g}")
        assert err < 5e-3 and e >= 4.0


@pytest.mark.parametrize("name,KB", [(n, kb) for n, kb in CASE_KB if U.CASES[n]["uniform"]])
def test_uniform_cases_are_bitwise_the_mean(name, KB):
    c = _case(name)
    y = U.flash_restatement(c, KB)
    mean = c["v"].double().mean(1, keepdim=True).expand(-1, c["Sq"], -1).half()
    assert torch.equal(y.view(torch.int16), mean.contiguous().view(torch.int16))
