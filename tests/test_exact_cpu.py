"""CPU: what tests/test_gpu_conv_exact.py stands on (tests/_exact.py), for every case it runs.

  1. Order independence: an fp32 convolution with the input channels permuted, and one summed tap by tap
     in reverse, equal the fp64 reference bitwise; so does an fp32 weight gradient over reversed images.
  2. The recipes' conditions, on the references alone: max |acc| <= 256 (lossless), sum |x| |w| < 2^24
     and the ties (rounding), the zero shares of the masks, sum |.| < 2^24 for db and dw.
  3. Emulated wrong answers, each applied to a reference: found by torch.equal, placed by
     mismatch_report, and the verdict of the older criterion (norm_rel < 4e-3 and 99.9 % of the elements
     within a bf16 step; 1e-6 norm-relative for db) on the same wrong answer pinned, whichever way it
     falls: this is what the tolerance tests of test_gpu_encoder.py / test_gpu_arena_encoder.py let
     through.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact as E  # noqa: E402

FWD_CASES = [(r, *s, *nh) for r in E.RECIPES for s in E.FWD_GEN for nh in E.FWD_NH] + \
            [(r, *s, *nh) for r in E.RECIPES for s in E.FWD_T for nh in E.FWD_T_NH]
WRW_CASES = [(s, nhw) for s in [E.FWD_K5] + E.WRW_GEN for nhw in E.WRW_NHW]


# ---------------------------------------------------------------------- 1 + 2: the forward cases
@pytest.mark.parametrize("recipe,k,ci,co,N,H", FWD_CASES)
def test_forward_case_is_order_independent_and_meets_its_conditions(recipe, k, ci, co, N, H):
    c = E.forward_case(recipe, k, ci, co, N, H)
    x, w, ref = E.nchw(c.x).float(), E.nchw(c.w).float(), E.nchw(c.acc)
    for t in (c.x, c.w):  # integer-valued bf16
        assert t.dtype == E.BF16 and torch.equal(t.float(), t.float().round())
    # the conditions
    bound = float(F.conv2d(x.double().abs(), w.double().abs(), padding=k // 2).max())
    assert bound < E.EXACT
    if recipe == "lossless":
        assert float(ref.abs().max()) <= E.LOSSLESS_MAX
        assert torch.equal(E.to_bf16(ref).double(), ref)
    else:
        mx, mw = E.rounding_range(ci * k * min(k, H))
        assert ci * k * k * mx * mw < E.EXACT
        ties = E.count_ties(ref)
        print(f"{recipe} k {k} ci {ci} co {co} N {N} H {H}: range ({mx}, {mw}), max |acc| {float(ref.abs().max()):.0f}, {ties} ties")
        assert ties >= E.min_ties(ref.numel()), ties
    # fp32, the input channels permuted
    perm = torch.randperm(ci, generator=E.gen("perm", ci))
    assert torch.equal(F.conv2d(x[:, perm], w[:, perm], padding=k // 2).double(), ref)
    # fp32, tap by tap in reverse
    xp = F.pad(x, (k // 2,) * 4)
    acc = torch.zeros(ref.shape, dtype=torch.float32)
    for kh in reversed(range(k)):
        for kw in reversed(range(k)):
            acc += torch.einsum("nchw,oc->nohw", xp[:, :, kh:kh + H, kw:kw + E.W_FWD], w[:, :, kh, kw])
    assert torch.equal(acc.double(), ref)
    # the bias is not integer-valued: the double rounding is exercised
    assert bool((c.bias.float() != c.bias.float().round()).any())


@pytest.mark.parametrize("recipe,N,H", [("lossless", *E.EPI_NH), ("rounding", *E.EPI_NH), ("lossless", *E.EPI_BIG_NH)])
def test_epilogue_case_meets_its_conditions(recipe, N, H):
    c = E.epilogue_case(recipe, N, H)
    assert N * (H // 2) > 256 or (N, H) == E.EPI_NH
    if recipe == "lossless":
        assert float(c.acc.abs().max()) <= E.LOSSLESS_MAX
    for name in ("g2", "t", "m", "pa", "cb"):
        t = c[name].float()
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
    assert float((c.m == 0).float().mean()) >= E.MIN_ZERO_SHARE
    assert float(((c.pa + c.cb) == 0).float().mean()) >= E.MIN_ZERO_SHARE
    a, out = E.res_ref(c)
    assert float(((a + c.cb) == 0).float().mean()) > 0 and bool((out == 0).any()) and bool((out > 0).any())
    for mode, with_g2 in ((1, False), (1, True), (2, True)):
        r = E.dgrad_ref(c, mode, with_g2)
        assert float(r["db_abs"].max()) < E.EXACT, (mode, with_g2)
        assert torch.equal(r["db"].float().double(), r["db"])
        assert bool((r["out"] != 0).any())


def test_no_older_case_reaches_the_second_reduce_iteration():
    """conv_chan_reduce_kernel adds rows t, t + 256, ...: the kernel tests run N * H / 2 = 6 workgroups,
    the encoder tests N = 4, H = 128: 256. The (129, 4) case has 258."""
    assert 2 * (6 // 2) <= 256 and 4 * (128 // 2) <= 256
    N, H = E.EPI_BIG_NH
    assert N * (H // 2) == 258


# ---------------------------------------------------------------------- 1 + 2: the weight gradients
@pytest.mark.parametrize("shape,nhw", WRW_CASES)
def test_weight_gradient_case_is_order_independent_and_exact(shape, nhw):
    (k, ci, co), (N, H, W) = shape, nhw
    c = E.wrw_case("rounding", k, ci, co, N, H, W)
    assert c.abs_max < E.EXACT
    assert float(c.dw.abs().max()) > 1000  # sums reach the thousands
    assert torch.equal(c.dw.float().double(), c.dw)
    x, dy = E.nchw(c.x).float().flip(0), E.nchw(c.dy).float().flip(0)  # fp32 over the images in reverse
    dw32 = torch.nn.grad.conv2d_weight(x, (co, ci, k, k), dy, padding=k // 2)
    assert torch.equal(E.nhwc(dw32).double(), c.dw)


# ---------------------------------------------------------------------- 3: emulated wrong answers
def found(wrong, ref, dims=("n", "h", "w", "c")):
    """torch.equal finds it; the report (returned) places it."""
    assert not torch.equal(wrong, ref)
    rep = E.mismatch_report(wrong, ref, dims)
    assert rep and "elements differ" in rep
    assert E.mismatch_report(ref, ref.clone(), dims) == ""
    return rep


MAIN = ("rounding", *E.FWD_K5, *E.EPI_NH)


def test_truncating_conversion():
    c = E.forward_case(*MAIN)
    ref, wrong = E.forward_ref(c.acc), E.forward_ref(c.acc, cast=E.trunc_bf16)
    rep = found(wrong, ref)
    assert "largest difference 1 bf16 steps" in rep
    nr, share, verdict = E.old_criterion(wrong, ref)
    print(rep, f"\nold criterion: norm_rel {nr:.3e}, share {share:.5f}")
    assert verdict == OLD["trunc"]


def test_truncating_conversion_on_the_older_tests_data():
    """test_conv_forward_kernel_against_fp32's own data (seed 17, randn): the truncation misses the norm
    bound by 2 % (4.07e-3 against 4e-3) and passes the element criterion outright."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 128, 6, 128, generator=g).to(E.BF16)
    w = (torch.randn(128, 128, 5, 5, generator=g) / 40).to(E.BF16)
    acc = F.conv2d(x.double(), w.double(), padding=2)
    ref = acc.to(E.BF16)
    nr, share, verdict = E.old_criterion(E.trunc_bf16(acc), ref)
    print(f"old criterion on truncation: norm_rel {nr:.3e}, share {share:.5f}")
    assert 4e-3 < nr < 4.2e-3 and share == 1.0 and not verdict
    corner = ref.clone()
    corner[0, :, 0, 0] = 0  # one corner pixel, all 128 channels
    nr, share, verdict = E.old_criterion(corner, ref)
    print(f"old criterion on a zeroed corner pixel: norm_rel {nr:.3e}, share {share:.5f}")
    assert share > 0.999 and verdict == OLD["corner"]
    assert "per h (1 of 6 have any): 0:" in found(corner.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1))


def test_single_rounding_of_acc_plus_bias():
    c = E.forward_case(*MAIN)
    ref = E.forward_ref(c.acc, c.bias)
    wrong = E.forward_ref(c.acc, c.bias, single_rounding=True)
    rep = found(wrong, ref)
    nr, share, verdict = E.old_criterion(wrong, ref)
    print(rep, f"\nold criterion: norm_rel {nr:.3e}, share {share:.5f}")
    assert verdict == OLD["single"]


def test_round_half_away():
    c = E.forward_case(*MAIN)
    ref, wrong = E.forward_ref(c.acc), E.forward_ref(c.acc, cast=E.half_away_bf16)
    rep = found(wrong, ref)
    differ = int((wrong != ref).sum())
    assert 0 < differ <= E.count_ties(c.acc)  # ties only: those whose even neighbour lies towards zero
    assert torch.equal(wrong[wrong != ref].abs() > ref[wrong != ref].abs(), torch.ones(differ, dtype=torch.bool))
    nr, share, verdict = E.old_criterion(wrong, ref)
    print(rep, f"\nold criterion: norm_rel {nr:.3e}, share {share:.5f}")
    assert verdict == OLD["half_away"]


def test_mask_greater_or_equal():
    c = E.epilogue_case("lossless", *E.EPI_NH)
    for mode in (1, 2):
        ref, wrong = E.dgrad_ref(c, mode, True), E.dgrad_ref(c, mode, True, ge=True)
        rep = found(wrong["out"], ref["out"])
        assert not torch.equal(wrong["db"], ref["db"])
        differ = wrong["out"] != ref["out"]
        assert bool((c.m[differ] == 0).all())
        nr, share, verdict = E.old_criterion(wrong["out"], ref["out"])
        print(rep, f"\nold criterion (had it been applied): norm_rel {nr:.3e}, share {share:.5f}")
        assert verdict == OLD["ge"]
    # the older tests' masks are randn planes: no element is 0, so `>=` and `>` agree on them
    m = torch.randn(2, 6, 128, 128, generator=torch.Generator().manual_seed(5)).to(E.BF16)
    assert not bool((m == 0).any())


def test_one_tap_dropped_at_one_pixel():
    k, ci, co, N, H = 7, 128, 64, 3, 10
    c = E.forward_case("lossless", k, ci, co, N, H)
    n, h, w_, kh, kw = 1, 4, 70, 5, 1  # an interior pixel, an off-centre tap
    term = c.w[:, kh, kw, :].double() @ c.x[n, h + kh - k // 2, w_ + kw - k // 2, :].double()  # [co]
    acc = c.acc.clone()
    acc[n, h, w_] -= term
    ref, wrong = E.forward_ref(c.acc), E.forward_ref(acc)
    rep = found(wrong, ref)
    assert int(term.ne(0).sum()) > co // 2
    assert f"per n (1 of {N} have any): {n}:" in rep and f"per h (1 of {H} have any): {h}:" in rep
    assert f"per w (1 of 128 have any): {w_}:" in rep
    nr, share, verdict = E.old_criterion(wrong, ref)
    print(rep, f"\nold criterion: norm_rel {nr:.3e}, share {share:.5f}")
    assert verdict == OLD["tap"]


def test_first_256_partial_rows_only_in_db():
    c = E.epilogue_case("lossless", *E.EPI_BIG_NH)
    for mode in (1, 2):
        ref, wrong = E.dgrad_ref(c, mode, True), E.dgrad_ref(c, mode, True, blocks=256)
        rep = found(wrong["db"].float(), ref["db"].float(), dims=("c",))
        assert torch.equal(wrong["out"], ref["out"])
        nr = E.norm_rel(wrong["db"], ref["db"])
        print(rep, f"\nthe older db criterion (1e-6), had a case reached 258 workgroups: norm_rel {nr:.3e}")
        assert (nr < 1e-6) == OLD["db256"]


# The older criterion's verdicts on the emulations above (True: it lets the wrong answer pass), with the
# figures it gave here. On the exact data every conversion error is invisible to it (about half its norm
# bound, no element further than a step), and so is a dropped tap; what it does catch, it catches by the
# norm alone (the corner pixel: 1.7e-2, share 0.99935 > 0.999) or would have, had a case supplied the
# zeros (`>=`: the older masks are randn) or the 258 workgroups (db: the older cases stop at 256).
OLD = {"trunc": True,       # norm_rel 2.01e-3, share 1.0 (10,587 elements a step off)
       "corner": False,     # norm_rel 1.71e-2, share 0.99935
       "single": True,      # norm_rel 1.99e-3, share 0.99999
       "half_away": True,   # norm_rel 2.01e-3, share 1.0
       "ge": False,         # norm_rel 7.1e-1, share 0.805
       "tap": True,         # norm_rel 2.45e-3, share 0.9998 (49 of 64 channels of one pixel)
       "db256": False}      # norm_rel 7.7e-2
