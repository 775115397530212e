"""CPU: the row-local references of tests/_rows.py, and the conditions tests/test_gpu_rows_stack.py
stands on.

  1. stack_rows without rounding is the oracle (orc.siren_forward + autograd, fp64) to 1e-12; the
     one-hot contributions of all rows add up to the full dW and db.
  2. On every GPU case the bf16/bf16 emulation stays under EMU_ROW_CAP per row (y, dx) and under
     EMU_PROBE_CAP per one-hot probe, so that k x the emulation's worst row stays below ROW_FLOOR and
     the project's 5e-2 leaves a correct kernel a factor of 2.
  3. The blind spot, pinned: wrong results confined to a row or two (the last row's contribution
     missing from dW and dx, the last two rows of y swapped, a row computed with the next set's
     weights) pass the whole-tensor bounds TOL["bf16"] of tests/test_gpu_siren_stack.py on a case of
     the arena grid, and every one of them exceeds ROW_FLOOR or PROBE_FLOOR of the row-local measure.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _rows import (EMU_PROBE_CAP, EMU_ROW_CAP, PROBE_FLOOR, ROW_CASES, ROW_FLOOR, per_row_err, probe_rows,  # noqa: E402
                   probe_sets, row_contribution, stack_rows, to_bf16)
from oracle import siren_oracle as orc  # noqa: E402
from test_gpu_arena_stack import problem  # noqa: E402
from test_gpu_siren_stack import TOL  # noqa: E402

W0 = 30.0


def exact(p):
    return stack_rows(p["x"], p["params"], p["dy"], W0, p["outermost_linear"])


def emulation(p):
    return stack_rows(p["x"], p["params"], p["dy"], W0, p["outermost_linear"], to_bf16, to_bf16)


# ---------------------------------------------------------------------- 1. the exact pass
@pytest.mark.parametrize("dims,sets,rows,lin", [((2, 32, 32, 1), 0, 37, True), ((3, 16, 24, 2), 3, 21, True),
                                                ((3, 16, 16, 4), 0, 33, False), ((5, 8, 4), 2, 9, False)])
def test_exact_pass_is_the_oracle(dims, sets, rows, lin):
    p = problem("fp32", dims, sets, rows, lin)
    res = exact(p)
    assert orc.norm_rel(res["y"], p["ref"]["y"]) <= 1e-12
    assert orc.norm_rel(res["dx"], p["ref"]["dx"]) <= 1e-12
    for l in range(len(dims) - 1):
        assert orc.norm_rel(res["dW"][l], p["ref"][f"dW{l}"]) <= 1e-12
        assert orc.norm_rel(res["db"][l], p["ref"][f"db{l}"]) <= 1e-12
        assert res["a"][l].shape == (max(sets, 1), rows, dims[l]) and res["dZ"][l].shape == (max(sets, 1), rows, dims[l + 1])


@pytest.mark.parametrize("dims,sets,rows,lin", [((2, 32, 32, 1), 0, 37, True), ((3, 16, 24, 2), 3, 21, True),
                                                ((3, 16, 16, 4), 0, 33, False)])
def test_row_contributions_add_up(dims, sets, rows, lin):
    p = problem("fp32", dims, sets, rows, lin)
    res = exact(p)
    for l in range(len(dims) - 1):
        dW, db = row_contribution(res, l, range(rows))
        assert orc.norm_rel(dW, p["ref"][f"dW{l}"]) <= 1e-12 and orc.norm_rel(db, p["ref"][f"db{l}"]) <= 1e-12
        parts = [row_contribution(res, l, [r], b) for r in range(rows) for b in range(max(sets, 1))]
        assert orc.norm_rel(sum(w for w, _ in parts), p["ref"][f"dW{l}"]) <= 1e-12
        assert orc.norm_rel(sum(v for _, v in parts), p["ref"][f"db{l}"]) <= 1e-12


def test_a_probe_is_the_backward_of_a_masked_dy():
    """row_contribution(rows, b) equals a whole backward whose dy is masked to those rows of that set."""
    p = problem("fp32", (3, 16, 24, 2), 3, 21, True)
    res = exact(p)
    dy = torch.zeros_like(p["dy"])
    dy[1, [4, 20]] = p["dy"][1, [4, 20]]
    one = stack_rows(p["x"], p["params"], dy, W0, True)
    for l in range(3):
        dW, db = row_contribution(res, l, [4, 20], 1)
        assert orc.norm_rel(dW, one["dW"][l]) <= 1e-12 and orc.norm_rel(db, one["db"][l]) <= 1e-12
        assert float(dW[0].abs().max()) == 0.0 and float(dW[2].abs().max()) == 0.0


def test_per_row_err_uses_the_rms_row_norm():
    ref = torch.tensor([[[3.0, 4.0], [0.0, 1e-6], [5.0, 0.0]]])
    a = ref.clone()
    a[0, 1, 1] += 0.5
    e = per_row_err(a, ref)
    rms = ((25.0 + 1e-12 + 25.0) / 3) ** 0.5
    assert e.shape == (1, 3) and e[0, 0] == 0 and e[0, 2] == 0 and float(e[0, 1]) == pytest.approx(0.5 / rms)


def test_rounding_is_to_bf16_and_spares_layer_0():
    t = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -12], dtype=torch.float64)
    assert to_bf16(t).tolist() == [1.0, 1.0] and to_bf16(t + 2.0 ** -7).tolist() == [1.0 + 2.0 ** -7] * 2
    p = problem("fp32", (2, 32, 32, 1), 0, 37, True)
    res = emulation(p)
    assert 1e-4 < orc.norm_rel(res["y"], p["ref"]["y"]) < 3e-2   # rounded, and still the same function
    one = stack_rows(p["x"], p["params"][:1], torch.ones(1, 37, 32), W0, False, to_bf16, None)
    assert orc.norm_rel(one["y"], exact(dict(p, params=p["params"][:1], dy=torch.ones(1, 37, 32),
                                             outermost_linear=False))["y"]) == 0.0  # layer 0 stays exact


# ---------------------------------------------------------------------- 2. what the GPU tests stand on
def probe_errors(p, res, ref):
    """Worst error of `res` over the one-hot probes of the GPU tests: norm-rel of every dW_l and db_l
    contribution against the exact one, and of the probed dx row against the exact row."""
    worst = 0.0
    for b in probe_sets(p["sets"]):
        for r in probe_rows(p["rows"]):
            for l in range(len(p["dims"]) - 1):
                (dW, db), (rW, rb) = row_contribution(res, l, [r], b), row_contribution(ref, l, [r], b)
                worst = max(worst, orc.norm_rel(dW, rW), orc.norm_rel(db, rb))
            worst = max(worst, orc.norm_rel(res["dx"][b, r], ref["dx"][b, r]))
    return worst


@pytest.mark.parametrize("case", sorted(ROW_CASES))
def test_emulation_stays_under_the_caps(case):
    p = problem(*ROW_CASES[case][:5], seed=ROW_CASES[case][5])
    ref, emu = exact(p), emulation(p)
    ey, edx = float(per_row_err(emu["y"], ref["y"]).max()), float(per_row_err(emu["dx"], ref["dx"]).max())
    ep = probe_errors(p, emu, ref)
    print(f"case {case}: emulation worst row y {ey:.3e} dx {edx:.3e}, worst probe {ep:.3e}")
    assert ey <= EMU_ROW_CAP and edx <= EMU_ROW_CAP, (ey, edx)
    assert ep <= EMU_PROBE_CAP, ep


# ---------------------------------------------------------------------- 3. the blind spot
# Each wrong result is applied to the exact reference of a draw of an arena-grid shape (seed 0 is the
# arena grid's own data) on which it stays under the whole-tensor bounds; whether it does depends on the
# draw (two adjacent rows of y can lie close together), so the draws are named, not searched for.
def grid_problem(case, seed):
    return problem(*ROW_CASES[case][:5], seed=seed)


def whole_tensor_passes(p, wrong):
    """The wrong result under the whole-tensor measure of the existing suites."""
    ty, tg = TOL["bf16"]
    return all(orc.norm_rel(v, p["ref"][k]) <= (ty if k == "y" else tg) for k, v in wrong.items())


@pytest.mark.parametrize("case,seed", [("a", 0), ("d", 0), ("g", 0), ("c", 2), ("f", 2)])
def test_blind_spot_last_row_dropped(case, seed):
    """The last row (of the last set) contributes nothing to any dW_l or db_l, and its dx is zero."""
    p = grid_problem(case, seed)
    ref = exact(p)
    b, r, wrong = max(p["sets"], 1) - 1, p["rows"] - 1, {}
    for l in range(len(p["dims"]) - 1):
        dW, db = row_contribution(ref, l, [r], b)
        wrong[f"dW{l}"], wrong[f"db{l}"] = ref["dW"][l] - dW, ref["db"][l] - db
    wrong["dx"] = ref["dx"].clone()
    wrong["dx"][b, r] = 0.0
    assert whole_tensor_passes(p, wrong)
    # the one-hot probe of that row: the wrong kernel returns zeros for it
    for l in range(len(p["dims"]) - 1):
        rW, rb = row_contribution(ref, l, [r], b)
        assert orc.norm_rel(torch.zeros_like(rW), rW) > PROBE_FLOOR and orc.norm_rel(torch.zeros_like(rb), rb) > PROBE_FLOOR
    assert orc.norm_rel(wrong["dx"][b, r], ref["dx"][b, r]) > PROBE_FLOOR


@pytest.mark.parametrize("case,seed", [("a", 2), ("d", 2), ("f", 2)])
def test_blind_spot_last_two_rows_of_y_swapped(case, seed):
    p = grid_problem(case, seed)
    ref = exact(p)
    y = ref["y"].clone()
    y[:, [-2, -1]] = y[:, [-1, -2]]
    assert whole_tensor_passes(p, {"y": y})
    assert float(per_row_err(y, ref["y"]).max()) > ROW_FLOOR


@pytest.mark.parametrize("case,seed", [("e", 0), ("f", 0), ("g", 0)])
def test_blind_spot_row_computed_with_the_next_sets_weights(case, seed):
    """The last row of set 0 (y and dx) computed with set 1's weights."""
    p = grid_problem(case, seed)
    ref = exact(p)
    nxt = [(torch.roll(W, -1, 0), torch.roll(b, -1, 0)) for W, b in p["params"]]
    other = stack_rows(p["x"], nxt, p["dy"], W0, True)
    r = p["rows"] - 1
    wrong = {"y": ref["y"].clone(), "dx": ref["dx"].clone()}
    wrong["y"][0, r], wrong["dx"][0, r] = other["y"][0, r], other["dx"][0, r]
    assert whole_tensor_passes(p, wrong)
    worst = max(float(per_row_err(wrong["y"], ref["y"]).max()), float(per_row_err(wrong["dx"], ref["dx"]).max()))
    assert worst > ROW_FLOOR, worst
