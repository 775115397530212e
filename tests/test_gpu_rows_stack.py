"""GPU: row r of the bf16 SIREN stack's result against row r of the fp64 reference.

The parity tests of the stack judge a whole tensor by one norm (||a - b|| / ||b|| <= 3e-2 / 5e-2 in bf16
mode); an error confined to a few rows (a tail tile, the last valid row, a ring stage handed over one tile
late, a set boundary of the batched-weights form) passes that (tests/test_rows_cpu.py pins it). Rows are
independent in a SIREN, so here every row answers for itself (tests/_rows.py):

  R1  per_row_err(y), per_row_err(y without `saved`) <= K_ROW x the bf16 emulation's worst row, every row
  R2  the same for dx under the full random dy
  R3  dy zero except row r of set b: every dW_l, db_l within 5e-2 norm-rel of that row's contribution
      dZ_l[r]^T a_l[r] of the exact pass, and dx[b, r] within 5e-2 of the reference row
  R4  under the same probe every other row of dx, and with batched weights every other set's dW_l and
      db_l, is 0.0 exactly: a zero dZ row times finite factors is zero, and no atomics or cross-row terms
      are on the path
  R5  the fp64 sum over the 32-row tiles of the backward of dy masked to the tile equals the backward of
      the full dy to 1e-5 norm-rel (tests/test_gpu_hyper.py's bound for "differs in summation order only")
  R6  diff_operators.gradient through SingleBVPNet(precision="bf16") (the tangent-stream kernels), per row,
      against the exact dx for dy = 1: <= K_ROW x the emulation's worst row

The entry points are driven through problem / run_stack of tests/test_gpu_arena_stack.py on Plain buffers,
so the flag variants only the C ABI can be handed come along (no dx, x 8 bytes past a 16-byte boundary, dy
4 bytes past). K_ROW: profiles/rowwise_probes.txt has every case's measured ratio (the kernel's worst row
over the emulation's worst row; the largest is 1.44) and the rule K_ROW = max(3, 1.5 x the largest), one
digit. At 3, K_ROW x EMU_ROW_CAP is what a wrong row exceeds (ROW_FLOOR of tests/_rows.py); a ratio that asks
for more than 6 is a finding about that row, not a reason to raise K_ROW. The same file has the mutants (tail
row dropped from dW, dx rows swapped in the tail tile, a forward row repeated) and which tests caught them.
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from _arena import Plain  # noqa: E402
from _rows import (EMU_ROW_CAP, ROW_CASES, per_row_err, probe_rows, probe_sets, row_contribution,  # noqa: E402
                   stack_rows, to_bf16)
from make_golden_stack_plan import VARIANTS  # noqa: E402
from make_golden_stack_sizes import setting  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from test_gpu_arena_stack import problem, run_stack  # noqa: E402
from test_gpu_siren_stack import TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W0 = 30.0
K_ROW = 3.0
assert K_ROW <= 6
PROBE_TOL = TOL["bf16"][1]
SUM_ORDER_TOL = 1e-5

# every setting is another backward plan
ALL_SETTINGS = ("default", "pair_ring=0", "dx_ring=0", "dw_ring=0", "fused_backward=0", "ring_output_fusion=0",
                "pair_tail_reduce=0", "debug_keep_p0=1")
TWO_SETTINGS = ALL_SETTINGS[:2]
GRID = [(c, s) for c in "acd" for s in ALL_SETTINGS] + [(c, s) for c in "efgh" for s in TWO_SETTINGS] + \
       [("sine", "default")] + [(c, s) for c in ("tiny1", "tiny2", "tiny31", "tiny33") for s in ALL_SETTINGS]


def flag_variants(case):
    """Bit 0: dx wanted, bit 1: x 16-byte aligned, bit 2: dy 16-byte aligned. The grid cases get the
    arena grid's variants and always 7; the others what the arena tests give them."""
    if case in VARIANTS:
        return sorted(set(VARIANTS[case]) | {7}, reverse=True)
    return (7, 6) if case == "sine" else (7, 6, 1)


@functools.lru_cache(maxsize=None)
def references(case):
    """The case's problem, its exact pass and its bf16/bf16 emulation's worst rows."""
    args = ROW_CASES[case]
    p = problem(*args[:5], seed=args[5])
    ref = stack_rows(p["x"], p["params"], p["dy"], W0, p["outermost_linear"])
    emu = stack_rows(p["x"], p["params"], p["dy"], W0, p["outermost_linear"], to_bf16, to_bf16)
    worst = {k: float(per_row_err(emu[k], ref[k]).max()) for k in ("y", "dx")}
    assert 0 < worst["y"] <= EMU_ROW_CAP and 0 < worst["dx"] <= EMU_ROW_CAP, worst
    return p, ref, worst


def masked(p, rows, b=None):
    """The problem with dy zero except `rows` of set b (None: of every set)."""
    dy = torch.zeros_like(p["dy"])
    if b is None:
        dy[:, rows] = p["dy"][:, rows]
    else:
        dy[b, rows] = p["dy"][b, rows]
    return dict(p, dy=dy)


def check_rows(tag, name, got, ref, emu_worst):
    """R1 / R2 / R6: every row within K_ROW x the emulation's worst row; prints the measured ratio."""
    e = per_row_err(got.cpu(), ref)
    worst, at = float(e.max()), int(e.argmax())
    b, r = divmod(at, e.shape[1])
    print(f"ROWS {tag} {name}: worst row {worst:.3e} (set {b} row {r}), emulation {emu_worst:.3e}, ratio {worst / emu_worst:.2f}")
    assert torch.isfinite(e).all() and worst <= K_ROW * emu_worst, \
        f"{tag} {name}: set {b} row {r} is {worst:.3e} of the RMS row norm off, > {K_ROW} x {emu_worst:.3e}"


def check_probe(tag, p, ref, out, b, r):
    """R3 and R4 of one probe (row r of set b)."""
    for l in range(len(p["dims"]) - 1):
        for k, want in zip((f"dW{l}", f"db{l}"), row_contribution(ref, l, [r], b)):
            got = out[k]
            if p["sets"]:
                assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[b])), \
                    f"R4 {tag}: probe of set {b} row {r} reached another set's {k}"
                got, want = got[b], want[b]
            e = orc.norm_rel(got.cpu(), want)
            assert e <= PROBE_TOL, f"R3 {tag}: {k} of the probe of set {b} row {r}: norm-rel {e:.3e} > {PROBE_TOL}"
    if "dx" in out:
        dx = out["dx"]
        assert int(torch.count_nonzero(dx)) == int(torch.count_nonzero(dx[b, r])), \
            f"R4 {tag}: probe of set {b} row {r} reached other rows of dx: " \
            f"{torch.nonzero(dx.abs().sum(-1))[:4].tolist()}"
        e = orc.norm_rel(dx[b, r].cpu(), ref["dx"][b, r])
        assert e <= PROBE_TOL, f"R3 {tag}: dx of the probed set {b} row {r}: norm-rel {e:.3e} > {PROBE_TOL}"


@pytest.mark.parametrize("case,s", GRID)
def test_rows(case, s):
    """R1 - R4 of one case under one setting, every flag variant."""
    p, ref, emu_worst = references(case)
    with setting(s):
        for flags in flag_variants(case):
            tag = f"{case}|{s}|{flags}"
            out = run_stack(Plain(DEV), p, flags)
            check_rows(tag, "y", out["y"], ref["y"], emu_worst["y"])
            check_rows(tag, "y_nosaved", out["y_nosaved"], ref["y"], emu_worst["y"])
            if flags & 1:
                check_rows(tag, "dx", out["dx"], ref["dx"], emu_worst["dx"])
            for b in probe_sets(p["sets"]):
                for r in probe_rows(p["rows"]):
                    check_probe(tag, p, ref, run_stack(Plain(DEV), masked(p, [r], b), flags), b, r)


@pytest.mark.parametrize("case,s", [("c", s) for s in ALL_SETTINGS] + [("e", s) for s in TWO_SETTINGS])
def test_tiles_add_up(case, s):
    """R5: one backward per 32-row tile (dy masked to the tile, in every set), summed in fp64."""
    p, _, _ = references(case)
    keys = [f"d{t}{l}" for l in range(len(p["dims"]) - 1) for t in "Wb"]
    with setting(s):
        full = run_stack(Plain(DEV), p, 7)
        total = {k: torch.zeros_like(full[k], dtype=torch.float64) for k in keys}
        for t0 in range(0, p["rows"], 32):
            part = run_stack(Plain(DEV), masked(p, list(range(t0, min(t0 + 32, p["rows"])))), 7)
            for k in keys:
                total[k] += part[k].double()
    for k in keys:
        e = orc.norm_rel(total[k].cpu(), full[k].double().cpu())
        print(f"ROWS {case}|{s} tiles {k}: norm-rel {e:.3e}")
        assert e <= SUM_ORDER_TOL, f"R5 {case}|{s}: the per-tile {k} add up to the full one only to {e:.3e}"


@pytest.mark.parametrize("side,hidden", [(33, 256), (20, 64)])
def test_gradient_rows(side, hidden):
    """R6: the analytic gradient (tangent-stream kernels) per row, on random coordinates."""
    from siren_mri_amd import diff_operators, modules
    torch.manual_seed(side)
    m = modules.SingleBVPNet(out_features=1, in_features=2, type="sine", hidden_features=hidden,
                             num_hidden_layers=3, precision="bf16").to(DEV)
    coords = torch.rand(1, side * side, 2, generator=torch.Generator().manual_seed(hidden)) * 2 - 1
    o = m({"coords": coords.to(DEV)})
    g = diff_operators.gradient(o["model_out"], o["model_in"])
    sd = m.state_dict()
    params = [(sd[f"net.net.{i}.0.weight"].cpu(), sd[f"net.net.{i}.0.bias"].cpu()) for i in range(5)]
    ones = torch.ones(1, side * side, 1)
    ref = stack_rows(coords, params, ones, W0, True)
    emu = stack_rows(coords, params, ones, W0, True, to_bf16, to_bf16)
    emu_worst = float(per_row_err(emu["dx"], ref["dx"]).max())
    assert 0 < emu_worst <= EMU_ROW_CAP, emu_worst
    assert g.shape == coords.shape
    check_rows(f"gradient|{side}x{side}|{hidden}", "gradient", g.detach(), ref["dx"], emu_worst)
    check_rows(f"gradient|{side}x{side}|{hidden}", "y", o["model_out"].detach(), ref["y"],
               float(per_row_err(emu["y"], ref["y"]).max()))
