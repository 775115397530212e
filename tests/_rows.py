"""Row-local references for the SIREN stack (CPU, float64).

Rows are independent in a SIREN: row r of y, of dx and of every dZ_l depends on row r of x and dy alone,
and each dW_l is a sum of per-row outer products dZ_l[r]^T a_l[r]. A whole-tensor norm hides an error
confined to a few rows (a tail tile, the last valid row, a set boundary); the three functions here make
row r of a kernel's result answer to row r of a reference.

  stack_rows        a hand-written forward and backward (no autograd) that keeps every layer's input
                    activation a_l and every per-row dZ_l. With both rounding functions None it is the exact
                    reference. With a rounding function it is the EMULATION: the arithmetic the 16-bit
                    kernels are allowed (operands rounded to a 16-bit format, exact products, exact sums)
                    and none of their tiling, phase codes or sine approximation. Its distance from the
                    exact pass is the yardstick the kernels' per-row error is measured in.
  row_contribution  dW_l and db_l of a dy that is nonzero only on some rows, from the exact pass: one pass
                    serves every one-hot probe.
  per_row_err       ||a[r] - ref[r]|| over the RMS row norm of ref, for every row of every set.

A plain helper module (not a conftest): the tests import it by name after putting tests/ on sys.path.
"""
import torch

F64 = torch.float64


def to_bf16(t):
    """Round to bfloat16 (nearest even) and widen again."""
    return t.to(torch.bfloat16).to(t.dtype)


def _same(t):
    return t


def _wt(W):
    return W.transpose(-1, -2)


def stack_rows(x, params, dy, w0, outermost_linear, round_fwd=None, round_bwd=None):
    """Forward and backward of a SIREN stack in float64, written out by hand.

    x [B, rows, C]; params [(W_l, b_l)] with W_l [out, in] (shared) or [B, out, in] (one set per batch
    entry), b_l to match; dy [B, rows, O]. Layer l: z_l = a_l W_l^T + b_l, a_{l+1} = sin(w0 z_l) (the
    last layer without the sine if outermost_linear), a_0 = x.

    round_fwd / round_bwd: None, or a function that rounds a float64 tensor to a 16-bit format and
    widens it again. round_fwd rounds a_l and W_l of every matmul but layer 0's (layer 0 runs in exact
    fp32 in the kernels too). round_bwd rounds, in the backward, dZ_l of every layer and a_l and W_l of
    every layer but 0 (x and W_0 stay as they are); cos(w0 z_l) is taken from the (rounded) forward.

    Returns a dict: y, dx, a (list, a[l] [B, rows, in_l]: what layer l's dW multiplies, rounded if
    round_bwd), dZ (list, dZ[l] [B, rows, out_l], rounded if round_bwd), dW and db (lists, summed over
    the rows, and over the batch when the weights are shared), batched (bool)."""
    rf, rb = round_fwd or _same, round_bwd or _same
    x, dy = x.to(F64), dy.to(F64)
    params = [(W.detach().to(F64), b.detach().to(F64)) for W, b in params]
    L = len(params)
    batched = params[0][0].dim() == 3
    acts, cosf = [x], []
    for l, (W, b) in enumerate(params):
        a = acts[-1]
        z = (a @ _wt(W) if l == 0 else rf(a) @ _wt(rf(W))) + b.unsqueeze(-2)
        if l < L - 1 or not outermost_linear:
            acts.append(torch.sin(w0 * z))
            cosf.append(w0 * torch.cos(w0 * z))
        else:
            acts.append(z)
            cosf.append(None)
    dA = dy
    a_out, dZ_out, dWs, dbs = [None] * L, [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        W = params[l][0]
        dZ = rb(dA if cosf[l] is None else dA * cosf[l])
        a = acts[l] if l == 0 else rb(acts[l])
        dW = _wt(dZ) @ a                      # [B, out, in]
        db = dZ.sum(-2)                       # [B, out]
        dWs[l], dbs[l] = (dW, db) if batched else (dW.sum(0), db.sum(0))
        a_out[l], dZ_out[l] = a, dZ
        dA = dZ @ (W if l == 0 else rb(W))
    return {"y": acts[-1], "dx": dA, "a": a_out, "dZ": dZ_out, "dW": dWs, "db": dbs, "batched": batched}


def row_contribution(res, l, rows, b=None):
    """(dW_l, db_l) of a dy that equals the pass's dy on `rows` (indices along the row axis) of set b
    (None: of every set) and is zero elsewhere: dZ_l[rows]^T a_l[rows], nothing else. With batched
    weights the result has every set's slab, zero for the sets that are not probed."""
    rows = torch.as_tensor(list(rows), dtype=torch.long).reshape(-1)
    dZ, a = res["dZ"][l][:, rows], res["a"][l][:, rows]
    if b is None:
        dW, db = _wt(dZ) @ a, dZ.sum(-2)
        return (dW, db) if res["batched"] else (dW.sum(0), db.sum(0))
    dWb, dbb = _wt(dZ[b]) @ a[b], dZ[b].sum(-2)
    if not res["batched"]:
        return dWb, dbb
    dW, db = torch.zeros((dZ.shape[0],) + dWb.shape, dtype=F64), torch.zeros((dZ.shape[0],) + dbb.shape, dtype=F64)
    dW[b], db[b] = dWb, dbb
    return dW, db


def per_row_err(a, ref):
    """[B, rows]: ||a[b, r] - ref[b, r]||_2 over the RMS over r of ||ref[b, r]||_2. The denominator is
    the set's RMS row norm, not the row's own: a single row's norm can be tiny (a dx row 1000 times
    below the median occurs in 4129 rows) without the row being any less accurate in absolute terms."""
    a, ref = torch.as_tensor(a).to(F64), torch.as_tensor(ref).to(F64)
    assert a.shape == ref.shape and a.dim() == 3, (a.shape, ref.shape)
    rn = torch.linalg.vector_norm(ref, dim=-1)
    rms = rn.pow(2).mean(-1, keepdim=True).sqrt()
    rms = torch.where(rms > 0, rms, torch.ones_like(rms))
    return torch.linalg.vector_norm(a - ref, dim=-1) / rms


# The row-local GPU cases, as arguments of test_gpu_arena_stack.problem (precision, dims, weight sets,
# rows per set, outermost_linear, seed): cases a, c, d, e, f, g, h of tests/golden/make_golden_stack_sizes.py
# with the rows made ragged as in the arena grid, a sine output layer, and the tiny row counts. The seed
# is the first draw at which the emulation meets the caps below (tests/test_rows_cpu.py asserts it): at
# seed 0, case a has a probed dx row (255) and tiny2 a dx row 0 so short that bf16 rounding alone moves
# it by 3.7e-2 and 8.6e-2 of its own length.
_D256x3 = (2, 256, 256, 256, 1)
ROW_CASES = {
    "a": ("bf16", (2, 256, 256, 256, 256, 1), 0, 4129, True, 1),    # 130 ring tiles, 17 forward rounds of 256 rows
    "c": ("bf16", _D256x3, 0, 333, True, 0),
    "d": ("bf16", (3, 128, 128, 128, 2), 0, 641, True, 0),
    "e": ("bf16", (16, 256, 256, 256, 2), 3, 500, True, 0),
    "f": ("bf16", (120, 256, 256, 256, 2), 2, 513, True, 0),
    "g": ("bf16", (2, 256, 256, 256, 256, 2), 65, 65, True, 0),     # sets shorter than a forward round
    "h": ("bf16", (2, 512, 512, 1), 0, 300, True, 0),               # the K = 512 kernels, 32-row tiles
    "sine": ("bf16", (3, 64, 64, 4), 0, 129, False, 0),
    "tiny1": ("bf16", _D256x3, 0, 1, True, 0),
    "tiny2": ("bf16", _D256x3, 0, 2, True, 1),
    "tiny31": ("bf16", _D256x3, 0, 31, True, 0),
    "tiny33": ("bf16", _D256x3, 0, 33, True, 0),
}
# The caps the CPU tests hold the bf16/bf16 emulation to on every case, and the GPU tests stand on: its
# worst per-row error of y and of dx, and its worst one-hot probe error (half of the 5e-2 the kernels get).
EMU_ROW_CAP = 0.1
EMU_PROBE_CAP = 2.5e-2
# What a wrong row must exceed (tests/test_rows_cpu.py pins that the wrong results the whole-tensor
# measure lets through do): K_ROW x EMU_ROW_CAP of tests/test_gpu_rows_stack.py must not exceed ROW_FLOOR.
ROW_FLOOR = 0.3
PROBE_FLOOR = 0.5


def probe_rows(rows):
    """The rows a one-hot probe visits: the edges of the 32-row ring and wave tiles, the 64-row fused
    tile, the 128-row TN tile, the 256-row forward round, and the tail."""
    cand = (0, 31, 32, 63, 64, 127, 128, 255, 256, rows - 33, rows - 32, rows - 2, rows - 1)
    return sorted({r for r in cand if 0 <= r < rows})


def probe_sets(sets):
    """First, a middle and the last weight set (shared weights: the one batch entry)."""
    return sorted({0, sets // 2, sets - 1}) if sets else [0]
