"""GPU: the SIREN stack's entry points (siren_mlp_forward with and without `saved`, siren_mlp_backward_ex,
siren_mlp_forward_loss) on a poisoned arena (tests/_arena.py): every operand exactly as long as the ABI
says, NaN bytes and 64 KiB guards all round, x and dy at 8- / 4-byte alignment where the planned flags
say so.

Each driver runs twice on the same inputs, on ordinary zero-filled buffers and on the arena. After the
arena run: I1 no guard byte changed, I2 no input changed (`saved` included, over the backward), I3 every
output element written, I4 the loss workspace zero again; I5 every output bit-equal to the plain run (the
kernels are the same, only the neighbourhood differs; the suite asserts run-to-run bit equality of all of
these); I6 the arena result within test_gpu_siren_stack.py's TOL of the fp64 oracle, so the two runs
cannot be wrong together; I7 a buffer one byte short is refused with SIREN_ENOSPACE before any launch.

The grid is CASES x SETTINGS of tests/golden/make_golden_stack_sizes.py with the backward flag variants
of make_golden_stack_plan.py (those only the C ABI can be handed included), rows that are a multiple of
32 made ragged; then tiny row counts (1, 2, 31, 33: the clamped 16-byte reads of siren_gemm.hip), and a
sine output layer."""
import ctypes
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from _arena import Plain, same_bits  # noqa: E402
from make_golden_stack_plan import VARIANTS  # noqa: E402
from make_golden_stack_sizes import CASES, SETTINGS, setting  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402
from test_gpu_siren_stack import TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
RAGGED = {4096: 4129, 640: 641, 512: 513, 64: 65}
U8 = torch.uint8


@functools.lru_cache(maxsize=None)
def problem(prec, dims, sets, rows, outermost_linear=True, seed=0):
    """Parameters, x and dy of one shape (CPU fp32), and the fp64 oracle's y, gradients and dx. seed:
    another draw of the same shape (tests/test_gpu_rows_stack.py; 0 is the draw of this file's tests)."""
    dims = list(dims)
    g = torch.Generator().manual_seed(1000 * len(dims) + 7 * rows + sets + dims[0] + 100003 * seed)
    params = []
    for l in range(len(dims) - 1):
        W, b = orc.siren_init(dims, seed=rows + l + 1009 * seed)[l]
        if sets:
            W = W.unsqueeze(0).repeat(sets, 1, 1) * (1 + 0.1 * torch.randn(sets, 1, 1, generator=g))
            b = b.unsqueeze(0).repeat(sets, 1) + 0.01 * torch.randn(sets, dims[l + 1], generator=g)
        params.append((W.contiguous(), b.contiguous()))
    B = max(sets, 1)
    x = torch.rand(B, rows, dims[0], generator=g) * 2 - 1
    if dims[0] > 4:  # Fourier-feature coordinates
        x = torch.sin(x * 3.14)
    dy = torch.randn(B, rows, dims[-1], generator=g)
    ps = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in params]
    xx = x.double().requires_grad_(True)
    y = orc.siren_forward(xx, ps, 30.0, outermost_linear)
    (y * dy.double()).sum().backward()
    ref = {"y": y.detach(), "dx": xx.grad}
    for l, (W, b) in enumerate(ps):
        ref[f"dW{l}"], ref[f"db{l}"] = W.grad, b.grad
    return {"prec": prec, "dims": dims, "sets": sets, "rows": rows, "outermost_linear": outermost_linear,
            "params": params, "x": x, "dy": dy, "ref": ref}


def _operands(alloc, p, flags):
    """Weights, biases, x and dy as inputs, and the descriptor over them."""
    ws = [alloc.take(W.shape, torch.float32, role="input", fill=W, name=f"W{l}") for l, (W, _) in enumerate(p["params"])]
    bs = [alloc.take(b.shape, torch.float32, role="input", fill=b, name=f"b{l}") for l, (_, b) in enumerate(p["params"])]
    x = alloc.take(p["x"].shape, torch.float32, role="input", fill=p["x"], name="x", offset_bytes=0 if flags & 2 else 8)
    dy = alloc.take(p["dy"].shape, torch.float32, role="input", fill=p["dy"], name="dy",
                    offset_bytes=0 if flags & 4 else 4)
    desc = _native.make_desc(p["dims"], ws, bs, w0=30.0, prec=_native.PRECISIONS[p["prec"]],
                             outermost_linear=p["outermost_linear"], weights_batched=p["sets"] > 0,
                             batch=max(p["sets"], 1), rows_per_batch=p["rows"])
    return ws, bs, x, dy, desc


def _sizes(desc):
    lib = _native.lib()
    assert lib.siren_mlp_check(ctypes.byref(desc)) == 0, _native.last_error()
    return int(lib.siren_mlp_saved_bytes(ctypes.byref(desc))), int(lib.siren_mlp_workspace_bytes(ctypes.byref(desc)))


def run_stack(alloc, p, flags, short=None):
    """siren_mlp_forward into `saved`, siren_mlp_forward without it, siren_mlp_backward_ex. short: the
    buffer handed over one byte short ("saved_fwd", "work_fwd", "saved_bwd", "work_bwd"); the return
    code of that call is then the result."""
    lib, st = _native.lib(), _native.stream_handle(DEV)
    ws, bs, x, dy, desc = _operands(alloc, p, flags)
    sb, wb = _sizes(desc)
    out = {"y": alloc.take(p["dy"].shape, torch.float32, role="output", name="y")}
    saved = alloc.take((sb,), U8, role="scratch", name="saved")
    work_f = alloc.take((wb,), U8, role="scratch", name="work_fwd")
    dref = ctypes.byref(desc)
    if short in ("saved_fwd", "work_fwd"):
        return lib.siren_mlp_forward(dref, x.data_ptr(), out["y"].data_ptr(), saved.data_ptr(),
                                     sb - (short == "saved_fwd"), work_f.data_ptr(), wb - (short == "work_fwd"), st)
    rc = lib.siren_mlp_forward(dref, x.data_ptr(), out["y"].data_ptr(), saved.data_ptr(), sb, work_f.data_ptr(), wb, st)
    assert rc == 0, _native.last_error()
    alloc.freeze("saved")  # read-only from here on
    if short is None:
        out["y_nosaved"] = alloc.take(p["dy"].shape, torch.float32, role="output", name="y_nosaved")
        work_n = alloc.take((wb,), U8, role="scratch", name="work_nosaved")
        rc = lib.siren_mlp_forward(dref, x.data_ptr(), out["y_nosaved"].data_ptr(), None, 0, work_n.data_ptr(), wb, st)
        assert rc == 0, _native.last_error()
    for l, (W, b) in enumerate(p["params"]):
        out[f"dW{l}"] = alloc.take(W.shape, torch.float32, role="output", name=f"dW{l}")
        out[f"db{l}"] = alloc.take(b.shape, torch.float32, role="output", name=f"db{l}")
    if flags & 1:
        out["dx"] = alloc.take(p["x"].shape, torch.float32, role="output", name="dx")
    work_b = alloc.take((wb,), U8, role="scratch", name="work_bwd")
    n = len(ws)
    VP = ctypes.c_void_p * n
    rc = lib.siren_mlp_backward_ex(dref, x.data_ptr(), dy.data_ptr(), None, saved.data_ptr(),
                                   sb - (short == "saved_bwd"), work_b.data_ptr(), wb - (short == "work_bwd"),
                                   VP(*[out[f"dW{l}"].data_ptr() for l in range(n)]),
                                   VP(*[out[f"db{l}"].data_ptr() for l in range(n)]),
                                   out["dx"].data_ptr() if flags & 1 else None, st)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    return out


def both(driver, *args):
    """The driver on plain buffers and on an arena sized for the same takes: I1-I5."""
    plain = Plain(DEV)
    a = driver(plain, *args)
    plain.verify()
    arena = plain.arena()
    b = driver(arena, *args)
    arena.verify()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"I5: {k} differs between the plain and the arena run"
    return b


def check_oracle(p, out):
    """I6: the arena run against the fp64 oracle at test_gpu_siren_stack.py's tolerances."""
    ty, tg = TOL[p["prec"]]
    for k, v in out.items():
        ref = p["ref"]["y" if k == "y_nosaved" else k]
        e = orc.norm_rel(v.cpu(), ref)
        tol = ty if k.startswith("y") else tg
        assert e <= tol, f"I6: {k} norm-rel {e:.3e} > {tol}"


def _case_problem(case):
    prec, dims, sets, rows = CASES[case]
    return problem(prec, tuple(dims), sets, RAGGED.get(rows, rows))


@pytest.mark.parametrize("s", SETTINGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_stack_grid(case, s):
    p = _case_problem(case)
    with setting(s):
        for flags in VARIANTS[case]:
            check_oracle(p, both(run_stack, p, flags))


TINY = [("bf16", (2, 256, 256, 256, 1)), ("fp32", (2, 64, 64, 2))]


@pytest.mark.parametrize("sets,rows", [(0, 1), (0, 2), (0, 31), (0, 33), (3, 1), (3, 33)])
@pytest.mark.parametrize("prec,dims", TINY)
def test_stack_tiny_rows(prec, dims, sets, rows):
    p = problem(prec, dims, sets, rows)
    for flags in (7, 6, 1):
        check_oracle(p, both(run_stack, p, flags))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_stack_sine_output(prec):
    p = problem(prec, (3, 64, 64, 4), 0, 129, False)
    for flags in (7, 6):
        check_oracle(p, both(run_stack, p, flags))


@pytest.mark.parametrize("short", ["saved_fwd", "work_fwd", "saved_bwd", "work_bwd"])
@pytest.mark.parametrize("case", ["c", "j"])
def test_stack_short_buffer_is_refused_before_any_launch(case, short):
    """I7. For the backward the forward has run: its outputs are taken after it, so they must still be
    all ones; for the forward nothing at all may be written."""
    p = _case_problem(case)
    plain = Plain(DEV)
    run_stack(plain, p, 7)
    arena = plain.arena()
    rc = run_stack(arena, p, 7, short=short)
    assert rc == ENOSPACE, (rc, _native.last_error())
    for r in arena.regions:  # the (full-size) forward before a refused backward wrote y
        if short.endswith("_bwd") and r.name == "y":
            r.role = "scratch"
    arena.assert_nothing_launched()


# ---------------------------------------------------------------------- siren_mlp_forward_loss
@functools.lru_cache(maxsize=None)
def loss_problem(prec, dims, sets, rows, hf, dc, noise):
    p = dict(problem(prec, dims, sets, rows))
    g = torch.Generator().manual_seed(rows + sets)
    B, O = max(sets, 1), dims[-1]
    p["target"] = torch.randn(B, rows, O, generator=g)
    p["hf"] = (torch.rand(rows, generator=g) > 0.3).float() if hf else None
    p["k0"] = torch.randn(B, O, rows, generator=g) if dc else None
    p["mask"] = (torch.rand(B, O, rows, generator=g) > 0.5).float() if dc else None
    p["noise"], p["weight"] = noise, 1.0 / 128 ** 2
    return p


def run_forward_loss(alloc, p, short=None):
    lib, st = _native.lib(), _native.stream_handle(DEV)
    ws, bs, x, _, desc = _operands(alloc, p, 7)
    sb, wb = _sizes(desc)
    f32 = torch.float32

    def inp(name):
        return alloc.take(p[name].shape, f32, role="input", fill=p[name], name=name) if p[name] is not None else None
    tgt, hf, k0, mask = inp("target"), inp("hf"), inp("k0"), inp("mask")
    shape = p["dy"].shape
    out = {"y": alloc.take(shape, f32, role="output", name="y")}
    if k0 is not None:
        out["y_dc"] = alloc.take(shape, f32, role="output", name="y_dc")
    out["dy"] = alloc.take(shape, f32, role="output", name="dy_unit")
    out["loss"] = alloc.take((1,), f32, role="output", name="loss")
    lws_bytes = int(lib.siren_sse_workspace_bytes())
    lws = alloc.take((lws_bytes,), U8, role="zeroed", name="loss_ws")
    saved = alloc.take((sb,), U8, role="scratch", name="saved")
    work = alloc.take((wb,), U8, role="scratch", name="work")
    ld = _native.SirenLossDesc()
    ld.target = tgt.data_ptr()
    ld.k0 = k0.data_ptr() if k0 is not None else None
    ld.mask = mask.data_ptr() if mask is not None else None
    ld.hf = hf.data_ptr() if hf is not None else None
    ld.hf_len = p["rows"] if hf is not None else 0
    ld.noise, ld.weight = p["noise"], p["weight"]
    ld.y_dc = out["y_dc"].data_ptr() if k0 is not None else None
    ld.dy, ld.loss = out["dy"].data_ptr(), out["loss"].data_ptr()
    ld.loss_workspace, ld.loss_workspace_bytes = lws.data_ptr(), lws_bytes - (short == "loss_ws")
    rc = lib.siren_mlp_forward_loss(ctypes.byref(desc), ctypes.byref(ld), x.data_ptr(), out["y"].data_ptr(),
                                    saved.data_ptr(), sb - (short == "saved"), work.data_ptr(), wb - (short == "work"), st)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    return out


LOSS_CASES = {
    "img_bf16_hf": ("bf16", (2, 256, 256, 1), 0, 1089, True, False, 0.0),    # the register forward's epilogue
    "img_bf16": ("bf16", (2, 256, 256, 1), 0, 1089, False, False, 0.0),
    "img_fp32_hf": ("fp32", (2, 64, 64, 1), 0, 1089, True, False, 0.0),      # the per-layer path's output kernel
    "img_fp32": ("fp32", (2, 64, 64, 1), 0, 1089, False, False, 0.0),
    "dc_fp32": ("fp32", (2, 64, 64, 2), 2, 333, False, True, 0.0),
    "dc_fp32_noise": ("fp32", (2, 64, 64, 2), 2, 333, False, True, 0.25),
    "dc_bf16": ("bf16", (2, 128, 128, 2), 2, 333, False, True, 0.0),
    "dc_bf16_noise": ("bf16", (2, 128, 128, 2), 2, 333, False, True, 0.25),
}


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_forward_loss(name):
    p = loss_problem(*LOSS_CASES[name])
    out = both(run_forward_loss, p)
    ty, _ = TOL[p["prec"]]
    e = orc.norm_rel(out["y"].cpu(), p["ref"]["y"])
    assert e <= ty, f"I6: y norm-rel {e:.3e} > {ty}"
    # the loss and dL/dy of the y the kernel produced, in fp64 (the formulas of include/siren_mri_amd.h)
    y = out["y"].cpu().double()
    if p["k0"] is not None:
        m, k0 = (t.double().permute(0, 2, 1) for t in (p["mask"], p["k0"]))
        yd = (1 - m) * y + m * (k0 if p["noise"] <= 0 else (y + p["noise"] * k0) / (1 + p["noise"]))
        coef = (1 - m) + (0 if p["noise"] <= 0 else m / (1 + p["noise"]))
        assert orc.norm_rel(out["y_dc"].cpu(), yd) <= 1e-6
    else:
        yd, coef = y, 1.0
    hf = p["hf"].double().reshape(1, -1, 1) if p["hf"] is not None else 1.0
    d = hf * (yd - p["target"].double())
    loss = p["weight"] * float((d ** 2).sum())
    assert float(out["loss"]) == pytest.approx(loss, rel=1e-5)
    assert orc.norm_rel(out["dy"].cpu(), 2 * p["weight"] * hf * d * coef) <= 1e-6


@pytest.mark.parametrize("short", ["saved", "work", "loss_ws"])
def test_forward_loss_short_buffer_is_refused_before_any_launch(short):
    p = loss_problem(*LOSS_CASES["dc_fp32"])
    plain = Plain(DEV)
    run_forward_loss(plain, p)
    arena = plain.arena()
    assert run_forward_loss(arena, p, short=short) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()
