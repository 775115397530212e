"""GPU: the analytic-derivative entry points (siren_jvp_forward_ex / siren_jvp_backward_ex, orders 1-4,
with and without a primal buffer) and the fp64 stack (siren_mlp64_forward / siren_mlp64_backward) on a
poisoned arena (tests/_arena.py): `saved` and the workspace exactly as long as siren_jvp_saved_bytes /
siren_jvp_workspace_bytes (siren_mlp64_*) say, NaN bytes and 64 KiB guards all round.

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs; `saved` and the primal buffer over the backward), I3 (outputs written in full) hold, I5 every
output is bit-equal to the plain run (the derivative passes and the fp64 stack sum in fixed orders:
test_gpu_jvp_bits.py, test_f64_is_deterministic), and I6 the arena run meets the bounds of
test_gpu_jvp.py / test_gpu_hessian.py (values 1e-5 fp32, 5e-2 bf16, times 4 for second derivatives;
parameter and input gradients 1e-4 / 8e-2) or test_gpu_f64.py (1e-13) against the float64 oracle. I7: a
buffer one byte short is refused with SIREN_ENOSPACE before any launch; for the derivative workspace this
is the forward without `saved`, the one call that needs all of siren_jvp_workspace_bytes.

The 256-wide fp32 case runs under the options that choose between the slab layouts whose maximum
jlayout_of (rt_jvp.hip) takes: jvp_adj, jvp_tn2, jvp_tan, f32_rows."""
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
from make_golden_stack_sizes import setting  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402
from test_gpu_f64 import _params as f64_params  # noqa: E402
from test_gpu_jvp import TOL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
F32, F64, U8 = torch.float32, torch.float64, torch.uint8


def both(driver, *args):
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


def refused(driver, *args, short):
    plain = Plain(DEV)
    driver(plain, *args)
    arena = plain.arena()
    assert driver(arena, *args, short=short) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()


# ---------------------------------------------------------------------- the float64 oracle
def _derivative(order, y, x):
    if order == 1:
        return orc.gradient(y, x)
    if order == 2:
        return orc.laplace(y, x)
    rows = [torch.autograd.grad(y[..., c].sum(), x, create_graph=True)[0] for c in range(y.shape[-1])]
    if order == 3:
        return torch.stack(rows, dim=-2)
    return torch.stack([torch.stack([torch.autograd.grad(r[..., j].sum(), x, create_graph=True)[0]
                                     for j in range(x.shape[-1])], dim=-2) for r in rows], dim=-3)


@functools.lru_cache(maxsize=None)
def problem(prec, dims, sets, rows, order):
    dims = list(dims)
    g = torch.Generator().manual_seed(100 * order + rows + sets + dims[0])
    params = []
    for l in range(len(dims) - 1):
        W, b = orc.siren_init(dims, seed=order + l)[l]
        if sets:
            W = torch.stack([W * (1 + 0.05 * i) for i in range(sets)])
            b = torch.stack([b * (1 + 0.05 * i) for i in range(sets)])
        params.append((W.contiguous(), b.contiguous()))
    B = max(sets, 1)
    x = torch.rand(B, rows, dims[0], generator=g) * 2 - 1
    ps = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in params]
    xx = x.double().requires_grad_(True)
    v = _derivative(order, orc.siren_forward(xx, ps), xx)
    cot = torch.randn(v.shape, generator=g)
    (v * cot.double()).sum().backward()
    ref = {"value": v.detach(), "dx": xx.grad}
    for l, (W, b) in enumerate(ps):
        ref[f"dW{l}"] = W.grad
        ref[f"db{l}"] = b.grad if b.grad is not None else torch.zeros_like(b)  # the output bias gets zeros
    return {"prec": prec, "dims": dims, "sets": sets, "rows": rows, "order": order, "params": params, "x": x,
            "cot": cot, "ref": ref}


def run_jvp(alloc, p, primal, short=None):
    """siren_jvp_forward_ex into `saved`, the same without `saved`, siren_jvp_backward_ex with dx."""
    lib, st, order = _native.lib(), _native.stream_handle(DEV), p["order"]
    ws = [alloc.take(W.shape, F32, role="input", fill=W, name=f"W{l}") for l, (W, _) in enumerate(p["params"])]
    bs = [alloc.take(b.shape, F32, role="input", fill=b, name=f"b{l}") for l, (_, b) in enumerate(p["params"])]
    x = alloc.take(p["x"].shape, F32, role="input", fill=p["x"], name="x")
    cot = alloc.take(p["cot"].shape, F32, role="input", fill=p["cot"], name="dout")
    desc = _native.make_desc(p["dims"], ws, bs, w0=30.0, prec=_native.PRECISIONS[p["prec"]], outermost_linear=True,
                             weights_batched=p["sets"] > 0, batch=max(p["sets"], 1), rows_per_batch=p["rows"])
    dref = ctypes.byref(desc)
    sb, wb = int(lib.siren_jvp_saved_bytes(dref, order)), int(lib.siren_jvp_workspace_bytes(dref, order))
    assert sb > 0 and wb > 0, _native.last_error()
    pr, pb = None, 0
    if primal:  # the plain forward's saved buffer: the primal stream
        pb, pw = int(lib.siren_mlp_saved_bytes(dref)), int(lib.siren_mlp_workspace_bytes(dref))
        y = alloc.take(p["x"].shape[:-1] + (p["dims"][-1],), F32, role="output", name="y")
        pr = alloc.take((pb,), U8, role="scratch", name="primal")
        pwork = alloc.take((pw,), U8, role="scratch", name="primal_work")
        assert lib.siren_mlp_forward(dref, x.data_ptr(), y.data_ptr(), pr.data_ptr(), pb, pwork.data_ptr(), pw, st) == 0
        alloc.freeze("primal")
    gshape = p["x"].shape if order in (1, 2) else p["cot"].shape
    out = {}

    def forward(tag, saved, nbytes, wshort=0):
        work = alloc.take((wb,), U8, role="scratch", name="work_" + tag)
        # order 2: `grad` is scratch of the gradient's size, the Laplacian is the result
        grad = alloc.take(gshape, F32, role="scratch" if order == 2 else "output", name="grad_" + tag)
        lap = alloc.take(p["cot"].shape, F32, role="output", name="lap_" + tag) if order == 2 else None
        out["value_" + tag] = lap if order == 2 else grad
        return lib.siren_jvp_forward_ex(dref, order, x.data_ptr(), grad.data_ptr(), lap.data_ptr() if order == 2 else None,
                                        saved.data_ptr() if saved is not None else None, nbytes, work.data_ptr(),
                                        wb - wshort, pr.data_ptr() if primal else None, pb, st)
    if short == "work_fwd":
        return forward("nosaved", None, 0, wshort=1)
    saved = alloc.take((sb,), U8, role="scratch", name="saved")
    rc = forward("saved", saved, sb - (short == "saved_fwd"))
    if short == "saved_fwd":
        return rc
    assert rc == 0, _native.last_error()
    alloc.freeze("saved")
    if not short:
        assert forward("nosaved", None, 0) == 0, _native.last_error()
    n = len(ws)
    for l, (W, b) in enumerate(p["params"]):
        out[f"dW{l}"] = alloc.take(W.shape, F32, role="output", name=f"dW{l}")
        out[f"db{l}"] = alloc.take(b.shape, F32, role="output", name=f"db{l}")
    out["dx"] = alloc.take(p["x"].shape, F32, role="output", name="dx")
    work_b = alloc.take((wb,), U8, role="scratch", name="work_bwd")
    VP = ctypes.c_void_p * n
    rc = lib.siren_jvp_backward_ex(dref, order, x.data_ptr(), cot.data_ptr(), saved.data_ptr(), sb - (short == "saved_bwd"),
                                   work_b.data_ptr(), wb, VP(*[out[f"dW{l}"].data_ptr() for l in range(n)]),
                                   VP(*[out[f"db{l}"].data_ptr() for l in range(n)]), out["dx"].data_ptr(),
                                   pr.data_ptr() if primal else None, pb, st)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    return out


def check_oracle(p, out):
    tv, tg = TOL[p["prec"]]
    if p["order"] in (2, 4):
        tv = 4 * max(tv, 1e-5)  # test_gpu_jvp.py's Laplacian bound, test_gpu_hessian.py's _tol
    for k, v in out.items():
        if k.startswith("value"):
            ref = p["ref"]["value"]
            if p["order"] == 4:
                assert torch.equal(v, v.transpose(-1, -2)), "the Hessian is exactly symmetric"
            e, tol = orc.norm_rel(v.cpu().reshape(ref.shape), ref), tv
        elif k == f"db{len(p['params']) - 1}":
            assert not bool(v.any()), "the output bias's gradient is zeros"
            continue
        else:
            e, tol = orc.norm_rel(v.cpu(), p["ref"][k]), tg
        assert e < tol, f"I6: order {p['order']} {k} norm-rel {e:.3e} >= {tol}"


def _run_case(prec, dims, sets, rows, order, primal=False):
    p = problem(prec, dims, sets, rows, order)
    check_oracle(p, both(run_jvp, p, primal))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_jvp_small(prec, order):
    _run_case(prec, (2, 64, 64, 1), 0, 129, order)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_jvp_small_with_primal(order):
    _run_case("fp32", (2, 64, 64, 1), 0, 129, order, primal=True)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("s", ["default", "jvp_adj=0", "jvp_tn2=0", "jvp_tan=0", "f32_rows=0"])
def test_jvp_wide_fp32_slab_settings(s, order):
    with setting(s):
        _run_case("fp32", (2, 256, 256, 256, 1), 0, 333, order)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("dims,rows", [((3, 64, 64, 1), 65), ((1, 64, 64, 1), 33)])
def test_hessian_ragged(dims, rows, prec):
    _run_case(prec, dims, 0, rows, 4)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_jvp_batched_weights(prec, order):
    _run_case(prec, (2, 64, 64, 2), 3, 70, order)


@pytest.mark.parametrize("short", ["saved_fwd", "work_fwd", "saved_bwd"])
def test_jvp_short_buffer_is_refused_before_any_launch(short):
    p = problem("fp32", (2, 64, 64, 1), 0, 129, 1)
    plain = Plain(DEV)
    run_jvp(plain, p, False)
    arena = plain.arena()
    rc = run_jvp(arena, p, False, short=short)
    assert rc == ENOSPACE, (rc, _native.last_error())
    for r in arena.regions:  # the (full-size) forward before a refused backward wrote its own output
        if short == "saved_bwd" and r.name == "grad_saved":
            r.role = "scratch"
    arena.assert_nothing_launched()


# ---------------------------------------------------------------------- the fp64 stack
F64_DIMS = (3, 40, 72, 72, 2)


@functools.lru_cache(maxsize=None)
def problem64(sets, rows, outermost_linear):
    ps = f64_params(F64_DIMS, sets or None, seed=rows)
    g = torch.Generator().manual_seed(7 + rows)
    lead = (max(sets, 1), rows)
    x = torch.rand(lead + (F64_DIMS[0],), generator=g, dtype=F64) * 2 - 1
    dy = torch.randn(lead + (F64_DIMS[-1],), generator=g, dtype=F64)
    rp = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in ps]
    rx = x.clone().requires_grad_(True)
    y = orc.siren_forward(rx, rp, outermost_linear=outermost_linear)
    (y * dy).sum().backward()
    ref = {"y": y.detach(), "dx": rx.grad}
    for l, (W, b) in enumerate(rp):
        ref[f"dW{l}"], ref[f"db{l}"] = W.grad, b.grad
    return {"sets": sets, "rows": rows, "outermost_linear": outermost_linear, "params": ps, "x": x, "dy": dy, "ref": ref}


def run_mlp64(alloc, p, short=None):
    lib, st = _native.lib(), _native.stream_handle(DEV)
    ws = [alloc.take(W.shape, F64, role="input", fill=W, name=f"W{l}") for l, (W, _) in enumerate(p["params"])]
    bs = [alloc.take(b.shape, F64, role="input", fill=b, name=f"b{l}") for l, (_, b) in enumerate(p["params"])]
    x = alloc.take(p["x"].shape, F64, role="input", fill=p["x"], name="x")
    dy = alloc.take(p["dy"].shape, F64, role="input", fill=p["dy"], name="dy")
    desc = _native.make_desc(F64_DIMS, ws, bs, w0=30.0, prec=_native.PREC_F64, outermost_linear=p["outermost_linear"],
                             weights_batched=p["sets"] > 0, batch=max(p["sets"], 1), rows_per_batch=p["rows"])
    dref = ctypes.byref(desc)
    sb, wb = int(lib.siren_mlp64_saved_bytes(dref)), int(lib.siren_mlp64_workspace_bytes(dref))
    assert sb > 0 and wb > 0, _native.last_error()
    out = {"y": alloc.take(p["dy"].shape, F64, role="output", name="y")}
    saved = alloc.take((sb,), U8, role="scratch", name="saved")
    work_f = alloc.take((wb,), U8, role="scratch", name="work_fwd")
    rc = lib.siren_mlp64_forward(dref, x.data_ptr(), out["y"].data_ptr(), saved.data_ptr(), sb - (short == "saved_fwd"),
                                 work_f.data_ptr(), wb - (short == "work_fwd"), st)
    if short in ("saved_fwd", "work_fwd"):
        return rc
    assert rc == 0, _native.last_error()
    alloc.freeze("saved")
    if not short:
        out["y_nosaved"] = alloc.take(p["dy"].shape, F64, role="output", name="y_nosaved")
        work_n = alloc.take((wb,), U8, role="scratch", name="work_nosaved")
        assert lib.siren_mlp64_forward(dref, x.data_ptr(), out["y_nosaved"].data_ptr(), None, 0, work_n.data_ptr(), wb,
                                       st) == 0, _native.last_error()
    n = len(ws)
    for l, (W, b) in enumerate(p["params"]):
        out[f"dW{l}"] = alloc.take(W.shape, F64, role="output", name=f"dW{l}")
        out[f"db{l}"] = alloc.take(b.shape, F64, role="output", name=f"db{l}")
    out["dx"] = alloc.take(p["x"].shape, F64, role="output", name="dx")
    work_b = alloc.take((wb,), U8, role="scratch", name="work_bwd")
    VP = ctypes.c_void_p * n
    rc = lib.siren_mlp64_backward(dref, x.data_ptr(), dy.data_ptr(), saved.data_ptr(), sb - (short == "saved_bwd"),
                                  work_b.data_ptr(), wb - (short == "work_bwd"),
                                  VP(*[out[f"dW{l}"].data_ptr() for l in range(n)]),
                                  VP(*[out[f"db{l}"].data_ptr() for l in range(n)]), out["dx"].data_ptr(), st)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    return out


@pytest.mark.parametrize("outermost_linear", [True, False])
@pytest.mark.parametrize("sets,rows", [(0, 1000), (3, 333), (0, 1), (0, 65), (3, 1), (3, 65)])
def test_mlp64(sets, rows, outermost_linear):
    p = problem64(sets, rows, outermost_linear)
    out = both(run_mlp64, p)
    assert torch.equal(out["y"], out["y_nosaved"])
    for k, v in out.items():
        e = orc.norm_rel(v.cpu(), p["ref"]["y" if k == "y_nosaved" else k])
        assert e < 1e-13, f"I6: {k} norm-rel {e:.3e}"  # test_gpu_f64.py's bound


@pytest.mark.parametrize("short", ["saved_fwd", "work_fwd", "saved_bwd", "work_bwd"])
def test_mlp64_short_buffer_is_refused_before_any_launch(short):
    p = problem64(0, 65, True)
    plain = Plain(DEV)
    run_mlp64(plain, p)
    arena = plain.arena()
    rc = run_mlp64(arena, p, short=short)
    assert rc == ENOSPACE, (rc, _native.last_error())
    for r in arena.regions:
        if short.endswith("_bwd") and r.name == "y":
            r.role = "scratch"
    arena.assert_nothing_launched()
