"""CPU: Helmholtz fitting without a device. loss_functions.helmholtz_pml's expression path and
dataio.SingleHelmholtzSource against what the reference recorded (tests/golden/helmholtz.npz, written by
make_golden_helmholtz.py), the complex helpers, helmholtz_eval, the fake kernels of
siren_mri_amd::helmholtz_loss / helmholtz_loss_bwd, the two entry points' C ABI and the script's options."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helmholtz as _h  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native, dataio, helmholtz_eval, loss_functions, modules  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "experiment_scripts", "train_helmholtz.py")


@pytest.fixture(scope="module")
def golden():
    return _h.load_golden()


# ------------------------------------------------------------------ the data set
@pytest.mark.parametrize("velocity", _h.VELOCITIES)
def test_source_reproduces_reference_items(golden, velocity):
    ds = dataio.SingleHelmholtzSource(sidelength=48, velocity=velocity)
    assert len(ds) == 1
    inp, gt = ds[0]
    assert sorted(inp) == ["coords"]
    assert sorted(gt) == ["gt", "source_boundary_values", "squared_slowness", "squared_slowness_grid", "wavenumber"]
    p = f"hs/{velocity}/"
    for got, key, shape in ((inp["coords"], "coords", (2304, 2)), (gt["source_boundary_values"], "src", (2304, 2)),
                            (gt["squared_slowness"], "slow", (2304, 2)), (gt["squared_slowness_grid"], "slow_grid", (2304, 1))):
        ref = torch.from_numpy(golden[p + key])
        assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape == shape, key
        assert torch.equal(got, ref), (velocity, key)
    assert gt["wavenumber"] == float(golden["hs/wavenumber"]) == 20.0
    src = gt["source_boundary_values"]
    assert ((src == 0) | (src >= 1e-5)).all() and (src != 0).any(dim=1).sum() == 102
    assert (gt["squared_slowness"][:, 1] == 0).all()
    assert set(gt["squared_slowness"][:, 0].tolist()) == ({1.0} if velocity == "uniform" else {1.0, 0.25})


def test_closed_form_field_within_bound(golden, monkeypatch):
    """The field from torch.special's J0 - i Y0 against the reference's (scipy.special.hankel2), norm-relative.
    Measured on the CPU: 1.66e-7 at sidelength 48 and 1.85e-7 at 230 (profiles/helmholtz_loss_gpu_errors.txt); the
    bound is 8x the measured figure. (The issue that asked for this quotes 1.5e-7 at 230 for its own trial; the
    largest element-wise relative difference here is 4.9e-3, on elements next to a zero of the real or the
    imaginary part, where the reference's own float32 rounding is of that size.)"""
    for side, key, measured in ((48, "hs/field48", 1.66e-7), (230, "hs/field230", 1.85e-7)):
        field = dataio.SingleHelmholtzSource(sidelength=side).field
        ref = torch.from_numpy(golden[key])
        assert field.dtype == torch.float32 and field.shape == ref.shape == (side * side, 2)
        err = orc.norm_rel(field, ref)
        print(f"\n[helmholtz] closed-form field, sidelength {side}: norm-rel {err:.2e} (bound {8 * measured:.1e})")
        assert err <= 8 * measured
    # no scipy: with its import blocked the data set still builds its field and an item
    for name in [n for n in sys.modules if n == "scipy" or n.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "scipy", None)
    ds = dataio.SingleHelmholtzSource(sidelength=12)
    assert ds.field.shape == (144, 2) and ds[0][1]["gt"] is ds.field


# ------------------------------------------------------------------ the loss
def test_expression_path_matches_reference(golden):
    """The reference's dict and its parameter gradients on the fixture's model and batch. The terms to 1e-6
    relative, as test_wave_cpu.py; the gradients to 1e-6 norm-relative or 8x the reference's own float32
    error against float64 where that is larger (here the derivative of A u_0 is written out, there it is
    taken by autograd, so the two float32 runs round differently); and both against float64 within 8x the
    reference's own error."""
    m = _h.golden_model(golden)
    inp, gt = _h.golden_batch(golden)
    losses = loss_functions.helmholtz_pml(m(inp), gt)
    assert tuple(losses) == _h.KEYS
    sum(losses.values()).backward()
    for i, k in enumerate(_h.KEYS):
        assert losses[k].shape == () and losses[k].device.type == "cpu"
        assert losses[k].item() == pytest.approx(float(golden["e2e/terms32"][i]), rel=1e-6), k
        ref_err = float(golden["e2e/terms_ref32_rel"][i])
        assert losses[k].item() == pytest.approx(float(golden["e2e/terms64"][i]), rel=max(1e-6, 8 * ref_err)), k
    assert float(losses["data_term"]) == 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None, k  # the output bias too: y itself is in the loss
        bound = max(1e-6, 8 * float(golden["e2e/grad_ref32_normrel/" + k]))
        assert orc.norm_rel(p.grad, torch.from_numpy(golden["e2e/grad32/" + k])) < bound, k
        assert orc.norm_rel(p.grad, torch.from_numpy(golden["e2e/grad64/" + k])) < bound, k


def test_formula64_equals_the_fixture(golden):
    """The float64 formula the GPU tests compare the kernels with, on the fixture's synthetic set (where the
    generator held it to the unchanged reference); and the expression path in float64 on the same operands
    gives the same values, zero conventions and all."""
    ops = _h.golden_operands(golden)
    ref = tuple(torch.from_numpy(golden["op/" + k]) for k in ("terms64", "dpred64", "djac64", "dhess64"))
    x, pred, jac, hess, src, slow, k = ops
    p, j, h = (t.double().requires_grad_(True) for t in (pred, jac, hess))
    expr = loss_functions._helmholtz_expression(x.double(), p, j, h, src.double(), slow.double(), k.double())
    terms = torch.stack([expr[key].reshape(()) for key in _h.KEYS])
    (terms * torch.tensor(_h.C, dtype=torch.float64)).sum().backward()
    rz, ri = int(golden["op/row_zero"]), int(golden["op/row_interior"])
    for t, dp, dj, dh in (_h.formula64_grads(*ops, _h.C), (terms.detach(), p.grad, j.grad, h.grad)):
        assert torch.allclose(t, ref[0], rtol=1e-12, atol=0)
        assert orc.norm_rel(dp, ref[1]) < 1e-12 and orc.norm_rel(dj, ref[2]) < 1e-12 and orc.norm_rel(dh, ref[3]) < 1e-12
        assert all((gr.reshape(514, -1)[rz] == 0).all() for gr in (dp, dj, dh))
        assert (dj.reshape(514, -1)[ri] == 0).all()
        offdiag = ~torch.eye(2, dtype=torch.bool)
        assert (dh[..., offdiag] == 0).all()
    assert np.all(golden["op/terms_ref32_rel"] < 1e-6) and np.all(golden["e2e/terms_ref32_rel"] < 1e-6)


def test_expression_path_repeats_coefficients_over_fields():
    """C = 4 channels (two fields): each pair gets the coefficients and the slowness of the one-field loss."""
    x, pred, jac, hess, src, slow, k = _h.operands(1, 40, seed=3)
    _, pred2, jac2, hess2, src2, _, _ = _h.operands(1, 40, seed=4)
    one = [loss_functions._helmholtz_expression(x.double(), p.double(), j.double(), h.double(), s.double(), slow.double(),
                                                k.double()) for p, j, h, s in ((pred, jac, hess, src), (pred2, jac2, hess2, src2))]
    both = loss_functions._helmholtz_expression(x.double(), torch.cat((pred, pred2), -1).double(),
                                                torch.cat((jac, jac2), -2).double(), torch.cat((hess, hess2), -3).double(),
                                                torch.cat((src, src2), -1).double(), slow.double(), k.double())
    for key in _h.KEYS:
        assert float(both[key]) == pytest.approx(float(one[0][key]) + float(one[1][key]), rel=1e-12)


def test_inverse_problem_is_out_of_scope(golden):
    m = _h.golden_model(golden)
    inp, gt = _h.golden_batch(golden)
    for key in ("pretrain", "rec_boundary_values"):
        with pytest.raises(NotImplementedError, match="inverse problem.*out of scope"):
            loss_functions.helmholtz_pml(m(inp), dict(gt, **{key: torch.zeros(1)}))


def test_switch_is_named_like_the_wave_one():
    assert loss_functions._HELMHOLTZ_NATIVE is True
    loss_functions.set_helmholtz_loss_native(False)
    try:
        assert loss_functions._HELMHOLTZ_NATIVE is False
    finally:
        loss_functions.set_helmholtz_loss_native(True)


def test_native_does_not_apply_off_the_gpu():
    ops = _h.operands(1, 5, seed=1)
    x, pred, jac, hess, src, slow, k = ops
    assert not loss_functions._helmholtz_native_applies(x, pred, jac, hess, src, slow, k)
    losses = loss_functions._helmholtz_expression(*ops)
    assert losses["data_term"].device == pred.device and float(losses["data_term"]) == 0.0


# ------------------------------------------------------------------ complex helpers
def test_complex_helpers_against_python_complex():
    g = torch.Generator().manual_seed(0)
    for channels in (2, 6):
        x = torch.randn(3, 5, channels, generator=g, dtype=torch.float64)
        y = torch.randn(3, 5, channels, generator=g, dtype=torch.float64)
        before = (x.clone(), y.clone())
        got = {"conj": modules.compl_conj(x), "div": modules.compl_div(x, y), "mul": modules.compl_mul(x, y)}
        assert torch.equal(x, before[0]) and torch.equal(y, before[1])
        for name, t in got.items():
            assert t.shape == x.shape and t.dtype == x.dtype
        fx, fy = x.reshape(-1, channels).tolist(), y.reshape(-1, channels).tolist()
        for r, (rx, ry) in enumerate(zip(fx, fy)):
            for q in range(channels // 2):
                a, b = complex(rx[2 * q], rx[2 * q + 1]), complex(ry[2 * q], ry[2 * q + 1])
                for name, ref in (("conj", a.conjugate()), ("div", a / b), ("mul", a * b)):
                    v = got[name].reshape(-1, channels)[r]
                    assert complex(v[2 * q], v[2 * q + 1]) == pytest.approx(ref, rel=1e-12, abs=1e-14), (name, r, q)
    # differentiable, and broadcast over the pairs of a leading dimension
    a = torch.randn(4, 2, generator=g, requires_grad=True)
    modules.compl_mul(modules.compl_div(a, torch.randn(1, 2, generator=g)), modules.compl_conj(a)).sum().backward()
    assert a.grad is not None and torch.isfinite(a.grad).all()


# ------------------------------------------------------------------ dense evaluation
def test_helmholtz_field_ragged_chunks_equal_the_model_on_the_grid():
    torch.manual_seed(0)
    m = modules.SingleBVPNet(type="sine", in_features=2, out_features=2, hidden_features=32, num_hidden_layers=1)
    field = helmholtz_eval.helmholtz_field(m, 5, chunk=7)
    assert field.shape == (5, 5) and field.dtype == torch.complex64 and field.device.type == "cpu"
    assert not field.requires_grad and m.training
    with torch.no_grad():
        ref = m({"coords": dataio.get_mgrid(5)[None]})["model_out"].reshape(5, 5, 2)
    assert torch.allclose(torch.view_as_real(field), ref, rtol=0, atol=1e-6)


def test_relative_error_looks_inside_the_layer_only():
    ds = dataio.SingleHelmholtzSource(sidelength=9)
    side = 9
    ref = torch.complex(ds.field[:, 0], ds.field[:, 1]).view(side, side)
    assert helmholtz_eval.relative_error(ref, ds.field) == 0.0
    grid = dataio.get_mgrid(side).view(side, side, 2)
    inner = (grid[..., 0].abs() <= 0.5) & (grid[..., 1].abs() <= 0.5)
    assert int(inner.sum()) == 25  # -0.5, -0.25, 0, 0.25, 0.5 on both axes: the edge counts as inside
    outside = torch.where(inner, ref, ref + 7.0)
    assert helmholtz_eval.relative_error(outside, ds.field) == 0.0
    assert helmholtz_eval.relative_error(torch.where(inner, 2 * ref, ref), ds.field) == pytest.approx(1.0, rel=1e-6)


# ------------------------------------------------------------------ ops and ABI
def test_fake_kernels():
    with FakeTensorMode():
        for b, n in ((1, 2304), (2, 77)):
            x = torch.empty(b, n, 2, device="cuda")
            jac, hess = torch.empty(b, n, 2, 2, device="cuda"), torch.empty(b, n, 2, 2, 2, device="cuda")
            k = torch.empty(1, device="cuda")
            terms = torch.ops.siren_mri_amd.helmholtz_loss(x, x, jac, hess, x, x, k)
            assert terms.shape == (3,) and terms.dtype == torch.float32 and terms.device.type == "cuda"
            dpred, djac, dhess = torch.ops.siren_mri_amd.helmholtz_loss_bwd(x, x, jac, hess, x, x, k, terms)
            assert dpred.shape == x.shape and djac.shape == jac.shape and dhess.shape == hess.shape
            assert dpred.dtype == djac.dtype == dhess.dtype == torch.float32 and dhess.device.type == "cuda"


def test_op_schemas():
    ops = torch.ops.siren_mri_amd
    assert str(ops.helmholtz_loss.default._schema) == \
        ("siren_mri_amd::helmholtz_loss(Tensor x, Tensor pred, Tensor jac, Tensor hess, Tensor src, Tensor slowness, "
         "Tensor wavenumber) -> Tensor")
    assert str(ops.helmholtz_loss_bwd.default._schema) == \
        ("siren_mri_amd::helmholtz_loss_bwd(Tensor x, Tensor pred, Tensor jac, Tensor hess, Tensor src, Tensor slowness, "
         "Tensor wavenumber, Tensor g) -> (Tensor, Tensor, Tensor)")


def test_abi_declares_and_binds_the_entry_points():
    """As test_native_abi.py: the header's declarations, _native's signature table and the library's exports;
    then the argument checks that need no device."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siren_mri_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(siren_[a-z0-9_]+)\s*\(", text))
    lib = _native.load_library()
    for name in ("siren_helmholtz_loss_forward", "siren_helmholtz_loss_backward"):
        assert name in declared and name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    EINVAL, ENOSPACE = -1, -3
    fwd, bwd = lib.siren_helmholtz_loss_forward, lib.siren_helmholtz_loss_backward
    P = 256  # a dummy non-null pointer: nothing is launched by a refused call
    big = 1 << 20
    for k in range(7):  # every operand is required, the wavenumber too
        args = [P] * 7
        args[k] = None
        assert fwd(*args, 8, 8, P, P, big, None) == EINVAL, k
        assert "null pointer" in _native.last_error()
        assert bwd(*args, 8, 8, P, P, P, P, None) == EINVAL, k
    assert fwd(*[P] * 7, 8, 8, None, P, big, None) == EINVAL
    for k in range(4):  # g3, dpred, djac, dhess
        outs = [P] * 4
        outs[k] = None
        assert bwd(*[P] * 7, 8, 8, *outs, None) == EINVAL, k
    assert fwd(*[P] * 7, -1, 8, P, P, big, None) == EINVAL
    assert "rows=-1" in _native.last_error()
    assert bwd(*[P] * 7, -1, 8, P, P, P, P, None) == EINVAL
    assert fwd(*[P] * 7, 8, 0, P, P, big, None) == EINVAL
    assert "rows_per_batch=0" in _native.last_error()
    assert bwd(*[P] * 7, 8, 0, P, P, P, P, None) == EINVAL
    short = int(lib.siren_sse_workspace_bytes()) - 1
    assert fwd(*[P] * 7, 8, 8, P, P, short, None) == ENOSPACE
    assert "workspace" in _native.last_error()
    assert fwd(*[P] * 7, 8, 8, P, None, big, None) == ENOSPACE
    # rows == 0: the backward is a no-op
    assert bwd(*[None] * 7, 0, 0, None, None, None, None, None) == 0


# ------------------------------------------------------------------ the script's options
def test_script_help_and_scope():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--experiment_name", "--velocity", "--clip_grad", "--model", "--mode", "--device", "--sidelength",
                "--precision", "--checkpoint_path", "--lr", "--num_epochs"):
        assert opt in r.stdout, opt
    for extra in (["--mode", "pinn"], ["--mode", "rbf"], ["--model", "tanh"]):
        r = subprocess.run([sys.executable, SCRIPT, "--experiment_name", "x", "--device", "cpu", *extra],
                           capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0 and "NotImplementedError" in r.stderr and "out of scope" in r.stderr, extra
