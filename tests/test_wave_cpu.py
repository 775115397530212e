"""CPU: wave-equation fitting without a device. loss_functions.wave_pml's expression path and
dataio.WaveSource against what the reference recorded (tests/golden/wave.npz, written by
make_golden_wave.py), the two velocity regions against their closed form, wave_eval.wave_field, the fake
kernels of siren_mri_amd::wave_loss / wave_loss_bwd and the two entry points' C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wave  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native, dataio, loss_functions, wave_eval  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return _wave.load_golden()


def test_expression_path_matches_reference(golden):
    """The reference's dict and its parameter gradients on the fixture's model and train-mode batch, to the
    bound test_sdf_cpu.py holds its expression path to (1e-6 relative; the gradients 1e-6 norm-relative)."""
    m = _wave.golden_model(golden)
    inp, gt = _wave.golden_batch(golden)
    losses = loss_functions.wave_pml(m(inp), gt)
    assert tuple(losses) == _wave.KEYS
    sum(losses.values()).backward()
    for i, k in enumerate(_wave.KEYS):
        assert losses[k].shape == ()
        assert losses[k].item() == pytest.approx(float(golden["e2e/terms32"][i]), rel=1e-6), k
    for k, p in m.named_parameters():
        assert p.grad is not None, k  # the output bias too: y itself is in the loss
        assert orc.norm_rel(p.grad, torch.from_numpy(golden["e2e/grad32/" + k])) < 1e-6, k


def test_pretrain_batch_has_no_pde_term(golden):
    m = _wave.golden_model(golden)
    inp, gt = _wave.golden_batch(golden, mode="pre")
    losses = loss_functions.wave_pml(m(inp), gt)
    assert tuple(losses) == _wave.KEYS and float(losses["diff_constraint_hom"]) == 0.0
    sum(v.sum() for v in losses.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_formula64_equals_the_fixture(golden):
    """The float64 formula the GPU tests compare the kernels with, on the fixture's synthetic set; and the
    expression path in float64 on the same operands gives the same values, zero conventions and all."""
    ops = _wave.golden_operands(golden)
    ref = tuple(torch.from_numpy(golden["op/" + k]) for k in ("terms64", "dpred64", "djac64", "dhess64"))
    pred, jac, hess, src, slow, mask = ops
    p, j, h = (t.double().requires_grad_(True) for t in (pred, jac, hess))
    expr = loss_functions._wave_expression(p, j, h, src.double(), slow.double(), mask, pred.shape[1])
    terms = torch.stack([expr[k] for k in _wave.KEYS])
    (terms * torch.tensor(_wave.C, dtype=torch.float64)).sum().backward()
    for t, dp, dj, dh in (_wave.formula64_grads(*ops, _wave.C), (terms.detach(), p.grad, j.grad, h.grad)):
        assert torch.allclose(t, ref[0], rtol=1e-12, atol=0)
        assert orc.norm_rel(dp, ref[1]) < 1e-12 and orc.norm_rel(dj, ref[2]) < 1e-12 and orc.norm_rel(dh, ref[3]) < 1e-12
        assert dp.reshape(-1)[int(golden["op/row_pred_eq_src"])] == 0
        assert dj.reshape(-1, 3)[int(golden["op/row_ut0"]), 0] == 0
        assert (dh.reshape(-1, 9)[int(golden["op/row_e0"])] == 0).all()
    # the end-to-end float64 terms are this formula's too (the generator asserts nothing about them)
    assert golden["e2e/terms64"].shape == (3,) and np.all(golden["e2e/terms_ref32_rel"] < 1e-6)


@pytest.mark.parametrize("mode,pretrain", [("pre", True), ("train", False)])
def test_wave_source_reproduces_reference_items(golden, mode, pretrain):
    """Two consecutive items per mode (the second has counter 1: the time ramp), bit for bit."""
    ds = dataio.WaveSource(sidelength=48, pretrain=pretrain)
    assert len(ds) == 1
    for item in (0, 1):
        inp, gt = ds[0]
        assert sorted(inp) == ["coords"]
        assert sorted(gt) == ["dirichlet_mask", "source_boundary_values", "squared_slowness", "squared_slowness_grid"]
        ref_inp, ref_gt = _wave.golden_item(golden, mode, item)
        assert inp["coords"].dtype == torch.float32 and inp["coords"].shape == (2304, 3)
        assert torch.equal(inp["coords"], ref_inp["coords"]), (mode, item)
        for k, ref in ref_gt.items():
            assert gt[k].dtype == ref.dtype and gt[k].shape == ref.shape == (2304, 1), k
            assert torch.equal(gt[k], ref), (mode, item, k)
        assert gt["squared_slowness_grid"].shape == (2304, 1) and (gt["squared_slowness_grid"] == 1).all()
    # the training mode's ramp: item 1 draws its times below 0.4 * 1 / 1e5, the last 2000 rows at the start
    t = inp["coords"][:, 0]
    if not pretrain:
        assert (t[-2000:] == 0).all() and t[:-2000].max() < 0.4 / 100e3 and t[:-2000].max() > 0
        assert torch.equal(gt["dirichlet_mask"][:, 0], t == 0)
        assert (gt["source_boundary_values"][~gt["dirichlet_mask"]] == 0).all()
    else:
        assert gt["dirichlet_mask"].all() and t.abs().max() <= 1e-3
    # the clamp: nothing below 1e-5 but 0
    bv = gt["source_boundary_values"]
    assert ((bv == 0) | (bv >= 1e-5)).all() and bv.max() > 1e-2


def test_wave_source_switches_pretraining_off_at_2000():
    ds = dataio.WaveSource(sidelength=4, pretrain=True)
    ds.N_src_samples = 4
    ds.counter = 1998
    ds[0]
    assert ds.pretrain is True and ds.counter == 1999
    ds[0]
    assert ds.pretrain is False and ds.counter == 0
    _, gt = ds[0]  # a training item now: counter 0, an empty time window
    assert ds.counter == 1 and gt["dirichlet_mask"].all()
    inp, gt = ds[0]
    assert not gt["dirichlet_mask"].all() and gt["dirichlet_mask"][-8:].all()


@pytest.mark.parametrize("velocity", ["square", "circle"])
def test_velocity_regions_closed_form(velocity):
    """1/4 inside the region, 1 outside, decided by the two spatial columns (the reference's two branches
    raise: DESIGN.md §8)."""
    ds = dataio.WaveSource(sidelength=48, velocity=velocity)
    ds[0]
    inp, gt = ds[0]
    x, y = inp["coords"][:, 1].double(), inp["coords"][:, 2].double()
    inside = ((x.abs() < 0.3) & (y.abs() < 0.3)) if velocity == "square" else (torch.sqrt(x * x + y * y) < 0.1)
    near = ((x.abs() - 0.3).abs() < 1e-6) | ((y.abs() - 0.3).abs() < 1e-6) if velocity == "square" \
        else (torch.sqrt(x * x + y * y) - 0.1).abs() < 1e-6
    slow = gt["squared_slowness"]
    assert slow.shape == (2304, 1) and slow.dtype == torch.float32
    assert inside.any() and (~inside).any()
    keep = ~near
    assert torch.equal(slow[keep, 0], torch.where(inside, 0.25, 1.0).float()[keep])
    # time plays no part: column 0 is not looked at
    moved = inp["coords"].clone()
    moved[:, 0] = 0.9
    assert torch.equal(ds.get_squared_slowness(moved), slow[:, 0])
    # and the grid's slowness, on the 2-column grid
    gx, gy = ds.mgrid[:, 0], ds.mgrid[:, 1]
    gin = ((gx.abs() < 0.3) & (gy.abs() < 0.3)) if velocity == "square" else (torch.sqrt(gx ** 2 + gy ** 2) < 0.1)
    assert torch.equal(gt["squared_slowness_grid"][:, 0], torch.where(gin, 0.25, 1.0).float())


def test_gaussian_is_the_density():
    x = torch.tensor([[0.0, 0.0], [0.01, -0.02]])
    got = dataio.gaussian(x, mu=torch.zeros(1, 2), sigma=5e-4, d=2)
    assert got.dtype == torch.float32 and got.shape == (2,)
    ref = 1 / (2 * np.pi * 5e-4) * np.exp(-0.5 * np.array([0.0, 5e-4]) / 5e-4)
    assert np.allclose(got.numpy(), ref, rtol=1e-5)


def test_wave_field_ragged_chunks_equal_the_model_on_the_grid():
    from siren_mri_amd import modules
    torch.manual_seed(0)
    m = modules.SingleBVPNet(type="sine", in_features=3, hidden_features=32, num_hidden_layers=1)
    field = wave_eval.wave_field(m, 0.25, N=5, max_batch=7)
    assert field.shape == (5, 5) and field.dtype == torch.float32 and field.device.type == "cpu"
    assert not field.requires_grad and m.training
    rows = torch.cat((torch.full((25, 1), 0.25), dataio.get_mgrid(5)), dim=1)
    with torch.no_grad():
        ref = m({"coords": rows[None]})["model_out"].reshape(5, 5)
    assert torch.allclose(field, ref, rtol=0, atol=1e-6)
    with torch.no_grad():
        one = m({"coords": torch.tensor([[[0.25, -1 + 2 * 1 / 4, -1 + 2 * 3 / 4]]])})["model_out"]
    assert float(field[1, 3]) == pytest.approx(float(one), abs=1e-6)


def test_fake_kernels():
    with FakeTensorMode():
        for b, n in ((1, 2304), (2, 77)):
            pred = torch.empty(b, n, 1, device="cuda")
            jac = torch.empty(b, n, 1, 3, device="cuda")
            hess = torch.empty(b, n, 1, 3, 3, device="cuda")
            mask = torch.empty(b, n, 1, device="cuda", dtype=torch.bool)
            for h in (hess, None):
                terms = torch.ops.siren_mri_amd.wave_loss(pred, jac, h, pred, pred, mask)
                assert terms.shape == (3,) and terms.dtype == torch.float32 and terms.device.type == "cuda"
                dpred, djac, dhess = torch.ops.siren_mri_amd.wave_loss_bwd(pred, jac, h, pred, pred, mask, terms)
                assert dpred.shape == pred.shape and djac.shape == jac.shape
                assert dhess.shape == (hess.shape if h is not None else (0,))
                assert dpred.dtype == djac.dtype == dhess.dtype == torch.float32 and dhess.device.type == "cuda"


def test_op_schemas():
    ops = torch.ops.siren_mri_amd
    assert str(ops.wave_loss.default._schema) == \
        "siren_mri_amd::wave_loss(Tensor pred, Tensor jac, Tensor? hess, Tensor src, Tensor slowness, Tensor mask) -> Tensor"
    assert str(ops.wave_loss_bwd.default._schema) == \
        ("siren_mri_amd::wave_loss_bwd(Tensor pred, Tensor jac, Tensor? hess, Tensor src, Tensor slowness, Tensor mask, "
         "Tensor g) -> (Tensor, Tensor, Tensor)")


def test_abi_declares_and_binds_the_entry_points():
    """As test_native_abi.py: the header's declarations, _native's signature table and the library's exports;
    then the argument checks that need no device."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siren_mri_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(siren_[a-z0-9_]+)\s*\(", text))
    lib = _native.load_library()
    for name in ("siren_wave_loss_forward", "siren_wave_loss_backward"):
        assert name in declared and name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    EINVAL, ENOSPACE = -1, -3
    fwd, bwd = lib.siren_wave_loss_forward, lib.siren_wave_loss_backward
    P = 256  # a dummy non-null pointer: nothing is launched by a refused call
    big = 1 << 20
    # a null required pointer with rows > 0 (hess may be null)
    for k in (0, 1, 3, 4, 5):
        args = [P] * 6
        args[k] = None
        assert fwd(*args, 8, 8, P, P, big, None) == EINVAL, k
        assert "null pointer" in _native.last_error()
        assert bwd(*args, 8, 8, P, P, P, P, None) == EINVAL, k
    assert fwd(P, P, P, P, P, P, 8, 8, None, P, big, None) == EINVAL
    for k in (0, 1, 2):  # g3, dpred, djac
        outs = [P, P, P]
        outs[k] = None
        assert bwd(P, P, P, P, P, P, 8, 8, *outs, P, None) == EINVAL, k
    # rows < 0; rows_per_batch < 1 with rows > 0
    assert fwd(P, P, P, P, P, P, -1, 8, P, P, big, None) == EINVAL
    assert "rows=-1" in _native.last_error()
    assert bwd(P, P, P, P, P, P, -1, 8, P, P, P, P, None) == EINVAL
    assert fwd(P, P, P, P, P, P, 8, 0, P, P, big, None) == EINVAL
    assert "rows_per_batch=0" in _native.last_error()
    assert bwd(P, P, P, P, P, P, 8, 0, P, P, P, P, None) == EINVAL
    # dhess is null exactly when hess is
    assert bwd(P, P, P, P, P, P, 8, 8, P, P, P, None, None) == EINVAL
    assert "go together" in _native.last_error()
    assert bwd(P, P, None, P, P, P, 8, 8, P, P, P, P, None) == EINVAL
    # a short or missing workspace
    short = int(lib.siren_sse_workspace_bytes()) - 1
    assert fwd(P, P, P, P, P, P, 8, 8, P, P, short, None) == ENOSPACE
    assert "workspace" in _native.last_error()
    assert fwd(P, P, None, P, P, P, 8, 8, P, None, big, None) == ENOSPACE
    # rows == 0: the backward is a no-op
    assert bwd(None, None, None, None, None, None, 0, 0, None, None, None, None, None) == 0


def test_switch_is_named_like_the_sdf_one():
    assert loss_functions._WAVE_NATIVE is True
    loss_functions.set_wave_loss_native(False)
    try:
        assert loss_functions._WAVE_NATIVE is False
    finally:
        loss_functions.set_wave_loss_native(True)


def test_native_does_not_apply_off_the_gpu():
    pred, jac, hess, src, slow, mask = _wave.operands(1, 5, seed=1)
    assert not loss_functions._wave_native_applies(pred, jac, hess, src, slow, mask)
    losses = loss_functions._wave_expression(pred, jac, None, src, slow, mask, 5)
    assert losses["diff_constraint_hom"].device == pred.device and float(losses["diff_constraint_hom"]) == 0.0
