"""CPU: signed-distance fitting without a device. loss_functions.sdf's expression path and
dataio.PointCloud against what the reference recorded (tests/golden/sdf.npz, written by
make_golden_sdf.py), the synthetic point clouds, sdf_meshing.sdf_volume, the fake kernels of
siren_mri_amd::sdf_loss / sdf_loss_bwd and the two entry points' C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sdf  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native, dataio, loss_functions, sdf_meshing  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return _sdf.load_golden()


def test_expression_path_matches_reference(golden):
    """The reference's dict and its parameter gradients on the fixture's model and batch, to the bound
    test_api_cpu.test_losses_match_reference_values holds the other losses to (1e-6 relative; the
    gradients 1e-6 norm-relative)."""
    m = _sdf.golden_model(golden)
    inp, gt = _sdf.golden_batch(golden)
    losses = loss_functions.sdf(m(inp), gt)
    assert tuple(losses) == _sdf.KEYS
    sum(losses.values()).backward()
    for i, k in enumerate(_sdf.KEYS):
        assert losses[k].shape == ()
        assert losses[k].item() == pytest.approx(float(golden["e2e/terms32"][i]), rel=1e-6), k
    for k, p in m.named_parameters():
        assert p.grad is not None, k  # the output bias too: y itself is in the loss
        assert orc.norm_rel(p.grad, torch.from_numpy(golden["e2e/grad32/" + k])) < 1e-6, k


@pytest.mark.parametrize("tag", ["d3", "d2"])
def test_op_level_sets(golden, monkeypatch, tag):
    """pred and grad as independent leaves (the gradient operator replaced, as the generator does), planted
    zero rows included: the expression path in float64 reproduces the reference's float64 record, and so
    does the float64 formula the GPU tests compare the kernels with (zero conventions and all)."""
    pred, grad, sdf, normals = (torch.from_numpy(golden[f"{tag}/{k}"]) for k in ("pred", "grad", "sdf", "normals"))
    ref_t, ref_dp, ref_dg = (torch.from_numpy(golden[f"{tag}/{k}"]) for k in ("terms64", "dpred64", "dgrad64"))
    p, g = pred.double().requires_grad_(True), grad.double().requires_grad_(True)
    monkeypatch.setattr(loss_functions.diff_operators, "gradient", lambda y, x: g)
    losses = loss_functions.sdf({"model_in": None, "model_out": p}, {"sdf": sdf.double(), "normals": normals.double()})
    terms = torch.stack([losses[k] for k in _sdf.KEYS])
    (terms * torch.tensor(_sdf.C, dtype=torch.float64)).sum().backward()
    for t, dp, dg in ((terms.detach(), p.grad, g.grad), _sdf.formula64_grads(pred, grad, sdf, normals, _sdf.C)):
        assert torch.allclose(t, ref_t, rtol=1e-12, atol=0)
        assert orc.norm_rel(dp, ref_dp) < 1e-12 and orc.norm_rel(dg, ref_dg) < 1e-12
        assert (dp.reshape(-1)[torch.from_numpy(np.concatenate([golden[f"{tag}/pred0_on"], golden[f"{tag}/pred0_off"]]))] == 0).all()


@pytest.mark.parametrize("tag,keep", [("keep", True), ("free", False)])
def test_point_cloud_reproduces_reference_samples(golden, tmp_path, tag, keep):
    path = tmp_path / "cloud.xyz"
    np.savetxt(path, golden["pc/cloud"], fmt="%.18e")
    ds = dataio.PointCloud(str(path), on_surface_points=16, keep_aspect_ratio=keep)
    assert len(ds) == 4
    np.random.seed(0)
    inp, gt = ds[0]
    assert sorted(inp) == ["coords"] and sorted(gt) == ["normals", "sdf"]
    for got, key in ((inp["coords"], "coords"), (gt["sdf"], "sdf"), (gt["normals"], "normals")):
        ref = golden[f"pc/{tag}/{key}"]
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        assert np.array_equal(got.numpy(), ref), key
    assert (gt["sdf"][:16] == 0).all() and (gt["sdf"][16:] == -1).all() and (gt["normals"][16:] == -1).all()


@pytest.mark.parametrize("shape", ["torus", "sphere"])
def test_synthetic_point_cloud(tmp_path, shape):
    path = tmp_path / f"{shape}.xyz"
    ret = dataio.write_synthetic_point_cloud(str(path), shape=shape, n=500, seed=3)
    cloud = np.genfromtxt(path)
    assert cloud.shape == (500, 6) and np.allclose(cloud, ret, atol=1e-11)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    assert np.abs(np.linalg.norm(cloud[:, 3:], axis=1) - 1).max() < 1e-6
    if shape == "torus":
        R, r = dataio.TORUS_RADII
        implicit = (np.sqrt(x ** 2 + y ** 2) - R) ** 2 + z ** 2 - r ** 2
        centre = np.stack((R * x, R * y, 0 * z), axis=1) / np.sqrt(x ** 2 + y ** 2)[:, None]
        outward = (cloud[:, :3] - centre) / r
    else:
        implicit = x ** 2 + y ** 2 + z ** 2 - dataio.SPHERE_RADIUS ** 2
        outward = cloud[:, :3] / dataio.SPHERE_RADIUS
    assert np.abs(implicit).max() < 1e-6
    assert np.abs(outward - cloud[:, 3:]).max() < 1e-6  # the exact outward normals
    # uniform by area: the outer half of the torus (cos v > 0) holds 1/2 + r / (pi R) of it
    if shape == "torus":
        frac = np.mean(np.sqrt(x ** 2 + y ** 2) > R)
        assert abs(frac - (0.5 + r / (np.pi * R))) < 0.08
    assert np.array_equal(dataio.write_synthetic_point_cloud(str(tmp_path / "again.xyz"), shape=shape, n=500, seed=3), ret)
    ds = dataio.PointCloud(str(path), on_surface_points=100)
    assert len(ds) == 5
    assert ds.coords.min() >= -1 and ds.coords.max() <= 1
    inp, _ = ds[0]
    assert inp["coords"].shape == (200, 3) and inp["coords"].abs().max() <= 1
    with pytest.raises(ValueError, match="unknown shape"):
        dataio.write_synthetic_point_cloud(str(path), shape="cube")


def test_sdf_volume_ragged_chunks_equal_the_model_on_the_grid():
    from siren_mri_amd import modules
    torch.manual_seed(0)
    m = modules.SingleBVPNet(type="sine", in_features=3, hidden_features=32, num_hidden_layers=1)
    vol = sdf_meshing.sdf_volume(m, N=5, max_batch=7)
    assert vol.shape == (5, 5, 5) and vol.dtype == torch.float32 and vol.device.type == "cpu" and not vol.requires_grad
    with torch.no_grad():
        ref = m({"coords": dataio.get_mgrid(5, dim=3)[None]})["model_out"].reshape(5, 5, 5)
    assert torch.allclose(vol, ref, rtol=0, atol=1e-6)
    # the sample order: volume[i0, i1, i2] is the model at (-1 + 2 i_k / 4)_k
    with torch.no_grad():
        one = m({"coords": torch.tensor([[[-1 + 2 * 1 / 4, -1 + 2 * 3 / 4, -1 + 2 * 2 / 4]]])})["model_out"]
    assert float(vol[1, 3, 2]) == pytest.approx(float(one), abs=1e-6)
    assert m.training


def test_create_mesh_names_its_missing_dependencies(tmp_path):
    try:
        import plyfile  # noqa: F401
        import skimage.measure  # noqa: F401
    except ImportError:
        from siren_mri_amd import modules
        m = modules.SingleBVPNet(type="sine", in_features=3, hidden_features=32, num_hidden_layers=1)
        with pytest.raises(ImportError, match="skimage|plyfile"):
            sdf_meshing.create_mesh(m, str(tmp_path / "mesh"), N=5)
        assert not (tmp_path / "mesh.ply").exists()


def test_fake_kernels():
    with FakeTensorMode():
        for b, n, d in ((2, 1400, 3), (1, 77, 2)):
            pred = torch.empty(b, n, 1, device="cuda")
            grad = torch.empty(b, n, d, device="cuda")
            terms = torch.ops.siren_mri_amd.sdf_loss(pred, grad, pred, grad)
            assert terms.shape == (4,) and terms.dtype == torch.float32 and terms.device.type == "cuda"
            dpred, dgrad = torch.ops.siren_mri_amd.sdf_loss_bwd(pred, grad, pred, grad, terms)
            assert dpred.shape == pred.shape and dgrad.shape == grad.shape
            assert dpred.dtype == dgrad.dtype == torch.float32 and dgrad.device.type == "cuda"


def test_op_schemas():
    ops = torch.ops.siren_mri_amd
    assert str(ops.sdf_loss.default._schema) == \
        "siren_mri_amd::sdf_loss(Tensor pred, Tensor grad, Tensor sdf, Tensor normals) -> Tensor"
    assert str(ops.sdf_loss_bwd.default._schema) == \
        "siren_mri_amd::sdf_loss_bwd(Tensor pred, Tensor grad, Tensor sdf, Tensor normals, Tensor g) -> (Tensor, Tensor)"


def test_abi_declares_and_binds_the_entry_points():
    """As test_native_abi.py: the header's declarations, _native's signature table and the library's exports."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siren_mri_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(siren_[a-z0-9_]+)\s*\(", text))
    lib = _native.load_library()
    for name in ("siren_sdf_loss_forward", "siren_sdf_loss_backward"):
        assert name in declared and name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    # argument checks that need no device
    EINVAL, ENOSPACE = -1, -3
    assert lib.siren_sdf_loss_forward(256, 256, 256, 256, 8, 4, 256, 256, 1 << 20, None) == EINVAL
    assert "dims 4" in _native.last_error()
    assert lib.siren_sdf_loss_backward(256, 256, 256, 256, 8, 1, 256, 256, 256, None) == EINVAL
    assert lib.siren_sdf_loss_forward(256, None, 256, 256, 8, 3, 256, 256, 1 << 20, None) == EINVAL
    assert "null pointer" in _native.last_error()
    assert lib.siren_sdf_loss_backward(256, 256, 256, 256, 8, 3, None, 256, 256, None) == EINVAL
    assert lib.siren_sdf_loss_forward(256, 256, 256, 256, -1, 3, 256, 256, 1 << 20, None) == EINVAL
    short = int(lib.siren_sse_workspace_bytes()) - 1
    assert lib.siren_sdf_loss_forward(256, 256, 256, 256, 8, 3, 256, 256, short, None) == ENOSPACE
    assert "workspace" in _native.last_error()
    assert lib.siren_sdf_loss_backward(None, None, None, None, 0, 3, None, None, None, None) == 0  # rows == 0: a no-op


def test_switch_is_named_like_the_kspace_one():
    assert loss_functions._SDF_NATIVE is True
    loss_functions.set_sdf_loss_native(False)
    try:
        assert loss_functions._SDF_NATIVE is False
    finally:
        loss_functions.set_sdf_loss_native(True)
