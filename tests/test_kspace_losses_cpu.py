"""CPU: the k-space loss family of the MRI fork (loss_functions.py:12-64, 103-235, 295-323) — the
expression path against the reference's values recorded in golden/kspace_losses.npz
(make_golden_kspace_losses.py), the image_hypernetwork_* wrappers, the fake kernels and argument
checks of kspace_loss / kspace_loss_bwd (siren_kloss.hip), and the scripts' --loss helper."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from siren_mri_amd import _native, loss_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NAMES = ("image_mse_log", "image_mse_cubic", "image_smape", "image_asinh", "image_perp", "kspace_l1",
         "ift_image_mse", "image_l1")
WRAPPERS = {"image_hypernetwork_perp_loss": "image_perp", "image_hypernetwork_asinh_loss": "image_asinh",
            "image_hypernetwork_l1_loss": "kspace_l1", "image_hypernetwork_log_loss": "image_mse_log",
            "image_hypernetwork_cubic_loss": "image_mse_cubic", "image_hypernetwork_ift_loss": "ift_image_mse"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "kspace_losses.npz"), allow_pickle=False)


def _run(name, pred, tgt):
    p = pred.clone().requires_grad_(True)
    out = getattr(loss_functions, name)(None, {"model_out": p}, {"img": tgt})
    assert list(out) == ["img_loss"] and out["img_loss"].dim() == 0
    out["img_loss"].backward()
    return out["img_loss"].detach(), p.grad


@pytest.mark.parametrize("name", NAMES)
def test_expression_path_float64(golden, name):
    """The reference's float64 loss and gradient, to 1e-12 relative (the same expression, in torch)."""
    loss, grad = _run(name, torch.from_numpy(golden["pred"]).double(), torch.from_numpy(golden["tgt"]).double())
    ref_l, ref_g = float(golden[name + "_loss64"]), torch.from_numpy(golden[name + "_grad64"])
    assert loss.dtype == torch.float64
    assert abs(float(loss) - ref_l) <= 1e-12 * abs(ref_l)
    assert torch.linalg.vector_norm(grad - ref_g).item() <= 1e-12 * torch.linalg.vector_norm(ref_g).item()
    assert torch.isfinite(grad).all()


@pytest.mark.parametrize("name", NAMES)
def test_expression_path_float32(golden, name):
    """The reference's float32 loss, within 4x the reference's own float32-against-float64 error."""
    loss, grad = _run(name, torch.from_numpy(golden["pred"]), torch.from_numpy(golden["tgt"]))
    ref = float(golden[name + "_loss32"])
    assert loss.dtype == torch.float32 and torch.isfinite(grad).all()
    assert abs(float(loss) - ref) <= 4 * float(golden[name + "_ref32_loss_rel"]) * abs(ref)


def test_expression_path_ties_and_zeros(golden):
    """Pixels with pred == tgt (the planted ties and both-zero pixels) get a gradient of exactly 0 from
    the six k-space kinds, in float32 too."""
    pred, tgt = torch.from_numpy(golden["pred"]), torch.from_numpy(golden["tgt"])
    rows = torch.arange(pred.shape[0])[:, None]
    for name in NAMES[:6]:
        _, grad = _run(name, pred, tgt)
        for key in ("tie_idx", "both0_idx"):
            assert (grad[rows, torch.from_numpy(golden[key])] == 0).all(), (name, key)


def test_masked_compositions():
    """ift_image_mse and image_l1 with a mask: the reference's expressions (loss_functions.py:229, 235)."""
    g = torch.Generator().manual_seed(2)
    pred = torch.randn(2, 64, 2, generator=g, dtype=torch.float64)
    tgt = torch.randn(2, 64, 2, generator=g, dtype=torch.float64)
    m_img = (torch.rand(2, 8, 8, generator=g) < 0.5).double()
    cp = torch.complex(pred[..., 0], pred[..., 1]).view(2, 8, 8)
    ct = torch.complex(tgt[..., 0], tgt[..., 1]).view(2, 8, 8)
    want = ((m_img * (torch.fft.ifft2(cp).abs() - torch.fft.ifft2(ct).abs()) ** 2).sum() + 1e-8 * cp.abs().sum()
            + 0.0025 * ((pred - tgt) ** 2).sum())
    got = loss_functions.ift_image_mse(m_img, {"model_out": pred}, {"img": tgt})["img_loss"]
    assert float(got) == pytest.approx(float(want), rel=1e-12)
    m = (torch.rand(2, 64, 2, generator=g) < 0.5).double()
    got = loss_functions.image_l1(m, {"model_out": pred}, {"img": tgt})["img_loss"]
    assert float(got) == pytest.approx(float((m * (pred - tgt).abs()).mean()), rel=1e-12)


@pytest.mark.parametrize("wrapper", sorted(WRAPPERS))
def test_hypernetwork_wrappers(wrapper):
    g = torch.Generator().manual_seed(5)
    out = {"model_out": torch.randn(2, 16, 2, generator=g), "latent_vec": torch.randn(2, 8, generator=g),
           "hypo_params": {"a.weight": torch.randn(2, 4, 3, generator=g), "a.bias": torch.randn(2, 4, generator=g)}}
    gt = {"img": torch.randn(2, 16, 2, generator=g)}
    kl, fw = 1.07e-9, 1.11e-7
    got = getattr(loss_functions, wrapper)(None, kl, fw, out, gt)
    assert list(got) == ["img_loss", "latent_loss", "hypo_weight_loss"] == list(
        loss_functions.image_hypernetwork_loss(None, kl, fw, out, gt))
    assert torch.equal(got["latent_loss"], kl * loss_functions.latent_loss(out))
    assert torch.equal(got["hypo_weight_loss"], fw * loss_functions.hypo_weight_loss(out))
    assert torch.equal(got["img_loss"], getattr(loss_functions, WRAPPERS[wrapper])(None, out, gt)["img_loss"])


def test_native_switch():
    assert loss_functions._KLOSS_NATIVE is True
    loss_functions.set_kspace_loss_native(False)
    try:
        assert loss_functions._KLOSS_NATIVE is False
    finally:
        loss_functions.set_kspace_loss_native(True)


def test_kspace_loss_fake_kernels():
    with FakeTensorMode():
        pred = torch.empty(4, 16384, 2, device="cuda")
        k0 = torch.empty(4, 2, 128, 128, device="cuda")
        g = torch.empty((), device="cuda")
        for kind in range(_native.KLOSS_KINDS):
            for planes in (None, k0):
                loss = torch.ops.siren_mri_amd.kspace_loss(pred, planes, planes, pred, kind, 0.25)
                assert loss.shape == () and loss.device.type == "cuda" and loss.dtype == torch.float32
                d = torch.ops.siren_mri_amd.kspace_loss_bwd(pred, planes, planes, pred, g, kind, 0.25)
                assert d.shape == pred.shape and d.dtype == torch.float32 and d.device.type == "cuda"


def _call(lib, which, kind, channels, k0=None, mask=None, ws_bytes=None, desc=True):
    """One of the two C entry points with fake (non-null, never dereferenced) device pointers: the
    argument checks run before anything touches a device."""
    d = ctypes.byref(_native.SirenKlossDesc(1.0, 1e-3, 400.0, 6.7, 1e-4, 1e-4)) if desc else None
    if which == "forward":
        need = int(lib.siren_sse_workspace_bytes())
        return lib.siren_kspace_loss_forward(kind, d, 256, k0, mask, 256, 2, 64, channels, 0.0, 256, 256,
                                             need if ws_bytes is None else ws_bytes, None)
    return lib.siren_kspace_loss_backward(kind, d, 256, k0, mask, 256, 2, 64, channels, 0.0, 256, 256, None)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_entry_points_reject_bad_arguments(which):
    lib = _native.load_library()
    for kw, msg in [(dict(kind=-1, channels=2), "kind"),
                    (dict(kind=_native.KLOSS_KINDS, channels=2), "kind"),
                    (dict(kind=_native.KLOSS_L1, channels=0), "channels"),
                    (dict(kind=_native.KLOSS_ASINH, channels=9), "channels"),
                    (dict(kind=_native.KLOSS_PERP, channels=3), "channels == 2"),
                    (dict(kind=_native.KLOSS_LOG, channels=1), "channels == 2"),
                    (dict(kind=_native.KLOSS_SMAPE, channels=2, k0=256), "k0 and mask"),
                    (dict(kind=_native.KLOSS_CUBIC, channels=2, mask=256), "k0 and mask"),
                    (dict(kind=_native.KLOSS_L1, channels=2, desc=False), "descriptor")]:
        assert _call(lib, which, **kw) == -1, kw
        err = _native.last_error()
        assert msg in err and f"kspace_loss_{which}" in err, (kw, err)


def test_forward_rejects_small_workspace():
    lib = _native.load_library()
    assert _call(lib, "forward", _native.KLOSS_L1, 2, ws_bytes=int(lib.siren_sse_workspace_bytes()) - 1) == -3  # ENOSPACE
    assert "workspace" in _native.last_error()


def test_new_symbols_exported():
    lib = _native.load_library()
    for name in ("siren_kspace_loss_forward", "siren_kspace_loss_backward"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "siren_mri_amd.h")).read()
    for i, kind in enumerate(("ASINH", "CUBIC", "SMAPE", "L1", "PERP", "LOG")):
        assert f"SIREN_KLOSS_{kind} = {i}" in header and getattr(_native, f"KLOSS_{kind}") == i


def test_script_loss_helper():
    sys.path.insert(0, os.path.join(ROOT, "experiment_scripts"))
    try:
        import _common
    finally:
        sys.path.remove(os.path.join(ROOT, "experiment_scripts"))
    want = {"mse": "image_hypernetwork_loss", "asinh": "image_hypernetwork_asinh_loss",
            "perp": "image_hypernetwork_perp_loss", "l1": "image_hypernetwork_l1_loss",
            "log": "image_hypernetwork_log_loss", "cubic": "image_hypernetwork_cubic_loss",
            "ift": "image_hypernetwork_ift_loss"}
    for name, fn in want.items():
        assert _common.hypernetwork_loss(name) is getattr(loss_functions, fn)
    p = _common.base_parser()
    _common.add_loss_argument(p)
    assert p.parse_args(["--experiment_name", "x"]).loss == "mse"
    assert p.parse_args(["--experiment_name", "x", "--loss", "cubic"]).loss == "cubic"
    with pytest.raises(ValueError):
        _common.hypernetwork_loss("nope")
