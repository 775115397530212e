"""CPU: the native batched 2-D FFT and the image-domain (IFT) k-space loss (siren_kfft.hip) as far as
they go without a device — the three ops' registration and fake kernels, the argument checks of the
three C entry points, and ift_image_mse's routing (CPU tensors keep the expression path; the switch
set_kspace_loss_native is honoured)."""
import ctypes

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from siren_mri_amd import _native, loss_functions

SCHEMAS = {
    "kspace_fft2": "siren_mri_amd::kspace_fft2(Tensor x, bool inverse) -> Tensor",
    "kspace_ift_loss": "siren_mri_amd::kspace_ift_loss(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, "
                       "Tensor? img_mask, float noise, float img_weight, float l1_weight, float kspace_weight) -> Tensor",
    "kspace_ift_loss_bwd": "siren_mri_amd::kspace_ift_loss_bwd(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, "
                           "Tensor? img_mask, Tensor g, float noise, float img_weight, float l1_weight, "
                           "float kspace_weight) -> Tensor",
}
SYMBOLS = ("siren_kspace_fft2", "siren_kspace_ift_loss_forward", "siren_kspace_ift_loss_backward")


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_ops_registered(name):
    op = getattr(torch.ops.siren_mri_amd, name).default
    assert str(op._schema) == SCHEMAS[name]


def test_symbols_exported():
    lib = _native.load_library()
    for name in SYMBOLS:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_native.SirenKiftDesc) == 12
    assert _native.KFFT_SIDES == (8, 16, 32, 64, 128)


def test_fake_kernels():
    ops = torch.ops.siren_mri_amd
    with FakeTensorMode():
        b, side = 4, 128
        pred = torch.empty(b, side * side, 2, device="cuda")
        planes = torch.empty(b, 2, side, side, device="cuda")
        g = torch.empty((), device="cuda")
        for inverse in (False, True):
            out = ops.kspace_fft2(pred, inverse)
            assert out.shape == (b, side * side, 2) and out.dtype == torch.float32 and out.device.type == "cuda"
        for pl in (None, planes):
            for m in (None, torch.empty(side, side, device="cuda"), torch.empty(b, side, side, device="cuda")):
                loss = ops.kspace_ift_loss(pred, pl, pl, pred, m, 0.25, 1.0, 1e-8, 0.0025)
                assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == "cuda"
                d = ops.kspace_ift_loss_bwd(pred, pl, pl, pred, m, g, 0.25, 1.0, 1e-8, 0.0025)
                assert d.shape == pred.shape and d.dtype == torch.float32 and d.device.type == "cuda"


def _call(lib, which, side=16, batch=2, pred=256, k0=None, mask=None, tgt=256, ws_bytes=None, desc=True, out=256):
    """One of the C entry points with fake (non-null, never dereferenced) device pointers: the argument
    checks run before anything touches a device."""
    if which == "fft2":
        return lib.siren_kspace_fft2(pred, out, batch, side, 1, None)
    d = ctypes.byref(_native.SirenKiftDesc(1.0, 1e-8, 0.0025)) if desc else None
    if which == "ift_loss_forward":
        need = int(lib.siren_sse_workspace_bytes())
        return lib.siren_kspace_ift_loss_forward(d, pred, k0, mask, tgt, None, 0, batch, side, 0.0, out, 256,
                                                 need if ws_bytes is None else ws_bytes, None)
    return lib.siren_kspace_ift_loss_backward(d, pred, k0, mask, tgt, None, 0, batch, side, 0.0, 256, out, None)


def _slots(lib):
    return (int(lib.siren_sse_workspace_bytes()) - 256) // 4


@pytest.mark.parametrize("which", ["fft2", "ift_loss_forward", "ift_loss_backward"])
def test_entry_points_reject_bad_arguments(which):
    lib = _native.load_library()
    cases = [(dict(side=12), "side"), (dict(side=4), "side"), (dict(side=256), "side"),
             (dict(pred=None), "null pointer"), (dict(out=None), "null pointer")]
    if which != "fft2":
        cases += [(dict(tgt=None), "null pointer"), (dict(desc=False), "descriptor"),
                  (dict(k0=256), "k0 and mask"), (dict(mask=256), "k0 and mask"),
                  (dict(batch=_slots(lib) + 1), "batch"), (dict(batch=0), "batch")]
    for kw, msg in cases:
        assert _call(lib, which, **kw) == -1, kw
        err = _native.last_error()
        assert msg in err and f"kspace_{which}" in err, (kw, err)


def test_forward_rejects_short_workspace():
    lib = _native.load_library()
    assert _call(lib, "ift_loss_forward", ws_bytes=int(lib.siren_sse_workspace_bytes()) - 1) == -3  # ENOSPACE
    err = _native.last_error()
    assert "workspace" in err and "kspace_ift_loss_forward" in err
    assert loss_functions._kift_max_batch() == _slots(lib) == 1024


def _formula64(pred, tgt, m=None):
    side = int(round(pred.shape[1] ** 0.5))
    cp = torch.complex(pred[..., 0], pred[..., 1]).view(-1, side, side)
    ct = torch.complex(tgt[..., 0], tgt[..., 1]).view(-1, side, side)
    img = (torch.fft.ifft2(cp).abs() - torch.fft.ifft2(ct).abs()) ** 2
    if m is not None:
        img = m * img
    return img.sum() + 1e-8 * cp.abs().sum() + 0.0025 * ((pred - tgt) ** 2).sum()


@pytest.mark.parametrize("side", [8, 12])
def test_cpu_routing_unchanged(side):
    """CPU tensors (a supported side and another) keep the expression path: the fp64 formula to 1e-12."""
    g = torch.Generator().manual_seed(side)
    pred = torch.randn(2, side * side, 2, generator=g, dtype=torch.float64)
    tgt = torch.randn(2, side * side, 2, generator=g, dtype=torch.float64)
    for m in (None, (torch.rand(side, side, generator=g) < 0.5).double()):
        p = pred.clone().requires_grad_(True)
        assert not loss_functions._ift_native_applies(m, p, tgt)
        got = loss_functions.ift_image_mse(m, {"model_out": p}, {"img": tgt})["img_loss"]
        assert "KspaceIftLoss" not in type(got.grad_fn).__name__
        want = _formula64(pred, tgt, m)
        assert abs(float(got.detach()) - float(want)) <= 1e-12 * abs(float(want))
        wrapped = loss_functions.image_hypernetwork_ift_loss(
            m, 1.0, 1.0, {"model_out": p, "latent_vec": torch.zeros(2, 4), "hypo_params": {"w": torch.zeros(2, 3)}},
            {"img": tgt})["img_loss"]
        assert torch.equal(wrapped, got)
    p32 = pred.float()
    assert not loss_functions._ift_native_applies(None, p32, tgt.float())  # float32, but not on the device


def test_routing_predicate_and_switch():
    """On (fake) device tensors the predicate takes float32 [B, side^2, 2] with a supported side, a target
    without grad and a mask of one of the three shapes; set_kspace_loss_native(False) turns it off."""
    applies = loss_functions._ift_native_applies
    with FakeTensorMode():
        out = torch.empty(3, 256, 2, device="cuda")
        tgt = torch.empty(3, 256, 2, device="cuda")
        assert applies(None, out, tgt)
        for shape in ((16, 16), (1, 16, 16), (3, 16, 16)):
            assert applies(torch.empty(shape, device="cuda"), out, tgt), shape
        assert not applies(torch.empty(2, 16, 16, device="cuda"), out, tgt)
        assert not applies(torch.empty(16, 16, device="cuda", dtype=torch.float64), out, tgt)
        assert not applies(torch.empty(16, 16), out, tgt)  # a mask on the CPU
        assert not applies(torch.empty(16, 16, device="cuda", requires_grad=True), out, tgt)
        assert not applies(None, out, torch.empty(3, 256, 2, device="cuda", requires_grad=True))
        assert not applies(None, out.double(), tgt.double())
        assert not applies(None, torch.empty(3, 256, 3, device="cuda"), torch.empty(3, 256, 3, device="cuda"))
        for n in (144, 16, 256 * 256):  # side 12, 4, 256
            assert not applies(None, torch.empty(1, n, 2, device="cuda"), torch.empty(1, n, 2, device="cuda")), n
        big = loss_functions._kift_max_batch() + 1
        assert not applies(None, torch.empty(big, 64, 2, device="cuda"), torch.empty(big, 64, 2, device="cuda"))
        loss_functions.set_kspace_loss_native(False)
        try:
            assert not applies(None, out, tgt)
        finally:
            loss_functions.set_kspace_loss_native(True)
        assert applies(None, out, tgt)


def test_fft2_refuses_a_gradient():
    """kspace_fft2 has no autograd formula: an input that requires grad is an error under grad mode (raised
    by the op's Autograd kernel before anything reaches a device)."""
    x = torch.zeros(1, 64, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        torch.ops.siren_mri_amd.kspace_fft2(x, True)
