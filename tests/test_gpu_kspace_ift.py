"""GPU: the native batched 2-D FFT (siren_mri_amd::kspace_fft2) and the image-domain k-space loss
(siren_mri_amd::kspace_ift_loss / kspace_ift_loss_bwd, siren_kfft.hip) against the same formulas in
float64 (complex128) on the CPU with torch.fft, on inputs built like test_gpu_kspace_losses.py's
planted_inputs (amplitude 0.5 exp(-3 u), planted ties, zero pixels and zero channels).

Bounds: loss relative 1e-5, gradient / transform oracle.norm_rel 1e-6 (what the family's other
members are held to), or 8x the float32-against-float64 error of the same torch formula evaluated in
float32 on the CPU inside the test where that is larger (the reference's own arithmetic; with these
inputs it puts every bound between 1e-6 and about 3.3e-6). Every test prints what it measured; a run on
an MI355X is recorded in profiles/kspace_ift_gpu_errors.txt.
"""
import functools

import pytest
import torch

from oracle import siren_oracle as orc
from siren_mri_amd import loss_functions
from siren_mri_amd.data_consistency import DataConsistencyInKspace

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOSS_RTOL, NORMREL = 1e-5, 1e-6
SIDES = (8, 16, 32, 64, 128)
REF_WEIGHTS = (1.0, 1e-8, 0.0025)
OPS = torch.ops.siren_mri_amd


def planted_inputs(batch, side, seed):
    """test_gpu_kspace_losses.planted_inputs for two channels: (pred, tgt) [batch, side^2, 2]."""
    g = torch.Generator().manual_seed(seed)
    n, channels = side * side, 2
    amp = 0.5 * torch.exp(-3.0 * torch.rand(batch, n, 1, generator=g))
    pred = amp * torch.randn(batch, n, channels, generator=g)
    tgt = amp * torch.randn(batch, n, channels, generator=g)
    k = max(2, n // 16)
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        tie, p0, t0, both, ch = (perm[i * k:(i + 1) * k] for i in range(5))
        pred[b, tie] = tgt[b, tie]
        pred[b, p0] = 0.0
        tgt[b, t0] = 0.0
        pred[b, both] = 0.0
        tgt[b, both] = 0.0
        pred[b, ch, b % channels] = 0.0
    return pred, tgt


@functools.lru_cache(maxsize=None)
def inputs(batch, side):
    return planted_inputs(batch, side, seed=1000 + 10 * side + batch)


@functools.lru_cache(maxsize=None)
def img_mask(kind, batch, side):
    g = torch.Generator().manual_seed(7 + side)
    if kind == "none":
        return None
    shape = (side, side) if kind == "hw" else (batch, side, side)
    return (torch.rand(shape, generator=g) < 0.6).float()


@functools.lru_cache(maxsize=None)
def dc_planes(batch, side):
    """(k0, mask) [batch, 2, side, side]; the mask has both 0 and 1 entries."""
    g = torch.Generator().manual_seed(33 + side)
    amp = 0.5 * torch.exp(-3.0 * torch.rand(batch, 1, side, side, generator=g))
    k0 = amp * torch.randn(batch, 2, side, side, generator=g)
    mask = (torch.rand(batch, 2, side, side, generator=g) < 0.33).float()
    assert 0 < mask.sum() < mask.numel()
    return k0, mask


def to_complex(x, side):
    return torch.complex(x[..., 0], x[..., 1]).reshape(-1, side, side)


def formula(pred, tgt, m, weights, dc=None, scale=3.0):
    """(loss, d(scale loss)/dpred) of the issue's formula in pred's dtype on the CPU (torch.fft, autograd)."""
    dt = pred.dtype
    side = int(round(pred.shape[1] ** 0.5))
    p = pred.clone().requires_grad_(True)
    y = p
    if dc is not None:
        b = pred.shape[0]
        k = dc[0].to(dt).permute(0, 2, 3, 1).reshape(b, -1, 2)
        mk = dc[1].to(dt).permute(0, 2, 3, 1).reshape(b, -1, 2)
        y = (1 - mk) * p + (mk * k if dc[2] is None else mk * (p + dc[2] * k) / (1 + dc[2]))
    cy, ct = to_complex(y, side), to_complex(tgt, side)
    img = (torch.fft.ifft2(cy).abs() - torch.fft.ifft2(ct).abs()) ** 2
    if m is not None:
        img = m.to(dt) * img
    loss = weights[0] * img.sum() + weights[1] * cy.abs().sum() + weights[2] * ((y - tgt) ** 2).sum()
    (scale * loss).backward()
    return loss.detach(), p.grad


@functools.lru_cache(maxsize=None)
def reference(batch, side, mask_kind, weights, dc_noise="nodc"):
    """The float64 loss and gradient, and the bounds: the floor or 8x the float32 formula's own error."""
    pred, tgt = inputs(batch, side)
    m = img_mask(mask_kind, batch, side)
    dc = None if dc_noise == "nodc" else dc_planes(batch, side) + (dc_noise,)
    if dc is not None:  # tgt == k0 on the sampled elements, as a measured target is
        mk = dc[1].permute(0, 2, 3, 1).reshape(batch, -1, 2)
        tgt = torch.where(mk > 0, dc[0].permute(0, 2, 3, 1).reshape(batch, -1, 2), tgt)
    l64, g64 = formula(pred.double(), tgt.double(), m, weights, dc)
    l32, g32 = formula(pred, tgt, m, weights, dc)
    loss_tol = max(LOSS_RTOL, 8 * abs(float(l32) - float(l64)) / abs(float(l64)))
    grad_tol = max(NORMREL, 8 * orc.norm_rel(g32, g64))
    return pred, tgt, m, dc, l64, g64, loss_tol, grad_tol


def check(tag, loss, grad, ref_loss, ref_grad, loss_tol, grad_tol):
    le = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    ge = orc.norm_rel(grad, ref_grad)
    print(f"\n[kspace ift] {tag}: loss rel err {le:.2e} (bound {loss_tol:.1e}), "
          f"grad norm-rel {ge:.2e} (bound {grad_tol:.1e})")
    assert torch.isfinite(grad).all()
    assert le <= loss_tol
    assert ge < grad_tol


def dev(t):
    return t.to(DEV) if t is not None else None


def run_op(pred, tgt, m, weights, scale=3.0):
    p = pred.to(DEV).requires_grad_(True)
    loss = OPS.kspace_ift_loss(p, None, None, tgt.to(DEV), dev(m), 0.0, *weights)
    (scale * loss).backward()
    return loss.detach().cpu(), p.grad.cpu()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("side", SIDES)
def test_transform_alone(side, batch):
    x, _ = inputs(batch, side)
    c64 = to_complex(x.double(), side)
    xd = x.to(DEV)
    bounds = {}
    for inverse, fn in ((True, torch.fft.ifft2), (False, torch.fft.fft2)):
        ref = torch.view_as_real(fn(c64)).reshape(batch, -1, 2)
        ref32 = torch.view_as_real(fn(to_complex(x, side))).reshape(batch, -1, 2)
        bounds[inverse] = max(NORMREL, 8 * orc.norm_rel(ref32, ref))
        out = OPS.kspace_fft2(xd, inverse)
        assert out.shape == x.shape and out.dtype == torch.float32
        err = orc.norm_rel(out.cpu(), ref)
        print(f"\n[kspace ift] fft2 inverse={inverse} side {side} B={batch}: norm-rel {err:.2e} "
              f"(bound {bounds[inverse]:.1e})")
        assert err < bounds[inverse]
        assert torch.equal(out, OPS.kspace_fft2(xd, inverse))  # the same call twice: the same bits
    back = OPS.kspace_fft2(OPS.kspace_fft2(xd, True), False)
    err = orc.norm_rel(back.cpu(), x)
    print(f"[kspace ift] fft2(ifft2(x)) side {side} B={batch}: norm-rel {err:.2e} (bound {2 * min(bounds.values()):.1e})")
    assert err < 2 * min(bounds.values())


@pytest.mark.parametrize("mask_kind", ["none", "hw", "bhw"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("side", SIDES)
def test_image_term_alone(side, batch, mask_kind):
    """Weights (1, 0, 0): with the reference's weights the image term is about 0.5 % of the loss at
    128 x 128, so a wrong transform would hide inside the total's tolerance."""
    pred, tgt, m, _, l64, g64, lt, gt = reference(batch, side, mask_kind, (1.0, 0.0, 0.0))
    loss, grad = run_op(pred, tgt, m, (1.0, 0.0, 0.0))
    check(f"image term side {side} B={batch} mask {mask_kind}", loss, grad, l64, g64, lt, gt)


@pytest.mark.parametrize("weights", [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
@pytest.mark.parametrize("side", [8, 128])
def test_kspace_terms_alone(side, weights):
    pred, tgt, m, _, l64, g64, lt, gt = reference(2, side, "none", weights)
    loss, grad = run_op(pred, tgt, m, weights)
    check(f"weights {weights} side {side}", loss, grad, l64, g64, lt, gt)
    assert (grad[g64 == 0] == 0.0).all()  # |y| at 0 and y == t: exactly 0, as torch's


@pytest.mark.parametrize("dc_noise", ["nodc", None, 0.25])
@pytest.mark.parametrize("side", [16, 128])
def test_reference_weights_through_loss_functions(side, dc_noise):
    """ift_image_mse and image_hypernetwork_ift_loss, with and without DataConsistencyInKspace in front."""
    batch = 2
    pred, tgt, m, dc, l64, g64, lt, gt = reference(batch, side, "none", REF_WEIGHTS, dc_noise)
    p = pred.to(DEV).requires_grad_(True)
    out = p if dc is None else DataConsistencyInKspace(dc[2])(p, dc[0].to(DEV), dc[1].to(DEV))
    loss = loss_functions.ift_image_mse(None, {"model_out": out}, {"img": tgt.to(DEV)})["img_loss"]
    assert "KspaceIftLoss" in type(loss.grad_fn).__name__, type(loss.grad_fn).__name__
    (3.0 * loss).backward()
    grad = p.grad.cpu()
    check(f"ift_image_mse side {side} dc {dc_noise}", loss.detach().cpu(), grad, l64, g64, lt, gt)
    if dc is not None and dc[2] is None:  # sampled elements: the DC's coefficient is 0
        assert (grad[dc[1].permute(0, 2, 3, 1).reshape(batch, -1, 2) > 0] == 0.0).all()
    model_output = {"model_out": out, "latent_vec": torch.ones(batch, 4, device=DEV),
                    "hypo_params": {"w": torch.ones(batch, 3, device=DEV)}}
    wrapped = loss_functions.image_hypernetwork_ift_loss(None, 1e-3, 1e-3, model_output, {"img": tgt.to(DEV)})
    assert "KspaceIftLoss" in type(wrapped["img_loss"].grad_fn).__name__
    assert torch.equal(wrapped["img_loss"], loss)


def test_masked_loss_through_loss_functions():
    """The optional image mask of ift_image_mse, [H, W], [1, H, W] and [B, H, W], on the native op."""
    batch, side = 3, 16
    for kind in ("hw", "bhw"):
        pred, tgt, m, _, l64, g64, lt, gt = reference(batch, side, kind, REF_WEIGHTS)
        for mm in ((m, m[None]) if kind == "hw" else (m,)):
            p = pred.to(DEV).requires_grad_(True)
            loss = loss_functions.ift_image_mse(mm.to(DEV), {"model_out": p}, {"img": tgt.to(DEV)})["img_loss"]
            assert "KspaceIftLoss" in type(loss.grad_fn).__name__
            (3.0 * loss).backward()
            check(f"ift_image_mse mask {tuple(mm.shape)}", loss.detach().cpu(), p.grad.cpu(), l64, g64, lt, gt)


@pytest.mark.parametrize("side", [8, 128])
def test_exact_cases(side):
    w = (1.0, 0.0, 0.0)
    pred, tgt = (t.clone() for t in inputs(3, side))
    pred, tgt = pred[:2], tgt[:2]
    pred[0] = tgt[0]  # slice 0: pred == tgt bitwise
    loss2, grad2 = run_op(pred, tgt, None, w)
    loss1, grad1 = run_op(pred[1:], tgt[1:], None, w)
    print(f"\n[kspace ift] exact: B=2 loss {float(loss2):.9e}, slice 1 alone {float(loss1):.9e}")
    assert (grad2[0] == 0.0).all()
    assert torch.equal(loss2, loss1) and torch.equal(grad2[1], grad1[0])
    # a slice of zeros: the gradients of |x| and |y| at 0 are 0 (torch's convention), and finite
    pred[0] = 0.0
    _, grad = run_op(pred, tgt, None, (1.0, 1.0, 0.0))
    assert torch.isfinite(grad).all() and (grad[0] == 0.0).all()
    assert (grad[1] != 0.0).any()


def test_fallbacks():
    """Side 12, side 256 and float64 take the expression path; so does everything with the switch off."""
    for side, dt in ((12, torch.float32), (256, torch.float32), (16, torch.float64)):
        pred, tgt = planted_inputs(1, side, seed=side)
        p = pred.to(DEV, dt).requires_grad_(True)
        loss = loss_functions.ift_image_mse(None, {"model_out": p}, {"img": tgt.to(DEV, dt)})["img_loss"]
        assert "KspaceIftLoss" not in type(loss.grad_fn).__name__
        l64, _ = formula(pred.double(), tgt.double(), None, REF_WEIGHTS)
        err = abs(float(loss.detach()) - float(l64)) / abs(float(l64))
        print(f"\n[kspace ift] fallback side {side} {dt}: loss rel err {err:.2e}")
        assert err <= LOSS_RTOL
    pred, tgt, m, _, l64, g64, lt, gt = reference(2, 16, "none", REF_WEIGHTS)
    native_l, native_g = None, None
    for native in (True, False):
        loss_functions.set_kspace_loss_native(native)
        try:
            p = pred.to(DEV).requires_grad_(True)
            loss = loss_functions.ift_image_mse(None, {"model_out": p}, {"img": tgt.to(DEV)})["img_loss"]
            assert ("KspaceIftLoss" in type(loss.grad_fn).__name__) == native
            (3.0 * loss).backward()
        finally:
            loss_functions.set_kspace_loss_native(True)
        check(f"side 16 native={native}", loss.detach().cpu(), p.grad.cpu(), l64, g64, lt, gt)
        if native:
            native_l, native_g = loss.detach().cpu(), p.grad.cpu()
        else:
            check("side 16 native vs expression path", native_l, native_g, loss.detach().cpu(), p.grad.cpu(), lt, gt)


def test_double_backward_raises():
    pred, tgt = inputs(1, 8)
    p = pred.to(DEV).requires_grad_(True)
    loss = loss_functions.ift_image_mse(None, {"model_out": p}, {"img": tgt.to(DEV)})["img_loss"]
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(loss, p, create_graph=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        OPS.kspace_fft2(p, True)


def test_graph_capture_and_replay():
    """kspace_ift_loss then kspace_ift_loss_bwd captured on one stream (no autograd engine) at side 128:
    two replays each equal the eager result bit for bit."""
    pred, tgt = inputs(3, 128)
    p, t, g = pred[:2].to(DEV), tgt[:2].to(DEV), torch.tensor(3.0, device=DEV)
    k0, mask = (x.to(DEV) for x in dc_planes(2, 128))
    args = (p, k0, mask, t, None)
    eager_l = OPS.kspace_ift_loss(*args, 0.25, *REF_WEIGHTS)
    eager_d = OPS.kspace_ift_loss_bwd(*args, g, 0.25, *REF_WEIGHTS)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):  # warm-up on the capture stream: its workspace exists before the capture
        OPS.kspace_ift_loss(*args, 0.25, *REF_WEIGHTS)
        OPS.kspace_ift_loss_bwd(*args, g, 0.25, *REF_WEIGHTS)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cap_l = OPS.kspace_ift_loss(*args, 0.25, *REF_WEIGHTS)
        cap_d = OPS.kspace_ift_loss_bwd(*args, g, 0.25, *REF_WEIGHTS)
    for _ in range(2):
        cap_l.zero_()
        cap_d.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_l, eager_l) and torch.equal(cap_d, eager_d)
    assert float(eager_l) > 0 and (eager_d != 0).any()


def test_opcheck():
    pred, tgt = inputs(3, 8)
    k0, mask = (x.to(DEV) for x in dc_planes(3, 8))
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for planes in ((None, None), (k0, mask)):
        for m in (None, img_mask("hw", 3, 8).to(DEV), img_mask("bhw", 3, 8).to(DEV)):
            p = pred.to(DEV).requires_grad_(True)
            torch.library.opcheck(OPS.kspace_ift_loss.default,
                                  (p, planes[0], planes[1], tgt.to(DEV), m, 0.25) + REF_WEIGHTS, test_utils=utils)
            torch.library.opcheck(OPS.kspace_ift_loss_bwd.default,
                                  (pred.to(DEV), planes[0], planes[1], tgt.to(DEV), m, torch.tensor(3.0, device=DEV),
                                   0.25) + REF_WEIGHTS, test_utils=utils)
    torch.library.opcheck(OPS.kspace_fft2.default, (pred.to(DEV), True), test_utils=("test_schema", "test_faketensor"))
