"""GPU: the analytic SIREN Hessian (SIREN_JVP_HESSIAN tangent-stream kernels: one second-order
stream per pair j <= k) and its adjoint vs the oracle's nested autograd in float64.

  hessian            == diff_operators.hessian (diff_operators.py:5-24)
  backward of a loss on it == the reference's triple backward
  image_mse_FH_prior == loss_functions.py:255-272 restated on the oracle

Tolerances are those test_gpu_jvp.py applies to the Laplacian (the trace of the Hessian: the same
arithmetic): values 4 * max(tv, 1e-5) = 4e-5 (fp32) / 0.2 (bf16) norm-relative, parameter and input
gradients 1e-4 (fp32) / 8e-2 (bf16). The float64 recipe run in fp32 on the CPU is within 1.8e-6
(values) and 2.6e-6 (dW, FH prior) of itself on these shapes, and the smallest per-point Frobenius
norm is 1.1, so the FH prior's norm stays away from its non-differentiable point.

Shapes (rows, hidden, hidden layers, out, C): 10^2 rows (no multiple of any row tile), two output
channels, width 256 with 3 hidden layers (the shape the fp32 fast-path conditions test for), and
C = 3 on the 6^3 grid.
"""
import pytest
import torch

from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TOL = {"fp32": (1e-5, 1e-4), "bf16": (5e-2, 8e-2)}  # test_gpu_jvp.TOL


def _tol(precision):
    tv, tg = TOL[precision]
    return 4 * max(tv, 1e-5), tg


# name -> (coordinates [N, C], hidden, hidden layers, out)
SHAPES = {
    "10x10_h64": (lambda: orc.get_mgrid(10), 64, 1, 1),
    "20x20_h128_o2": (lambda: orc.get_mgrid(20), 128, 1, 2),
    "16x16_h256x3": (lambda: orc.get_mgrid(16), 256, 3, 1),
    "6x6x6_h64_c3": (lambda: orc.get_mgrid(6, dim=3), 64, 2, 1),
}


def _model(hidden, nh, seed, precision, out=1, inp=2):
    from siren_mri_amd import modules
    torch.manual_seed(seed)
    return modules.SingleBVPNet(out_features=out, in_features=inp, type="sine", hidden_features=hidden,
                                num_hidden_layers=nh, precision=precision).to(DEV)


def _oracle_params(sd, n_layers, bi=None):
    def pick(k):
        t = sd[k] if bi is None else sd[k][bi]
        return t.detach().double().cpu().clone().requires_grad_(True)
    return [(pick(f"net.net.{i}.0.weight"), pick(f"net.net.{i}.0.bias")) for i in range(n_layers)]


def _oracle_hessian(y, x):
    """diff_operators.hessian's recipe (nested autograd), differentiable: [B, N, O, C, C]."""
    rows = []
    for i in range(y.shape[-1]):
        dydx = torch.autograd.grad(y[..., i].sum(), x, create_graph=True)[0]
        rows.append(torch.stack([torch.autograd.grad(dydx[..., j].sum(), x, create_graph=True)[0]
                                 for j in range(x.shape[-1])], dim=-2))
    return torch.stack(rows, dim=-3)


_REF = {}


def _reference(name, seed):
    """The float64 Hessian of the shape's seeded model, computed once and left unchanged."""
    if name not in _REF:
        mk, hidden, nh, out = SHAPES[name]
        coords = mk()[None]
        m = _model(hidden, nh, seed, "fp32", out=out, inp=coords.shape[-1])
        ps = _oracle_params(m.state_dict(), nh + 2)
        x = coords.double().clone().requires_grad_(True)
        _REF[name] = _oracle_hessian(orc.siren_forward(x, ps), x).detach()
    return _REF[name]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hessian_forward(precision, name):
    from siren_mri_amd import diff_operators, jvp
    mk, hidden, nh, out = SHAPES[name]
    coords = mk()[None]
    N, C = coords.shape[1:]
    m = _model(hidden, nh, 17, precision, out=out, inp=C)
    ref = _reference(name, 17)
    tv, _ = _tol(precision)
    o = m({"coords": coords.to(DEV)})
    if precision == "fp32":  # the forward's saved phases are the primal stream
        assert getattr(o["model_out"], "_siren_primal", None) is not None
    h, status = diff_operators.hessian(o["model_out"], o["model_in"])
    h0 = jvp.siren_hessian(o["model_in"], m.net, primal=None)
    lap = diff_operators.laplace(o["model_out"], o["model_in"])
    h, h0, lap = h.detach(), h0.detach(), lap.detach()
    for t in (h, h0):
        assert t.shape == (1, N, out, C, C)
        err = orc.norm_rel(t.cpu(), ref)
        print(f"{precision} {name}: hessian norm-rel {err:.3e} (tolerance {tv:.1e})")
        assert err < tv
        assert torch.equal(t, t.transpose(-1, -2))
    assert status == 0
    trace = h.diagonal(dim1=-2, dim2=-1).sum(-1).sum(-1, keepdim=True)
    err = orc.norm_rel(trace.cpu(), lap.cpu())
    print(f"{precision} {name}: trace vs native laplace {err:.3e}")
    assert err < tv


def _check_param_grads(got_w, got_b, ps, tg, what):
    for i, (W, b) in enumerate(ps):
        err = orc.norm_rel(got_w[i].cpu(), W.grad)
        print(f"{what} layer {i} dW {err:.3e}")
        assert err < tg, f"{what} layer {i} dW"
        if b.grad is None:  # output bias: no path to the Hessian
            assert got_b[i] is None, f"{what} output bias"
        else:
            err = orc.norm_rel(got_b[i].cpu(), b.grad)
            print(f"{what} layer {i} db {err:.3e}")
            assert err < tg, f"{what} layer {i} db"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_hessian_backward_shared_weights(precision, name):
    """A seeded, non-symmetric cotangent on the Hessian: dW, db, dx vs the oracle's triple backward."""
    from siren_mri_amd import diff_operators
    mk, hidden, nh, out = SHAPES[name]
    coords = mk()[None]
    N, C = coords.shape[1:]
    m = _model(hidden, nh, 19, precision, out=out, inp=C)
    G = torch.randn(1, N, out, C, C, generator=torch.Generator().manual_seed(4))
    o = m({"coords": coords.to(DEV)})
    xin = o["model_in"]
    h, _ = diff_operators.hessian(o["model_out"], xin)
    (h * G.to(DEV)).sum().backward()
    ps = _oracle_params(m.state_dict(), nh + 2)
    x = coords.double().clone().requires_grad_(True)
    (_oracle_hessian(orc.siren_forward(x, ps), x) * G.double()).sum().backward()
    _, tg = _tol(precision)
    layers = [m.net.net[i][0] for i in range(nh + 2)]
    _check_param_grads([lw.weight.grad for lw in layers], [lw.bias.grad for lw in layers], ps, tg, name)
    err = orc.norm_rel(xin.grad.cpu(), x.grad)
    print(f"{name} dx {err:.3e}")
    assert err < tg


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hessian_backward_batched_weights(precision):
    """Per-sample (hypernetwork) weights, B = 2, as test_laplace_backward_input_grad_and_batched_weights."""
    from siren_mri_amd import diff_operators
    m = _model(64, 1, 11, precision)
    B = 2
    params = {k: torch.stack([v * (1 + 0.03 * i) for i in range(B)]).requires_grad_(True)
              for k, v in m.state_dict().items()}
    coords = orc.get_mgrid(10)[None].repeat(B, 1, 1)
    G = torch.randn(B, 100, 1, 2, 2, generator=torch.Generator().manual_seed(4))
    o = m({"coords": coords.to(DEV)}, params=params)
    xin = o["model_in"]
    h, _ = diff_operators.hessian(o["model_out"], xin)
    assert h.shape == G.shape
    (h * G.to(DEV)).sum().backward()
    _, tg = _tol(precision)
    assert params["net.net.2.0.bias"].grad is None
    for bi in range(B):
        ps = _oracle_params(params, 3, bi)
        x = coords[bi:bi + 1].double().clone().requires_grad_(True)
        (_oracle_hessian(orc.siren_forward(x, ps), x) * G[bi:bi + 1].double()).sum().backward()
        _check_param_grads([params[f"net.net.{i}.0.weight"].grad[bi] for i in range(3)],
                           [params[f"net.net.{i}.0.bias"].grad[bi] if i < 2 else None for i in range(3)],
                           ps, tg, f"sample {bi}")
        assert orc.norm_rel(xin.grad[bi:bi + 1].cpu(), x.grad) < tg, f"sample {bi} dx"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fh_prior_forward_and_backward(precision):
    """image_mse_FH_prior (mask [N, 1], k1 = 0.5, 16^2, a 2 x 64 net): one forward and backward
    against the loss restated on the oracle in float64 with the same random coordinates. Before
    the Hessian had its adjoint, .backward() raised the third-derivative RuntimeError."""
    from siren_mri_amd import loss_functions
    side, k1 = 16, 0.5
    m = _model(64, 2, 23, precision)
    gen = torch.Generator().manual_seed(9)
    coords = orc.get_mgrid(side)[None]
    gt = torch.randn(1, side * side, 1, generator=gen)
    mask = (torch.rand(side * side, 1, generator=gen) < 0.5).float()
    o = m({"coords": coords.to(DEV)})
    torch.manual_seed(31)
    losses = loss_functions.image_mse_FH_prior(mask.to(DEV), k1, m, o, {"img": gt.to(DEV)})
    sum(losses.values()).backward()

    ps = _oracle_params(m.state_dict(), 4)
    torch.manual_seed(31)
    xr = (2 * (torch.rand((1, side * side // 2, 2)) - 0.5)).double().requires_grad_(True)
    x = coords.double().clone().requires_grad_(True)
    y = orc.siren_forward(x, ps)
    hr = _oracle_hessian(orc.siren_forward(xr, ps), xr)
    ref = {"img_loss": (mask.double() * (y - gt.double()) ** 2).mean(),
           "prior_loss": k1 * hr.reshape(1, side * side // 2, -1).norm(dim=-1, keepdim=True).abs().mean()}
    sum(ref.values()).backward()
    tv, tg = _tol(precision)
    assert sorted(losses) == sorted(ref)
    for k in ref:
        print(f"{precision} {k}: {losses[k].item():.8g} vs {ref[k].item():.8g}")
        assert losses[k].item() == pytest.approx(ref[k].item(), rel=tv), k
    layers = [m.net.net[i][0] for i in range(4)]
    _check_param_grads([lw.weight.grad for lw in layers], [lw.bias.grad for lw in layers], ps, tg, "FH prior")


def test_hessian_backward_is_not_differentiable_again():
    from siren_mri_amd import diff_operators
    m = _model(32, 1, 2, "fp32")
    o = m({"coords": orc.get_mgrid(8)[None].to(DEV)})
    h, _ = diff_operators.hessian(o["model_out"], o["model_in"])
    gw = torch.autograd.grad(h.square().sum(), list(m.parameters())[:2], create_graph=True)
    with pytest.raises(RuntimeError, match="not provided"):
        gw[0].sum().backward()


def test_four_inputs_raise_natively_and_fall_back_in_diff_operators():
    from siren_mri_amd import diff_operators, jvp
    m = _model(32, 1, 3, "fp32", inp=4)
    coords = (torch.rand(1, 50, 4, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    o = m({"coords": coords.to(DEV)})
    with pytest.raises(RuntimeError, match="in_features <= 3"):
        jvp.siren_hessian(o["model_in"], m.net)
    h, status = diff_operators.hessian(o["model_out"], o["model_in"])
    ps = _oracle_params(m.state_dict(), 3)
    x = coords.double().clone().requires_grad_(True)
    ref = _oracle_hessian(orc.siren_forward(x, ps), x)
    assert status == 0 and h.shape == (1, 50, 1, 4, 4)
    assert orc.norm_rel(h.detach().cpu(), ref.detach()) < _tol("fp32")[0]


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("prec", [0, 1])
def test_fake_kernel_hessian_shape(batched, prec):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import siren_mri_amd.jvp  # noqa: F401 - registers the tangent-stream ops
    dims = [3, 64, 64, 2]
    B, N = 3, 777
    with FakeTensorMode():
        x = torch.empty(B if batched else 1, N, dims[0], device="cuda")
        ws = [torch.empty(*((B,) if batched else ()), dims[l + 1], dims[l], device="cuda") for l in range(3)]
        bs = [torch.empty(*((B,) if batched else ()), dims[l + 1], device="cuda") for l in range(3)]
        h, saved = torch.ops.siren_mri_amd.sine_mlp_jvp(x, ws, bs, 30.0, prec, batched, 4, True)
        jac, s3 = torch.ops.siren_mri_amd.sine_mlp_jvp(x, ws, bs, 30.0, prec, batched, 3, True)
        assert h.shape == x.shape[:-1] + (2, 3, 3) and h.dtype == torch.float32 and h.device.type == "cuda"
        assert jac.shape == x.shape[:-1] + (2, 3)
        assert saved.dtype == torch.uint8 and saved.numel() > s3.numel() > 0
