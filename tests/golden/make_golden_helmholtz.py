"""Golden vectors of Helmholtz fitting from the REAL reference (run in the build container only, on the
CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_helmholtz.py

  helmholtz.npz
    SingleHelmholtzSource ("hs/"): hs/V/coords, hs/V/src, hs/V/slow [2304, 2], hs/V/slow_grid [2304, 1] float32:
    one item of the reference's SingleHelmholtzSource(sidelength=48, velocity=V), V in ("uniform", "square",
    "circle"); hs/wavenumber; hs/field48 [2304, 2] and hs/field230 [52900, 2], the closed-form field
    (scipy.special.hankel2) of SingleHelmholtzSource(48) and (230).

    end to end ("e2e/"): SingleBVPNet(out_features=2, type='sine', in_features=2, hidden_features=64,
    num_hidden_layers=2) under torch.manual_seed(0), on the batch hs/uniform with a batch dimension of 1.
      e2e/init/*
      e2e/terms32 [3], e2e/grad32/*   the reference's helmholtz_pml dict in float32, in its order, and
                         d(sum of the dict)/d(parameter)
      e2e/terms64 [3], e2e/grad64/*   the float64 truth. The reference's jacobian fills a float32
                         torch.zeros, so the reference in .double() does not give float64 derivatives: these
                         come from tests/_helmholtz.formula64 on the reference model cast to double, with the
                         first and second derivatives by autograd
      e2e/terms_ref32_rel [3], e2e/grad_ref32_normrel/*   the reference's float32 against that float64
      e2e/min_margin     the smallest |e_c - src_c| over all elements, in float64 (how far the batch is from
                         the loss's kinks)
      e2e/traj [3, 3]    the three terms at the 3 steps of the reference's training.train (Adam, lr 2e-5, no
                         clipping) on this batch

    op-level ("op/"): tests/_helmholtz.operands(2, 257, seed=50), R = 514: op/x, op/pred, op/jac, op/hess,
    op/src, op/slow, op/k, with the planted flat rows op/row_NAME and slow in {(1, 0), (0.25, 0)}.
      op/terms64 [3], op/dpred64, op/djac64, op/dhess64   tests/_helmholtz.formula64_grads under the
                         upstream weights (1, 2, 3)
      op/terms_ref32_rel [3], op/dpred_ref32_normrel, op/djac_ref32_normrel, op/dhess_ref32_normrel
                         the reference's helmholtz_pml, unchanged, in float32 against that float64, on the
                         field y_c(x) = pred_c + jac_c . d + d^T hess_c d / 2 with d = x - x.detach(): its value,
                         Jacobian and Hessian at every row are op/pred, op/jac and op/hess, and the reference's
                         own jacobian differentiates through the layer's coefficients by autograd (so this
                         also holds formula64's product rule to the reference)
Only data leaves the reference: no source is copied.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _helmholtz as _h  # noqa: E402
from make_golden import OUT, import_reference, quiet, run_train, state_arrays  # noqa: E402

KEYS = _h.KEYS


def norm_rel(a, b):
    den = torch.linalg.vector_norm(b.double()).item()
    return torch.linalg.vector_norm(a.double() - b.double()).item() / (den if den > 0 else 1.0)


def rel(a, b):
    return np.array([abs(x - y) / abs(y) if y != 0 else abs(x) for x, y in zip(a.double().tolist(), b.tolist())])


def stack(losses):
    return torch.stack([losses[k].detach().reshape(()) for k in KEYS])


def source(R, out):
    for v in _h.VELOCITIES:
        ds = R.dataio.SingleHelmholtzSource(sidelength=48, velocity=v)
        inp, gt = ds[0]
        p = f"hs/{v}/"
        out[p + "coords"] = inp["coords"].numpy().copy()
        out[p + "src"] = gt["source_boundary_values"].numpy().copy()
        out[p + "slow"] = gt["squared_slowness"].numpy().copy()
        out[p + "slow_grid"] = gt["squared_slowness_grid"].numpy().copy()
        x, s = inp["coords"], gt["source_boundary_values"]
        on = (s != 0).any(dim=1)
        west, east, south, north = x[:, 0] < -0.5, x[:, 0] > 0.5, x[:, 1] < -0.5, x[:, 1] > 0.5
        pml, corner = west | east | south | north, (west | east) & (south | north)
        print(f"{p}: on rows {int(on.sum())}, PML rows {int(pml.sum())}, corner rows {int(corner.sum())} of {x.shape[0]}; "
              f"slowness values {sorted(set(gt['squared_slowness'][:, 0].tolist()))}")
        assert (s != 0).any() and (s == 0).any() and all(m.any() for m in (west, east, south, north))
        if v == "uniform":
            out["hs/wavenumber"] = np.array(gt["wavenumber"], dtype=np.float64)
            out["hs/field48"] = gt["gt"].numpy().copy()
    out["hs/field230"] = R.dataio.SingleHelmholtzSource(sidelength=230).field.numpy().copy()


def run_model32(R, model, coords, gt):
    model.zero_grad()
    losses = R.loss_functions.helmholtz_pml(model({"coords": coords}), gt)
    assert tuple(losses) == KEYS
    sum(losses.values()).backward()
    return stack(losses), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def derivatives64(model64, coords):
    """(x, y [B, N, 2], jac [B, N, 2, 2], hess [B, N, 2, 2, 2]) of the float64 model by autograd, differentiable."""
    o = model64({"coords": coords.double()})
    x, y = o["model_in"], o["model_out"]
    jac = torch.stack([torch.autograd.grad(y[..., c].sum(), x, create_graph=True)[0] for c in range(2)], dim=-2)
    hess = torch.stack([torch.stack([torch.autograd.grad(jac[..., c, j].sum(), x, create_graph=True)[0]
                                     for j in range(2)], dim=-2) for c in range(2)], dim=-3)
    return x, y, jac, hess


def run_model64(model, coords, gt):
    m = copy.deepcopy(model).double()
    x, y, jac, hess = derivatives64(m, coords)
    src, slow, k = gt["source_boundary_values"], gt["squared_slowness"], gt["wavenumber"]
    terms = _h.formula64(x.detach(), y, jac, hess, src, slow, k)
    terms.sum().backward()
    e = torch.view_as_real(_h.residual64(x.detach(), y.detach(), jac.detach(), hess.detach(), slow, k))
    margin = (e - src.double()).abs().min().item()
    return terms.detach(), {k_: p.grad.detach().clone() for k_, p in m.named_parameters()}, margin


def e2e(R, out):
    coords = torch.from_numpy(out["hs/uniform/coords"])[None]
    gt = {"source_boundary_values": torch.from_numpy(out["hs/uniform/src"])[None],
          "squared_slowness": torch.from_numpy(out["hs/uniform/slow"])[None],
          "wavenumber": torch.tensor([float(out["hs/wavenumber"])], dtype=torch.float64)}
    torch.manual_seed(0)
    model = quiet(R.modules.SingleBVPNet, out_features=2, type="sine", in_features=2, hidden_features=64,
                  num_hidden_layers=2)
    out.update(state_arrays(model, "e2e/init/"))
    t32, g32 = run_model32(R, model, coords, gt)
    t64, g64, margin = run_model64(model, coords, gt)
    assert all(torch.isfinite(g).all() for g in g32.values())
    out.update({"e2e/terms32": t32.numpy(), "e2e/terms64": t64.numpy(), "e2e/terms_ref32_rel": rel(t32, t64),
                "e2e/min_margin": np.array(margin)})
    for k in g32:
        out[f"e2e/grad32/{k}"] = g32[k].numpy()
        out[f"e2e/grad64/{k}"] = g64[k].numpy()
        out[f"e2e/grad_ref32_normrel/{k}"] = np.array(norm_rel(g32[k], g64[k]))
    traj = []

    def loss_fn(model_output, gt_):
        losses = R.loss_functions.helmholtz_pml(model_output, gt_)
        traj.append([float(losses[k]) for k in KEYS])
        return losses

    run_train(R, copy.deepcopy(model), coords, gt, loss_fn, steps=3, lr=2e-5, clip=False)
    out["e2e/traj"] = np.array(traj, dtype=np.float64)
    assert out["e2e/traj"].shape == (3, 3) and np.allclose(traj[0], t32.numpy(), rtol=1e-6)
    print("e2e terms32", t32.tolist(), "terms64", t64.tolist(), "ref32 rel", out["e2e/terms_ref32_rel"].tolist())
    print("e2e min margin |e_c - src_c|", margin)
    print("e2e grad ref32 norm-rel", {k: float(out[f"e2e/grad_ref32_normrel/{k}"]) for k in g32})
    print("e2e trajectory", out["e2e/traj"].tolist())


def op_set(R, out):
    ops = _h.operands(2, 257, seed=50)
    x, pred, jac, hess, src, slow, k = ops
    t64, dp64, dj64, dh64 = _h.formula64_grads(*ops, _h.C)
    # the reference, unchanged, in float32 on a field whose value and derivatives at each row are the operands
    p, j, h = (t.clone().requires_grad_(True) for t in (pred, jac, hess))
    xl = x.clone().requires_grad_(True)
    d = xl - xl.detach()
    y = p + (j * d[..., None, :]).sum(-1) + 0.5 * (d[..., None, :, None] * h * d[..., None, None, :]).sum((-1, -2))
    losses = R.loss_functions.helmholtz_pml({"model_in": xl, "model_out": y},
                                            {"source_boundary_values": src, "squared_slowness": slow,
                                             "wavenumber": k.double()})
    t32 = torch.stack([losses[key].reshape(()) for key in KEYS])
    (t32 * torch.tensor(_h.C)).sum().backward()
    planted = _h.planted_rows(514)
    assert len(planted) == len(_h.PLANTED)
    rz, ri = planted["zero"], planted["interior"]
    for grads in ((dp64, dj64, dh64), (p.grad, j.grad, h.grad)):
        assert all((gr.reshape(514, -1)[rz] == 0).all() for gr in grads)
        assert (grads[1].reshape(514, -1)[ri] == 0).all()
    assert set(slow[..., 0].reshape(-1).tolist()) == {1.0, 0.25} and (slow[..., 1] == 0).all()
    assert (src != 0).any() and (src == 0).any()
    for name, t in zip(_h.OPERANDS, ops):
        out["op/" + name] = t.numpy()
    for name, r in planted.items():
        out["op/row_" + name] = np.array(r)
    out.update({"op/terms64": t64.numpy(), "op/dpred64": dp64.numpy(), "op/djac64": dj64.numpy(),
                "op/dhess64": dh64.numpy(), "op/terms_ref32_rel": rel(t32.detach(), t64),
                "op/dpred_ref32_normrel": np.array(norm_rel(p.grad, dp64)),
                "op/djac_ref32_normrel": np.array(norm_rel(j.grad, dj64)),
                "op/dhess_ref32_normrel": np.array(norm_rel(h.grad, dh64))})
    print("op terms64", t64.tolist(), "ref32 rel", out["op/terms_ref32_rel"].tolist(), "dpred",
          float(out["op/dpred_ref32_normrel"]), "djac", float(out["op/djac_ref32_normrel"]), "dhess",
          float(out["op/dhess_ref32_normrel"]))


def main():
    R = import_reference()
    torch.set_num_threads(8)
    out = {}
    source(R, out)
    e2e(R, out)
    op_set(R, out)
    path = os.path.join(OUT, "helmholtz.npz")
    np.savez_compressed(path, **out)
    print("wrote helmholtz.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
