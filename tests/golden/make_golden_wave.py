"""Golden vectors of wave-equation fitting from the REAL reference (run in the build container only, on
the CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wave.py

  wave.npz
    WaveSource ("ws/"): ws/M/I/coords [2304, 3], ws/M/I/src, ws/M/I/slow [2304, 1] float32, ws/M/I/mask
    [2304, 1] bool: items I = 0, 1 drawn one after the other from the reference's
    WaveSource(sidelength=48, pretrain=(M == "pre")), M in ("pre", "train"). Item 0 of "train" has an empty
    time window (counter 0), so its mask is all true; item 1 has the mixed mask.

    end to end ("e2e/"): SingleBVPNet(type='sine', in_features=3, hidden_features=64, num_hidden_layers=2)
    under torch.manual_seed(0), on the batch ws/train/1 with a batch dimension of 1.
      e2e/init/*
      e2e/terms32 [3], e2e/grad32/*   the reference's wave_pml dict in float32, in its order, and
                         d(sum of the dict)/d(parameter)
      e2e/terms64 [3], e2e/grad64/*   the float64 truth. The reference's jacobian fills a float32
                         torch.zeros, so the reference in .double() does not give float64 derivatives: these
                         come from tests/_wave.formula64 on the reference model cast to double, with the
                         first and second derivatives by autograd
      e2e/terms_ref32_rel [3], e2e/grad_ref32_normrel/*   the reference's float32 against that float64
      e2e/min_margin [3]  the smallest |pred - src| and |u_t| over the masked rows and the smallest |e| over
                         all rows, in float64 (how far the batch is from the loss's kinks)
      e2e/traj [3, 3]    the three terms at the 3 steps of the reference's training.train (Adam, lr 2e-5, no
                         clipping) on this batch

    op-level ("op/"): tests/_wave.operands(2, 257, seed=40), R = 514: op/pred, op/jac, op/hess, op/src,
    op/slow, op/mask, with the planted flat rows op/row_pred_eq_src (masked), op/row_ut0 (masked) and
    op/row_e0, and slow in {1, 0.25}.
      op/terms64 [3], op/dpred64, op/djac64, op/dhess64   tests/_wave.formula64_grads under the upstream
                         weights (1, 2, 3)
      op/terms_ref32_rel [3], op/dpred_ref32_normrel, op/djac_ref32_normrel, op/dhess_ref32_normrel
                         the reference's wave_pml in float32 on these operands (its jacobian replaced by
                         functions returning op/jac and op/hess) against that float64
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
import _wave  # noqa: E402
from make_golden import OUT, import_reference, quiet, run_train, state_arrays  # noqa: E402

KEYS = _wave.KEYS


def norm_rel(a, b):
    den = torch.linalg.vector_norm(b.double()).item()
    return torch.linalg.vector_norm(a.double() - b.double()).item() / (den if den > 0 else 1.0)


def rel(a, b):
    return np.array([abs(x - y) / abs(y) if y != 0 else abs(x) for x, y in zip(a.double().tolist(), b.tolist())])


def wave_source(R, out):
    for mode, pretrain in (("pre", True), ("train", False)):
        ds = R.dataio.WaveSource(sidelength=48, pretrain=pretrain)
        for item in (0, 1):
            inp, gt = ds[0]
            p = f"ws/{mode}/{item}/"
            out[p + "coords"] = inp["coords"].numpy().copy()
            out[p + "src"] = gt["source_boundary_values"].numpy().copy()
            out[p + "mask"] = gt["dirichlet_mask"].numpy().copy()
            out[p + "slow"] = gt["squared_slowness"].numpy().copy()
            print(f"{p}: masked rows {int(gt['dirichlet_mask'].sum())}, t max {float(inp['coords'][:, 0].max()):.3e}, "
                  f"src max {float(gt['source_boundary_values'].max()):.4f}")


def run_model32(R, model, coords, gt):
    model.zero_grad()
    losses = R.loss_functions.wave_pml(model({"coords": coords}), gt)
    assert tuple(losses) == KEYS
    sum(losses.values()).backward()
    return (torch.stack([losses[k].detach().reshape(()) for k in KEYS]),
            {k: p.grad.detach().clone() for k, p in model.named_parameters()})


def derivatives64(model64, coords):
    """(y [B, N, 1], jac [B, N, 1, 3], hess [B, N, 1, 3, 3]) of the float64 model by autograd, differentiable."""
    o = model64({"coords": coords.double()})
    x, y = o["model_in"], o["model_out"]
    du = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
    hess = torch.stack([torch.autograd.grad(du[..., j].sum(), x, create_graph=True)[0] for j in range(3)], dim=-2)
    return y, du[:, :, None, :], hess[:, :, None]


def run_model64(model, coords, gt):
    m = copy.deepcopy(model).double()
    y, jac, hess = derivatives64(m, coords)
    src, slow, mask = gt["source_boundary_values"], gt["squared_slowness"], gt["dirichlet_mask"]
    terms = _wave.formula64(y, jac, hess, src, slow, mask)
    terms.sum().backward()
    e = (hess[..., 0, 0] - (hess[..., 1, 1] + hess[..., 2, 2]) / slow.double()).detach().abs()
    margin = np.array([(y.detach() - src.double()).abs()[mask].min().item(), jac.detach()[..., 0].abs()[mask].min().item(),
                       e.min().item()])
    return terms.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, margin


def e2e(R, out):
    coords = torch.from_numpy(out["ws/train/1/coords"])[None]
    gt = {"source_boundary_values": torch.from_numpy(out["ws/train/1/src"])[None],
          "dirichlet_mask": torch.from_numpy(out["ws/train/1/mask"])[None],
          "squared_slowness": torch.from_numpy(out["ws/train/1/slow"])[None]}
    torch.manual_seed(0)
    model = quiet(R.modules.SingleBVPNet, type="sine", in_features=3, hidden_features=64, num_hidden_layers=2)
    out.update(state_arrays(model, "e2e/init/"))
    t32, g32 = run_model32(R, model, coords, gt)
    t64, g64, margin = run_model64(model, coords, gt)
    assert all(torch.isfinite(g).all() for g in g32.values())
    out.update({"e2e/terms32": t32.numpy(), "e2e/terms64": t64.numpy(), "e2e/terms_ref32_rel": rel(t32, t64),
                "e2e/min_margin": margin})
    for k in g32:
        out[f"e2e/grad32/{k}"] = g32[k].numpy()
        out[f"e2e/grad64/{k}"] = g64[k].numpy()
        out[f"e2e/grad_ref32_normrel/{k}"] = np.array(norm_rel(g32[k], g64[k]))
    traj = []

    def loss_fn(model_output, gt_):
        losses = R.loss_functions.wave_pml(model_output, gt_)
        traj.append([float(losses[k]) for k in KEYS])
        return losses

    run_train(R, copy.deepcopy(model), coords, gt, loss_fn, steps=3, lr=2e-5, clip=False)
    out["e2e/traj"] = np.array(traj, dtype=np.float64)
    assert out["e2e/traj"].shape == (3, 3) and np.allclose(traj[0], t32.numpy(), rtol=1e-6)
    print("e2e terms32", t32.tolist(), "terms64", t64.tolist(), "ref32 rel", out["e2e/terms_ref32_rel"].tolist())
    print("e2e min margins (|pred - src|, |u_t|, |e|)", margin.tolist())
    print("e2e grad ref32 norm-rel", {k: float(out[f"e2e/grad_ref32_normrel/{k}"]) for k in g32})
    print("e2e trajectory", out["e2e/traj"].tolist())


def op_set(R, out):
    ops = _wave.operands(2, 257, seed=40)
    pred, jac, hess, src, slow, mask = ops
    t64, dp64, dj64, dh64 = _wave.formula64_grads(*ops, _wave.C)
    # the reference in float32 on the same operands: its two jacobian calls answered with jac and hess
    p, j, h = (t.clone().requires_grad_(True) for t in (pred, jac, hess))
    answers = iter([(j, 0), (h[:, :, 0], 0)])
    orig = R.loss_functions.diff_operators.jacobian
    R.loss_functions.diff_operators.jacobian = lambda y, x: next(answers)
    try:
        losses = R.loss_functions.wave_pml({"model_in": torch.zeros(2, 257, 3), "model_out": p},
                                           {"source_boundary_values": src, "squared_slowness": slow,
                                            "dirichlet_mask": mask})
    finally:
        R.loss_functions.diff_operators.jacobian = orig
    t32 = torch.stack([losses[k] for k in KEYS])
    (t32 * torch.tensor(_wave.C)).sum().backward()
    flat = mask.reshape(-1)
    assert flat[0] and flat[1] and pred.reshape(-1)[0] == src.reshape(-1)[0] and jac.reshape(-1, 3)[1, 0] == 0
    assert dp64.reshape(-1)[0] == 0 and dj64.reshape(-1, 3)[1, 0] == 0 and (dh64.reshape(-1, 9)[2] == 0).all()
    assert p.grad.reshape(-1)[0] == 0 and j.grad.reshape(-1, 3)[1, 0] == 0 and (h.grad.reshape(-1, 9)[2] == 0).all()
    assert set(slow.reshape(-1).tolist()) == {1.0, 0.25}
    for k, t in zip(_wave.OPERANDS, ops):
        out["op/" + k] = t.numpy()
    out.update({"op/row_pred_eq_src": np.array(0), "op/row_ut0": np.array(1), "op/row_e0": np.array(2),
                "op/terms64": t64.numpy(), "op/dpred64": dp64.numpy(), "op/djac64": dj64.numpy(),
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
    wave_source(R, out)
    e2e(R, out)
    op_set(R, out)
    path = os.path.join(OUT, "wave.npz")
    np.savez_compressed(path, **out)
    print("wrote wave.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
