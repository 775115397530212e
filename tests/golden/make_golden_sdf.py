"""Golden vectors of signed-distance fitting from the REAL reference (run in the build container only,
on the CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sdf.py

  sdf.npz
    op-level, per set S in ("d3": [2, 256, .] rows, D = 3; "d2": [1, 128, .], D = 2), every value fp32:
      S/pred, S/grad, S/sdf, S/normals   loss_functions.sdf's operands (loss_functions.py:460-484; its
                         diff_operators.gradient is replaced by a function returning S/grad, so pred and
                         grad are independent leaves). Half the rows of each batch are on the surface
                         (sdf 0, unit normals), half off it (sdf -1, normals -1); |grad| is 1 +- u,
                         u in [0.01, 0.5], above and below 1 in equal numbers. Planted rows (flat row
                         indices):
                           S/pred0_on, S/pred0_off   pred == 0
                           S/grad0                   grad == 0 (on- and off-surface)
                           S/grad_unit               grad == e_k, |grad| exactly 1 (on- and off-surface)
                           S/grad_par, S/grad_anti   grad = 0.7 normal, grad = -1.3 normal (on-surface)
      S/terms64 [4]      the reference's dict on the float64 copies, in its order
      S/dpred64, S/dgrad64   d(sum_k c_k term_k) / d(pred, grad) in float64, c = (1, 2, 3, 4)
      S/terms32, S/terms_ref32_rel [4], S/dpred_ref32_normrel, S/dgrad_ref32_normrel
                         the reference on the float32 values and its own float32-against-float64 errors
    The generator asserts that every row outside pred0_* has |pred| > 1e-3 and every row outside grad0 /
    grad_unit has | |grad| - 1 | > 1e-3 (so float32 and float64 take the same signs), and the zeros the
    tests rely on: dpred == 0 at pred0_*, and the grad_constraint part of dgrad == 0 at grad0 / grad_unit.

    end to end ("e2e/"): SingleBVPNet(type='sine', in_features=3, hidden_features=64, num_hidden_layers=1)
    under torch.manual_seed(seed); 128 points on the sphere of radius 0.6 with their normals, then 128
    uniform points of the cube (sdf -1, normals -1). seed is the first of 0..15 for which every row has
    |y| > 1e-3 and | |grad y| - 1 | > 1e-3 in float64, at the start and at each of the 3 training steps
    below (e2e/min_abs_y, e2e/min_abs_gnorm_m1 are the minima at the start; no seed qualifying is an error).
      e2e/init/*, e2e/coords, e2e/sdf, e2e/normals
      e2e/terms32 [4], e2e/grad32/*      the reference's float32 dict and d(sum of the dict)/d(parameter)
      e2e/terms64 [4], e2e/grad64/*      the same from the float64 copy of the model and the data
      e2e/terms_ref32_rel [4], e2e/grad_ref32_normrel/*   float32 against float64
      e2e/traj [3, 4]    the four terms at the 3 steps of the reference's training.train (Adam, lr 1e-4,
                         clip_grad=True) on this batch

    PointCloud ("pc/"): pc/cloud [64, 6] (an anisotropic oriented cloud as np.genfromtxt reads it back from
    its text file); pc/K/coords, pc/K/sdf, pc/K/normals: the reference's PointCloud(file, 16,
    keep_aspect_ratio=K).__getitem__(0) under np.random.seed(0), K in ("keep", "free").
Only data leaves the reference: no source is copied.
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, quiet, run_train, state_arrays  # noqa: E402

KEYS = ("sdf", "inter", "normal_constraint", "grad_constraint")
C = (1.0, 2.0, 3.0, 4.0)
MARGIN = 1e-3


def norm_rel(a, b):
    den = torch.linalg.vector_norm(b.double()).item()
    return torch.linalg.vector_norm(a.double() - b.double()).item() / (den if den > 0 else 1.0)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def make_op_inputs(batch, n, d, seed):
    """(pred [B, N, 1], grad [B, N, D], sdf [B, N, 1], normals [B, N, D]) float32 and the planted flat
    row indices."""
    g = torch.Generator().manual_seed(seed)
    rows = batch * n
    on = torch.zeros(batch, n, dtype=torch.bool)
    on[:, : n // 2] = True
    on = on.reshape(rows)
    sign = torch.where(torch.rand(rows, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    mag = torch.where(on, 0.05, 0.03) * torch.randn(rows, generator=g, dtype=torch.float64).abs() + 2 * MARGIN
    pred = (sign * mag).to(torch.float32)
    normals = unit(torch.randn(rows, d, generator=g, dtype=torch.float64))
    u = 0.01 + 0.49 * torch.rand(rows, generator=g, dtype=torch.float64)
    gnorm = torch.where(torch.arange(rows) % 2 == 0, 1 + u, 1 - u)
    grad = (gnorm[:, None] * unit(normals + 0.8 * torch.randn(rows, d, generator=g, dtype=torch.float64))).to(torch.float32)
    normals = normals.to(torch.float32)
    on_rows, off_rows = torch.nonzero(on)[:, 0], torch.nonzero(~on)[:, 0]
    on_rows = on_rows[torch.randperm(on_rows.numel(), generator=g)]
    off_rows = off_rows[torch.randperm(off_rows.numel(), generator=g)]
    idx = {"pred0_on": on_rows[0:4], "pred0_off": off_rows[0:4],
           "grad0": torch.cat([on_rows[4:6], off_rows[4:6]]),
           "grad_unit": torch.cat([on_rows[6:6 + d], off_rows[6:6 + d]]),
           "grad_par": on_rows[10:14], "grad_anti": on_rows[14:18]}
    pred[idx["pred0_on"]] = 0.0
    pred[idx["pred0_off"]] = 0.0
    grad[idx["grad0"]] = 0.0
    for j, r in enumerate(idx["grad_unit"].tolist()):
        grad[r] = torch.eye(d)[j % d]
    grad[idx["grad_par"]] = 0.7 * normals[idx["grad_par"]]
    grad[idx["grad_anti"]] = -1.3 * normals[idx["grad_anti"]]
    normals[~on] = -1.0
    sdf = torch.where(on, 0.0, -1.0).to(torch.float32)
    # what the tests rely on: float32 and float64 take the same signs off the planted rows
    free_p = torch.ones(rows, dtype=torch.bool)
    free_p[torch.cat([idx["pred0_on"], idx["pred0_off"]])] = False
    free_g = torch.ones(rows, dtype=torch.bool)
    free_g[torch.cat([idx["grad0"], idx["grad_unit"]])] = False
    assert (pred[free_p].abs() > MARGIN).all()
    assert ((grad.double().norm(dim=-1) - 1).abs()[free_g] > MARGIN).all()
    above = int(((grad.double().norm(dim=-1) > 1) & free_g).sum())
    assert abs(above - int(free_g.sum()) / 2) < 0.1 * rows, above
    return (pred.view(batch, n, 1), grad.view(batch, n, d), sdf.view(batch, n, 1), normals.view(batch, n, d)), idx


def run_op(R, pred, grad, sdf, normals):
    """The reference's dict and d(sum c_k term_k)/d(pred, grad) with the gradient operator replaced by `grad`."""
    p, gr = pred.clone().requires_grad_(True), grad.clone().requires_grad_(True)
    orig = R.loss_functions.diff_operators.gradient
    R.loss_functions.diff_operators.gradient = lambda y, x: gr
    try:
        losses = R.loss_functions.sdf({"model_in": None, "model_out": p}, {"sdf": sdf, "normals": normals})
    finally:
        R.loss_functions.diff_operators.gradient = orig
    assert tuple(losses) == KEYS
    terms = torch.stack([losses[k] for k in KEYS])
    (terms * torch.tensor(C, dtype=terms.dtype)).sum().backward()
    return terms.detach(), p.grad.detach(), gr.grad.detach()


def op_set(R, tag, batch, n, d, seed, out):
    (pred, grad, sdf, normals), idx = make_op_inputs(batch, n, d, seed)
    t64, dp64, dg64 = run_op(R, pred.double(), grad.double(), sdf.double(), normals.double())
    t32, dp32, dg32 = run_op(R, pred, grad, sdf, normals)
    for t in (t64, dp64, dg64, t32, dp32, dg32):
        assert torch.isfinite(t).all(), tag
    for k in ("pred0_on", "pred0_off"):
        assert (dp64.view(-1)[idx[k]] == 0).all() and (dp32.view(-1)[idx[k]] == 0).all(), k
    off = sdf.view(-1) == -1  # off-surface: dgrad is the grad_constraint part alone
    for k in ("grad0", "grad_unit"):
        rows = idx[k][off[idx[k]]]
        assert (dg64.view(-1, d)[rows] == 0).all() and (dg32.view(-1, d)[rows] == 0).all(), k
    out.update({f"{tag}/pred": pred.numpy(), f"{tag}/grad": grad.numpy(), f"{tag}/sdf": sdf.numpy(),
                f"{tag}/normals": normals.numpy(), f"{tag}/terms64": t64.numpy(), f"{tag}/dpred64": dp64.numpy(),
                f"{tag}/dgrad64": dg64.numpy(), f"{tag}/terms32": t32.numpy(),
                f"{tag}/terms_ref32_rel": ((t32.double() - t64).abs() / t64.abs()).numpy(),
                f"{tag}/dpred_ref32_normrel": np.array(norm_rel(dp32, dp64)),
                f"{tag}/dgrad_ref32_normrel": np.array(norm_rel(dg32, dg64))})
    out.update({f"{tag}/{k}": v.numpy() for k, v in idx.items()})
    print(f"{tag}: terms64 {t64.tolist()}\n    ref32 terms rel {out[f'{tag}/terms_ref32_rel'].tolist()} "
          f"dpred {out[f'{tag}/dpred_ref32_normrel']:.2e} dgrad {out[f'{tag}/dgrad_ref32_normrel']:.2e}")


def e2e_data():
    rs = np.random.RandomState(100)
    nrm = rs.standard_normal((128, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    coords = np.concatenate((0.6 * nrm, rs.uniform(-1, 1, size=(128, 3))), axis=0)
    normals = np.concatenate((nrm, -np.ones((128, 3))), axis=0)
    sdf = np.concatenate((np.zeros((128, 1)), -np.ones((128, 1))), axis=0)
    return (torch.from_numpy(coords).float()[None], torch.from_numpy(sdf).float()[None],
            torch.from_numpy(normals).float()[None])


def margins(R, model, coords):
    """(min |y|, min | |grad y| - 1 |) of the float64 copy of the model."""
    m = copy.deepcopy(model).double()
    o = m({"coords": coords.double()})
    g = R.diff_operators.gradient(o["model_out"], o["model_in"])
    return (o["model_out"].detach().abs().min().item(), (g.detach().norm(dim=-1) - 1).abs().min().item())


def run_model(R, model, coords, gt):
    model.zero_grad()
    losses = R.loss_functions.sdf(model({"coords": coords}), gt)
    assert tuple(losses) == KEYS
    sum(losses.values()).backward()
    return (torch.stack([losses[k].detach() for k in KEYS]),
            {k: p.grad.detach().clone() for k, p in model.named_parameters()})


def trajectory(R, model, coords, gt, steps=3):
    """The four terms at each step of the reference's training.train (Adam, lr 1e-4, clip_grad=True) on a
    copy of the model, or None if a step's rows come within MARGIN of the loss's kinks."""
    m = copy.deepcopy(model)
    traj, ok = [], []

    def loss_fn(model_output, gt_):
        my, mg = margins(R, m, coords)
        ok.append(my > MARGIN and mg > MARGIN)
        losses = R.loss_functions.sdf(model_output, gt_)
        traj.append([losses[k].item() for k in KEYS])
        return losses

    run_train(R, m, coords, gt, loss_fn, steps=steps, lr=1e-4, clip=True)
    assert len(traj) == steps
    return np.array(traj, dtype=np.float64) if all(ok) else None


def e2e(R, out):
    coords, sdf, normals = e2e_data()
    gt = {"sdf": sdf, "normals": normals}
    for seed in range(16):
        torch.manual_seed(seed)
        model = quiet(R.modules.SingleBVPNet, type="sine", in_features=3, hidden_features=64, num_hidden_layers=1)
        my, mg = margins(R, model, coords)
        traj = trajectory(R, model, coords, gt) if my > MARGIN and mg > MARGIN else None
        print(f"e2e seed {seed}: min |y| {my:.3e}, min ||grad y| - 1| {mg:.3e}, "
              f"{'qualifies' if traj is not None else 'too close to a kink at the start or at a later step'}")
        if traj is not None:
            break
    else:
        raise SystemExit("no seed in 0..15 keeps every row off the loss's kinks over the 3 steps")
    out.update({"e2e/seed": np.array(seed), "e2e/min_abs_y": np.array(my), "e2e/min_abs_gnorm_m1": np.array(mg),
                "e2e/coords": coords.numpy(), "e2e/sdf": sdf.numpy(), "e2e/normals": normals.numpy(),
                "e2e/traj": traj})
    out.update(state_arrays(model, "e2e/init/"))
    t32, g32 = run_model(R, model, coords, gt)
    m64 = copy.deepcopy(model).double()
    t64, g64 = run_model(R, m64, coords.double(), {k: v.double() for k, v in gt.items()})
    assert all(g is not None and torch.isfinite(g).all() for g in g32.values())
    assert np.allclose(traj[0], t32.numpy(), rtol=1e-6)
    out.update({"e2e/terms32": t32.numpy(), "e2e/terms64": t64.numpy(),
                "e2e/terms_ref32_rel": ((t32.double() - t64).abs() / t64.abs()).numpy()})
    for k in g32:
        out[f"e2e/grad32/{k}"] = g32[k].numpy()
        out[f"e2e/grad64/{k}"] = g64[k].numpy()
        out[f"e2e/grad_ref32_normrel/{k}"] = np.array(norm_rel(g32[k], g64[k]))
    print("e2e terms32", t32.tolist(), "ref32 rel", out["e2e/terms_ref32_rel"].tolist())
    print("e2e grad ref32 norm-rel", {k: float(out[f"e2e/grad_ref32_normrel/{k}"]) for k in g32})
    print("e2e trajectory", traj.tolist())


def point_cloud(R, out):
    rs = np.random.RandomState(7)
    nrm = rs.standard_normal((64, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cloud = np.concatenate((nrm * np.array([1.0, 0.5, 0.25]) + np.array([0.3, -0.1, 0.2]), nrm), axis=1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cloud.xyz")
        np.savetxt(path, cloud, fmt="%.8f")
        out["pc/cloud"] = np.genfromtxt(path)
        for tag, keep in (("keep", True), ("free", False)):
            ds = quiet(R.dataio.PointCloud, path, 16, keep_aspect_ratio=keep)
            assert len(ds) == 4
            np.random.seed(0)
            inp, gt = ds[0]
            out[f"pc/{tag}/coords"] = inp["coords"].numpy()
            out[f"pc/{tag}/sdf"] = gt["sdf"].numpy()
            out[f"pc/{tag}/normals"] = gt["normals"].numpy()


def main():
    R = import_reference()
    torch.set_num_threads(8)
    out = {}
    op_set(R, "d3", 2, 256, 3, 40, out)
    op_set(R, "d2", 1, 128, 2, 41, out)
    e2e(R, out)
    point_cloud(R, out)
    path = os.path.join(OUT, "sdf.npz")
    np.savez_compressed(path, **out)
    print("wrote sdf.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
