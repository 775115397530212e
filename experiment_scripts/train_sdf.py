"""Counterpart of experiment_scripts/train_sdf.py (reference): fit a 3-input SIREN to the signed
distance function of an oriented point cloud (loss_functions.sdf: the output and its analytic
gradient, four terms in one native launch). Without --point_cloud_path an analytic torus
(dataio.write_synthetic_point_cloud) is written to a temporary file and used."""
from _common import base_parser  # noqa: E402

import os
import tempfile

import torch
from torch.utils.data import DataLoader

from siren_mri_amd import dataio, loss_functions, modules, training

p = base_parser(batch_size=1400, lr=1e-4, epochs_til_ckpt=1, steps_til_summary=100)
p.add_argument("--point_cloud_path", type=str, default=None,
               help="x y z nx ny nz text rows; default: a synthetic torus")
p.add_argument("--synthetic_points", type=int, default=100000, help="points of the synthetic torus")
p.add_argument("--device", type=str, default="cuda")
opt = p.parse_args()

if opt.point_cloud_path is not None:
    sdf_dataset = dataio.PointCloud(opt.point_cloud_path, on_surface_points=opt.batch_size)
else:
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "torus.xyz")
        dataio.write_synthetic_point_cloud(path, shape="torus", n=opt.synthetic_points, seed=0)
        sdf_dataset = dataio.PointCloud(path, on_surface_points=opt.batch_size)
dataloader = DataLoader(sdf_dataset, shuffle=True, batch_size=1, pin_memory=True, num_workers=0)

if opt.model_type != "sine":
    raise NotImplementedError("the native path covers type='sine'")
model = modules.SingleBVPNet(type="sine", in_features=3, precision=opt.precision)
if opt.checkpoint_path is not None:
    model.load_state_dict(torch.load(opt.checkpoint_path, weights_only=True))
model.to(torch.device(opt.device))


def summary_fn(model, model_input, gt, model_output, writer, total_steps):
    """Logs the four terms (summary steps only: the loss is evaluated once more for them)."""
    losses = {k: float(v.detach()) for k, v in loss_functions.sdf(model_output, gt).items()}
    for k, v in losses.items():
        writer.add_scalar(k, v, total_steps)
    print(f"step {total_steps}: " + ", ".join(f"{k} {v:.6f}" for k, v in losses.items()), flush=True)


training.train(model=model, train_dataloader=dataloader, epochs=opt.num_epochs, lr=opt.lr,
               steps_til_summary=opt.steps_til_summary, epochs_til_checkpoint=opt.epochs_til_ckpt,
               model_dir=os.path.join(opt.logging_root, opt.experiment_name), overwrite=opt.overwrite,
               loss_fn=loss_functions.sdf, summary_fn=summary_fn, double_precision=False, clip_grad=True)
