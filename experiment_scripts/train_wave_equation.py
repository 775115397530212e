"""Counterpart of experiment_scripts/train_wave_equation.py (reference): fit a SIREN u(t, x, y) to the
wave equation with a Gaussian source pulse at t = 0 (loss_functions.wave_pml on dataio.WaveSource: the
output, its analytic Jacobian and Hessian, three terms in one native launch). --pretrain fits the
initial condition alone for the first 2000 steps, as the reference does."""
from _common import base_parser  # noqa: E402

import os

import torch
from torch.utils.data import DataLoader

from siren_mri_amd import dataio, loss_functions, modules, training

p = base_parser(batch_size=32, lr=2e-5, num_epochs=100000, epochs_til_ckpt=1000, steps_til_summary=100)
p.add_argument("--velocity", type=str, default="uniform", choices=["uniform", "square", "circle"],
               help="velocity model: uniform, or a square / circular region of twice the velocity")
p.add_argument("--pretrain", action="store_true", default=False, help="pretrain the Dirichlet and Neumann conditions")
p.add_argument("--clip_grad", default=0.0, type=float, help="clip the gradient norm to this value (0: no clipping)")
p.add_argument("--device", type=str, default="cuda")
p.add_argument("--sidelength", type=int, default=340, help="a batch is sidelength^2 rows (t, x, y)")
p.add_argument("--hidden_features", type=int, default=512)
opt = p.parse_args()

dataset = dataio.WaveSource(sidelength=opt.sidelength, velocity=opt.velocity, source_coords=[0., 0., 0.],
                            pretrain=opt.pretrain)
dataloader = DataLoader(dataset, shuffle=True, batch_size=opt.batch_size, pin_memory=True, num_workers=0)

if opt.model_type != "sine":
    raise NotImplementedError("the native path covers type='sine'")
model = modules.SingleBVPNet(type="sine", in_features=3, out_features=1, hidden_features=opt.hidden_features,
                             num_hidden_layers=3, precision=opt.precision)
if opt.checkpoint_path is not None:
    model.load_state_dict(torch.load(opt.checkpoint_path, weights_only=True))
model.to(torch.device(opt.device))

last = {}


def loss_fn(model_output, gt):
    losses = loss_functions.wave_pml(model_output, gt)
    last.clear()
    last.update({k: v.detach() for k, v in losses.items()})
    return losses


def summary_fn(model, model_input, gt, model_output, writer, total_steps):
    """Logs the three terms of the step's loss (summary steps only)."""
    losses = {k: float(v) for k, v in last.items()}
    for k, v in losses.items():
        writer.add_scalar(k, v, total_steps)
    print(f"step {total_steps}: " + ", ".join(f"{k} {v:.6f}" for k, v in losses.items()), flush=True)


training.train(model=model, train_dataloader=dataloader, epochs=opt.num_epochs, lr=opt.lr,
               steps_til_summary=opt.steps_til_summary, epochs_til_checkpoint=opt.epochs_til_ckpt,
               model_dir=os.path.join(opt.logging_root, opt.experiment_name), overwrite=opt.overwrite,
               loss_fn=loss_fn, summary_fn=summary_fn, double_precision=False, clip_grad=opt.clip_grad)
