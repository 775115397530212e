"""Counterpart of experiment_scripts/train_helmholtz.py (reference): fit a SIREN u(x0, x1), a complex
field as two output channels, to the Helmholtz equation with one point-like source inside a perfectly
matched layer (loss_functions.helmholtz_pml on dataio.SingleHelmholtzSource: the output, its analytic
Jacobian and Hessian, the terms in one native launch). Only --model sine / --mode mlp run here; the
reference's tensorboard summary (utils.write_helmholtz_summary) stays out: the terms are printed."""
from _common import base_parser  # noqa: E402

import os

import torch
from torch.utils.data import DataLoader

from siren_mri_amd import dataio, loss_functions, modules, training

p = base_parser(batch_size=32, lr=2e-5, num_epochs=50000, epochs_til_ckpt=1000, steps_til_summary=100)
p.add_argument("--model", type=str, default="sine", choices=["sine", "tanh", "sigmoid", "relu"],
               help="nonlinearity of the model; only sine is on the native path")
p.add_argument("--mode", type=str, default="mlp", choices=["mlp", "rbf", "pinn"],
               help="input mapping / architecture; only mlp is on the native path")
p.add_argument("--velocity", type=str, default="uniform", choices=["uniform", "square", "circle"],
               help="velocity model: uniform, or a square / circular region of twice the velocity")
p.add_argument("--clip_grad", default=0.0, type=float, help="clip the gradient norm to this value (0: no clipping)")
p.add_argument("--use_lbfgs", default=False, type=bool, help="L-BFGS (the reference's PINN mode); not provided")
p.add_argument("--device", type=str, default="cuda")
p.add_argument("--sidelength", type=int, default=230, help="a batch is sidelength^2 rows (x0, x1)")
opt = p.parse_args()

if opt.model != "sine" or opt.mode != "mlp" or opt.use_lbfgs:
    raise NotImplementedError(f"train_helmholtz: --model {opt.model} --mode {opt.mode}"
                              f"{' --use_lbfgs' if opt.use_lbfgs else ''} is out of scope: the native path covers "
                              "--model sine --mode mlp with Adam (no PINNet, rbf or L-BFGS)")

# a velocity perturbation sits at the centre, so the source moves aside
source_coords = [0., 0.] if opt.velocity == "uniform" else [-0.35, 0.]
dataset = dataio.SingleHelmholtzSource(sidelength=opt.sidelength, velocity=opt.velocity, source_coords=source_coords)
dataloader = DataLoader(dataset, shuffle=True, batch_size=opt.batch_size, pin_memory=True, num_workers=0)

model = modules.SingleBVPNet(out_features=2, type="sine", mode="mlp", final_layer_factor=1., precision=opt.precision)
if opt.checkpoint_path is not None:
    model.load_state_dict(torch.load(opt.checkpoint_path, weights_only=True))
model.to(torch.device(opt.device))

last = {}


def loss_fn(model_output, gt):
    losses = loss_functions.helmholtz_pml(model_output, gt)
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
