"""Time signed-distance fitting in train_sdf.py's configuration (a 3-256x4-1 SIREN, 1400 on-surface and
1400 off-surface points): the native loss op (siren_mri_amd::sdf_loss) against the expression path
(set_sdf_loss_native(False)), in fp32 and bf16 mode. Two figures per precision and arm:

  step   forward, diff_operators.gradient, the loss, backward, clip_grad_norm_ and the Adam step
  loss   forward + backward of the loss alone on a fixed (y, grad y) of that model: no stack op

Both arms run in one process, interleaved, after a warm-up; each repetition is `--inner` steps between
two device events, and the figure per arm is the median over `--reps` repetitions (the raw repetitions
are printed too). Also printed: the launches of one step of each arm (torch.profiler).

    python tools/sdf_time.py [--rows 1400] [--reps 30] [--inner 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siren_mri_amd import _native, diff_operators, loss_functions, modules, training  # noqa: E402


def make_batch(on_surface, dev):
    """One PointCloud-shaped batch: points of the unit-box torus's surface with their normals, then
    uniform points (sdf -1, normals -1)."""
    rs = np.random.RandomState(0)
    u, v = rs.uniform(0, 2 * np.pi, on_surface), rs.uniform(0, 2 * np.pi, on_surface)
    nrm = np.stack((np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)), axis=1)
    pts = (np.stack((0.6 * np.cos(u), 0.6 * np.sin(u), 0 * u), axis=1) + 0.25 * nrm) / 0.85
    coords = np.concatenate((pts, rs.uniform(-1, 1, (on_surface, 3))))
    normals = np.concatenate((nrm, -np.ones((on_surface, 3))))
    sdf = np.concatenate((np.zeros((on_surface, 1)), -np.ones((on_surface, 1))))
    t = [torch.from_numpy(a).float()[None].to(dev) for a in (coords, sdf, normals)]
    return {"coords": t[0]}, {"sdf": t[1], "normals": t[2]}


def make_steps(precision, on_surface, dev):
    torch.manual_seed(0)
    model = modules.SingleBVPNet(type="sine", in_features=3, precision=precision).to(dev)
    optim = training.make_adam(model.parameters(), 1e-4)
    inp, gt = make_batch(on_surface, dev)

    def step():
        losses = loss_functions.sdf(model(inp), gt)
        training.compute_loss(losses, None, 0, None).backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        optim.step()
        optim.zero_grad()

    o = model(inp)
    y = o["model_out"].detach().clone().requires_grad_(True)
    g = diff_operators.gradient(o["model_out"], o["model_in"]).detach().clone().requires_grad_(True)
    del o

    def loss_only():
        y.grad = g.grad = None
        if loss_functions._sdf_native_applies(y, g, gt["sdf"], gt["normals"]):
            terms = torch.ops.siren_mri_amd.sdf_loss(y, g, gt["sdf"], gt["normals"])
            losses = dict(zip(loss_functions._SDF_KEYS, terms.unbind(0)))
        else:
            losses = loss_functions._sdf_expression(y, g, gt["sdf"], gt["normals"])
        training.compute_loss(losses, None, 0, None).backward()

    return {"step": step, "loss": loss_only}


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1400, help="on-surface points (as many off-surface ones are added)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_time: no GPU (a timing is taken on the device or not at all)")
    _native.load_library()
    dev = torch.device("cuda", 0)
    arms = {"native": True, "expression": False}
    lines = [f"sdf_time: signed-distance fitting, 3-256x4-1 SIREN, {2 * args.rows} rows, {torch.cuda.get_device_name(0)}",
             f"  {args.reps} repetitions per arm, interleaved, {args.inner} steps each between device events, "
             f"{args.warmup} warm-up steps; us per step"]
    out = {"rows": 2 * args.rows, "reps": args.reps, "inner": args.inner}
    try:
        for precision in ("fp32", "bf16"):
            fns = make_steps(precision, args.rows, dev)
            for what, fn in fns.items():
                times, count = {k: [] for k in arms}, {}
                for name, native in arms.items():
                    loss_functions.set_sdf_loss_native(native)
                    for _ in range(args.warmup):
                        fn()
                    count[name] = launches(fn)
                for _ in range(args.reps):
                    for name, native in arms.items():
                        loss_functions.set_sdf_loss_native(native)
                        fn()
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        for _ in range(args.inner):
                            fn()
                        t1.record()
                        t1.synchronize()
                        times[name].append(t0.elapsed_time(t1) / args.inner * 1e3)
                res = {}
                for name in arms:
                    t = times[name]
                    res[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                 "launches": count[name], "rounds_us": [round(x, 1) for x in t]}
                    lines.append(f"  {precision} {what:<4} {name:<10} median {res[name]['median_us']:8.1f}  (min {min(t):.1f}, "
                                 f"max {max(t):.1f}), {count[name]} launches per step")
                    lines.append(f"      rounds: {' '.join(f'{x:.1f}' for x in t)}")
                res["expression_over_native"] = res["expression"]["median_us"] / res["native"]["median_us"]
                lines.append(f"  {precision} {what:<4} expression / native = {res['expression_over_native']:.2f}x")
                out[f"{precision}_{what}"] = res
    finally:
        loss_functions.set_sdf_loss_native(True)
    lines.append(json.dumps(out))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
