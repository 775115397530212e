"""Time Helmholtz fitting in train_helmholtz.py's configuration (a 2-256x4-2 SIREN, one
SingleHelmholtzSource(sidelength=230) item: 1 x 52,900 rows), in fp32 and bf16 mode. Per precision:

  loss   forward + backward of the loss alone on a fixed native (y, jac, hess) of that model: the native op
         (siren_mri_amd::helmholtz_loss + helmholtz_loss_bwd) against the expression path
         (set_helmholtz_loss_native(False)),
         interleaved
  step   the whole training step (forward, diff_operators.jacobian and hessian, the loss, backward, Adam),
         both arms, interleaved
  parts  what the step is made of, each alone, forward + backward to the parameters under a fixed
         cotangent: the model's forward, the Jacobian pass, the Hessian pass (the loss is `loss` above)

Everything runs in one process after a warm-up; a repetition is `--inner` calls between two device events,
and a figure is the median over `--reps` repetitions (min, max and the raw repetitions are printed too).

    python tools/helmholtz_time.py [--sidelength 230] [--reps 12] [--inner 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siren_mri_amd import _native, dataio, diff_operators, loss_functions, modules, training  # noqa: E402


def make_batch(sidelength, dev):
    inp, gt = dataio.SingleHelmholtzSource(sidelength=sidelength)[0]
    gt = {"source_boundary_values": gt["source_boundary_values"], "squared_slowness": gt["squared_slowness"],
          "wavenumber": torch.tensor(gt["wavenumber"], dtype=torch.float32)}
    return {k: v[None].to(dev) for k, v in inp.items()}, {k: v[None].to(dev) for k, v in gt.items()}


def make_fns(precision, sidelength, dev):
    torch.manual_seed(0)
    model = modules.SingleBVPNet(type="sine", in_features=2, out_features=2, hidden_features=256, num_hidden_layers=3,
                                 precision=precision).to(dev)
    params = list(model.parameters())
    optim = training.make_adam(params, 2e-5)
    inp, gt = make_batch(sidelength, dev)
    src, slow, k = gt["source_boundary_values"], gt["squared_slowness"], gt["wavenumber"]

    def step():
        losses = loss_functions.helmholtz_pml(model(inp), gt)
        training.compute_loss(losses, None, 0, None).backward()
        optim.step()
        optim.zero_grad()

    o = model(inp)
    y0, x0 = o["model_out"], o["model_in"]
    jac0, hess0 = diff_operators.jacobian(y0, x0)[0], diff_operators.hessian(y0, x0)[0]
    y, jac, hess = (t.detach().clone().requires_grad_(True) for t in (y0, jac0, hess0))
    cy, cj, ch = (torch.randn_like(t) for t in (y0, jac0, hess0))
    x = x0.detach()
    del o, y0, x0, jac0, hess0

    def loss_only():
        y.grad = jac.grad = hess.grad = None
        if loss_functions._helmholtz_native_applies(x, y, jac, hess, src, slow, k):
            terms = torch.ops.siren_mri_amd.helmholtz_loss(x, y, jac, hess, src, slow, k)
            losses = dict(zip(loss_functions._HELMHOLTZ_KEYS, terms.unbind(0)))
        else:
            losses = loss_functions._helmholtz_expression(x, y, jac, hess, src, slow, k)
        training.compute_loss(losses, None, 0, None).backward()

    def forward_part():
        torch.autograd.grad(model(inp)["model_out"], params, cy)

    def pass_part(op, cot):
        out = model(inp)
        yy, xx = out["model_out"], out["model_in"]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        d = op(yy, xx)[0]
        torch.autograd.grad(d, params, cot, allow_unused=True)
        t1.record()
        return t0, t1

    return {"step": step, "loss": loss_only, "forward": forward_part,
            "jacobian": lambda: pass_part(diff_operators.jacobian, cj),
            "hessian": lambda: pass_part(diff_operators.hessian, ch)}, inp["coords"].shape[1]


def timed(fn, inner):
    """us per call: between two device events, or, for a part that brackets itself, the sum of its brackets."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    own = [fn() for _ in range(inner)]
    t1.record()
    t1.synchronize()
    if own[0] is not None:
        return sum(a.elapsed_time(b) for a, b in own) / inner * 1e3
    return t0.elapsed_time(t1) / inner * 1e3


def summary(t):
    return {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "rounds_us": [round(x, 1) for x in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sidelength", type=int, default=230)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("helmholtz_time: no GPU (a timing is taken on the device or not at all)")
    _native.load_library()
    dev = torch.device("cuda", 0)
    arms = {"native": True, "expression": False}
    lines, out = [], {"reps": args.reps, "inner": args.inner}
    try:
        for precision in ("fp32", "bf16"):
            fns, rows = make_fns(precision, args.sidelength, dev)
            if not lines:
                lines += [f"helmholtz_time: Helmholtz fitting, 2-256x4-2 SIREN, 1 x {rows} rows, {torch.cuda.get_device_name(0)}",
                          f"  {args.reps} repetitions, {args.inner} calls each between device events, {args.warmup} "
                          "warm-up calls; us per call: median (min, max)"]
                out["rows"] = rows
            for what in ("loss", "step"):
                times = {k: [] for k in arms}
                for native in arms.values():
                    loss_functions.set_helmholtz_loss_native(native)
                    for _ in range(args.warmup):
                        fns[what]()
                for _ in range(args.reps):
                    for name, native in arms.items():
                        loss_functions.set_helmholtz_loss_native(native)
                        times[name].append(timed(fns[what], args.inner))
                res = {name: summary(t) for name, t in times.items()}
                res["expression_over_native"] = res["expression"]["median_us"] / res["native"]["median_us"]
                for name in arms:
                    r = res[name]
                    lines.append(f"  {precision} {what:<8} {name:<10} {r['median_us']:10.1f}  ({r['min_us']:.1f}, {r['max_us']:.1f})")
                    lines.append(f"      rounds: {' '.join(f'{x:.1f}' for x in r['rounds_us'])}")
                lines.append(f"  {precision} {what:<8} expression / native = {res['expression_over_native']:.2f}x")
                out[f"{precision}_{what}"] = res
            loss_functions.set_helmholtz_loss_native(True)
            step_us = out[f"{precision}_step"]["native"]["median_us"]
            for what in ("forward", "jacobian", "hessian"):
                for _ in range(args.warmup):
                    fns[what]()
                r = summary([timed(fns[what], args.inner) for _ in range(args.reps)])
                lines.append(f"  {precision} {what:<8} fwd + bwd  {r['median_us']:10.1f}  ({r['min_us']:.1f}, {r['max_us']:.1f})  "
                             f"= {100 * r['median_us'] / step_us:.1f}% of the native step")
                lines.append(f"      rounds: {' '.join(f'{x:.1f}' for x in r['rounds_us'])}")
                out[f"{precision}_{what}"] = r
            loss_us = out[f"{precision}_loss"]["native"]["median_us"]
            lines.append(f"  {precision} loss     fwd + bwd  {loss_us:10.1f}  = {100 * loss_us / step_us:.1f}% of the native step")
            del fns
            torch.cuda.empty_cache()
    finally:
        loss_functions.set_helmholtz_loss_native(True)
    lines.append(json.dumps(out))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
