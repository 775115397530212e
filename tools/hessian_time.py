"""Time diff_operators.hessian of a SIREN output (default: 256^2 coordinates, a 2-256-256-256-256-1
fp32 SIREN), and one image_mse_FH_prior step (forward plus backward) where the tree it runs in has
that loss. The model's forward runs before each timed call with grad mode on (the composite
autograd path needs its graph); the timed call itself runs under no_grad where the tree has the
native Hessian and with grad mode on otherwise (the composite path cannot run under no_grad). Each
figure is the median over --reps calls, each bracketed by two device events, after --warmup calls.
The file imports the package of the tree it lies in, so a copy of it in a checkout of another
commit times that commit on the same inputs.

    python tools/hessian_time.py [--side 256] [--hidden 256] [--layers 3] [--reps 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siren_mri_amd import _native, dataio, diff_operators, jvp, loss_functions, modules  # noqa: E402


def timed(fn, reps, warmup, before=None):
    """Median / min / max time of fn() in microseconds; before() runs ahead of every call, outside
    its two device events."""
    ts = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if i >= warmup:
            ts.append(t0.elapsed_time(t1) * 1e3)
    ts.sort()
    return {"median_us": statistics.median(ts), "min_us": ts[0], "max_us": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3, help="num_hidden_layers")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hessian_time: no GPU (a timing is taken on the device or not at all)")
    _native.load_library()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = modules.SingleBVPNet(type="sine", mode="mlp", hidden_features=args.hidden, num_hidden_layers=args.layers,
                             precision="fp32").to(dev)
    coords = dataio.get_mgrid(args.side)[None].to(dev)
    native = hasattr(jvp, "siren_hessian")
    state = {}

    def forward():
        state["o"] = m({"coords": coords})

    def hess():
        o = state["o"]
        if native:
            with torch.no_grad():
                state["h"] = diff_operators.hessian(o["model_out"], o["model_in"])[0]
        else:
            state["h"] = diff_operators.hessian(o["model_out"], o["model_in"])[0].detach()

    out = {"side": args.side, "hidden": args.hidden, "layers": args.layers, "reps": args.reps, "warmup": args.warmup,
           "path": "native tangent streams" if native else "composite autograd rounds"}
    out["hessian"] = timed(hess, args.reps, args.warmup, before=forward)
    h = state["h"]
    out["hessian_checksum"] = h.double().abs().sum().item()
    lines = [f"hessian_time: diff_operators.hessian, {args.side}^2 coordinates, 2-" +
             "-".join([str(args.hidden)] * (args.layers + 1)) + f"-1 SIREN, fp32, {torch.cuda.get_device_name(0)}",
             f"  path: {out['path']}; median of {args.reps} calls between device events after {args.warmup} warm-up calls",
             "  hessian      median {median_us:10.1f} us  (min {min_us:.1f}, max {max_us:.1f})".format(**out["hessian"]),
             f"  sum |H| = {out['hessian_checksum']:.9g}"]
    if hasattr(loss_functions, "image_mse_FH_prior"):
        g = torch.Generator().manual_seed(1)
        gt = {"img": torch.randn(1, args.side ** 2, 1, generator=g).to(dev)}
        mask = (torch.rand(args.side ** 2, 1, generator=g) < 0.1).float().to(dev)

        def fh_step():
            m.zero_grad(set_to_none=True)
            o = m({"coords": coords})
            losses = loss_functions.image_mse_FH_prior(mask, 0.5, m, o, gt)
            sum(losses.values()).backward()

        out["fh_prior_step"] = timed(fh_step, args.reps, args.warmup)
        lines.append("  FH prior step median {median_us:10.1f} us  (min {min_us:.1f}, max {max_us:.1f}): model forward, "
                     "image_mse_FH_prior, backward".format(**out["fh_prior_step"]))
    lines.append(json.dumps(out))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
