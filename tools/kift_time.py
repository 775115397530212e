"""Time image_hypernetwork_ift_loss, forward plus backward, on a data-consistent [B, side^2, 2] output
(default: config 4's [32, 16384, 2]): the native op (siren_mri_amd::kspace_ift_loss) against the
expression path (set_kspace_loss_native(False): torch.fft.ifft2 twice, the complex elementwise chain,
complex autograd). Both arms run in one process, interleaved, after a warm-up; each repetition is
`--inner` steps between two device events, and the figure per arm is the median over `--reps`
repetitions. Also printed: the launches of one step of each arm (torch.profiler) and how far the two
arms' loss and gradient are apart.

    python tools/kift_time.py [--batch 32] [--side 128] [--reps 30] [--inner 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from siren_mri_amd import _native, loss_functions  # noqa: E402
from siren_mri_amd.data_consistency import DataConsistencyInKspace  # noqa: E402


def make_step(batch, side, dev):
    g = torch.Generator().manual_seed(0)
    n = side * side
    amp = 0.5 * torch.exp(-3.0 * torch.rand(batch, n, 1, generator=g))
    pred = (amp * torch.randn(batch, n, 2, generator=g)).to(dev).requires_grad_(True)
    tgt = (amp * torch.randn(batch, n, 2, generator=g)).to(dev)
    k0 = tgt.permute(0, 2, 1).reshape(batch, 2, side, side).contiguous()
    mask = (torch.rand(batch, 2, side, side, generator=g) < 0.33).float().to(dev)
    latent = torch.randn(batch, 256, generator=g).to(dev).requires_grad_(True)
    hypo = {"w": torch.randn(batch, 4096, generator=g).to(dev).requires_grad_(True)}
    dc = DataConsistencyInKspace(None)

    def step():
        pred.grad = None
        out = dc(pred, k0, mask)
        losses = loss_functions.image_hypernetwork_ift_loss(
            None, 1e-1, 1e2, {"model_out": out, "latent_vec": latent, "hypo_params": hypo}, {"img": tgt})
        total = losses["img_loss"] + losses["latent_loss"] + losses["hypo_weight_loss"]
        total.backward()
        return losses["img_loss"].detach(), pred.grad

    return step


def launches(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kift_time: no GPU (a timing is taken on the device or not at all)")
    _native.load_library()
    dev = torch.device("cuda", 0)
    step = make_step(args.batch, args.side, dev)
    arms = {"native": True, "expression": False}
    result, count, times = {}, {}, {k: [] for k in arms}
    try:
        for name, native in arms.items():
            loss_functions.set_kspace_loss_native(native)
            for _ in range(args.warmup):
                step()
            loss, grad = step()
            result[name] = (loss.double().cpu(), grad.double().cpu().clone())
            count[name] = launches(step)
        for _ in range(args.reps):
            for name, native in arms.items():
                loss_functions.set_kspace_loss_native(native)
                step()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.inner):
                    step()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) / args.inner * 1e3)
    finally:
        loss_functions.set_kspace_loss_native(True)
    ln, gn = result["native"]
    le, ge = result["expression"]
    lines = [f"kift_time: image_hypernetwork_ift_loss forward + backward, DC'd [{args.batch}, {args.side ** 2}, 2], "
             f"{torch.cuda.get_device_name(0)}",
             f"  {args.reps} repetitions per arm, interleaved, {args.inner} steps each between device events, "
             f"{args.warmup} warm-up steps"]
    out = {"batch": args.batch, "side": args.side, "reps": args.reps, "inner": args.inner}
    for name in arms:
        t = sorted(times[name])
        med = statistics.median(t)
        out[name] = {"median_us": med, "min_us": t[0], "max_us": t[-1], "launches": count[name]}
        lines.append(f"  {name:<10} median {med:8.1f} us/step  (min {t[0]:.1f}, max {t[-1]:.1f}), "
                     f"{count[name]} launches per step")
    out["speedup"] = out["expression"]["median_us"] / out["native"]["median_us"]
    out["loss_rel_diff"] = abs(float(ln) - float(le)) / abs(float(le))
    out["grad_norm_rel_diff"] = (torch.linalg.vector_norm(gn - ge) / torch.linalg.vector_norm(ge)).item()
    lines.append(f"  expression / native = {out['speedup']:.2f}x; native against expression: loss rel diff "
                 f"{out['loss_rel_diff']:.2e}, grad norm-rel diff {out['grad_norm_rel_diff']:.2e}")
    lines.append(json.dumps(out))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
