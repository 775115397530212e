"""Golden vectors of the k-space loss family from the REAL reference (run in the build container
only, on the CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kspace_losses.py

  kspace_losses.npz  image_mse_log, image_mse_cubic, image_smape, image_asinh, image_perp, kspace_l1,
                     ift_image_mse and image_l1 (loss_functions.py:12-64, 103-235; mask None) on one
                     k-space-like input: B = 2 images of 16x16 complex pixels (C = 2), every value an
                     fp32 number, a per-pixel amplitude 0.5 exp(-3 u) (a dynamic range of e^3) times
                     independent normal deviates for the prediction and the target. Planted per image,
                     at the pixel indices stored with them:
                       tie_idx       16 pixels with pred == tgt
                       pred0_idx      8 pixels with pred == 0 in both channels
                       tgt0_idx       8 pixels with tgt == 0 in both channels
                       both0_idx      4 pixels with both zero
                       chan0_idx      4 pixels with one channel of pred zero (channel 0, 1, 0, 1)
                     Per loss NAME: NAME_loss64 and NAME_grad64 (the reference run on the float64
                     copies: loss and dL/dpred), NAME_loss32 (run on the float32 values), and the
                     reference's own float32-against-float64 errors NAME_ref32_loss_rel (relative) and
                     NAME_ref32_grad_normrel (|g32 - g64| / |g64|, the oracle's norm_rel).
The generator asserts what the tests rely on: every gradient is finite; for the six k-space kinds a
pixel with pred == tgt (the ties and the both-zero pixels) has a gradient of exactly 0, and so has a
pixel with pred == 0 for the kinds whose derivative vanishes there under torch's conventions (log:
|.| and angle at 0; perp: |.| at 0 and sign(0) = 0; cubic: sign(0) = 0). For asinh, smape and L1 the
derivative at pred == 0 != tgt is not zero, in the reference as in calculus.
Only data leaves the reference: no source is copied.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference, quiet  # noqa: E402

NAMES = ("image_mse_log", "image_mse_cubic", "image_smape", "image_asinh", "image_perp", "kspace_l1",
         "ift_image_mse", "image_l1")
KSPACE = NAMES[:6]
ZERO_AT_PRED0 = ("image_mse_log", "image_perp", "image_mse_cubic")
B, SIDE, C, SEED = 2, 16, 2, 20
PLANTED = (("tie_idx", 16), ("pred0_idx", 8), ("tgt0_idx", 8), ("both0_idx", 4), ("chan0_idx", 4))


def make_inputs(batch=B, side=SIDE, channels=C, seed=SEED):
    """(pred, tgt) float32 [batch, side^2, channels] and the planted pixel indices {name: [batch, k]}."""
    g = torch.Generator().manual_seed(seed)
    n = side * side
    amp = 0.5 * torch.exp(-3.0 * torch.rand(batch, n, 1, generator=g, dtype=torch.float64))
    pred = (amp * torch.randn(batch, n, channels, generator=g, dtype=torch.float64)).to(torch.float32)
    tgt = (amp * torch.randn(batch, n, channels, generator=g, dtype=torch.float64)).to(torch.float32)
    idx = {k: [] for k, _ in PLANTED}
    for b in range(batch):
        perm = torch.randperm(n, generator=g)
        at = 0
        for k, cnt in PLANTED:
            idx[k].append(perm[at:at + cnt].clone())
            at += cnt
        pred[b, idx["tie_idx"][b]] = tgt[b, idx["tie_idx"][b]]
        pred[b, idx["pred0_idx"][b]] = 0.0
        tgt[b, idx["tgt0_idx"][b]] = 0.0
        pred[b, idx["both0_idx"][b]] = 0.0
        tgt[b, idx["both0_idx"][b]] = 0.0
        for j, p in enumerate(idx["chan0_idx"][b].tolist()):
            pred[b, p, j % channels] = 0.0
    return pred, tgt, {k: torch.stack(v) for k, v in idx.items()}


def run(fn, pred, tgt):
    p = pred.clone().requires_grad_(True)
    loss = quiet(fn, None, {"model_out": p}, {"img": tgt})["img_loss"]
    loss.backward()
    return loss.detach(), p.grad.detach()


def norm_rel(a, b):
    den = torch.linalg.vector_norm(b.double()).item()
    return torch.linalg.vector_norm(a.double() - b.double()).item() / (den if den > 0 else 1.0)


def main():
    R = import_reference()
    pred, tgt, idx = make_inputs()
    out = {"pred": pred.numpy(), "tgt": tgt.numpy(), "seed": np.array(SEED)}
    out.update({k: v.numpy() for k, v in idx.items()})
    rows = torch.arange(B)[:, None]
    for name in NAMES:
        fn = getattr(R.loss_functions, name)
        l64, g64 = run(fn, pred.double(), tgt.double())
        l32, g32 = run(fn, pred, tgt)
        assert torch.isfinite(g64).all() and torch.isfinite(g32).all() and torch.isfinite(l64) and torch.isfinite(l32), name
        if name in KSPACE:
            zero = [idx["tie_idx"], idx["both0_idx"]] + ([idx["pred0_idx"]] if name in ZERO_AT_PRED0 else [])
            for z in zero:
                assert (g64[rows, z] == 0).all() and (g32[rows, z] == 0).all(), name
        out[name + "_loss64"] = l64.numpy()
        out[name + "_grad64"] = g64.numpy()
        out[name + "_loss32"] = l32.numpy()
        out[name + "_ref32_loss_rel"] = np.array(abs(l32.double().item() - l64.item()) / abs(l64.item()))
        out[name + "_ref32_grad_normrel"] = np.array(norm_rel(g32, g64))
        print(f"{name:16s} loss64 {l64.item():.9e}  ref32 loss rel {out[name + '_ref32_loss_rel']:.2e}  "
              f"grad norm-rel {out[name + '_ref32_grad_normrel']:.2e}")
    path = os.path.join(OUT, "kspace_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote kspace_losses.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
