"""Bits of every loss that ends in an inter-workgroup hand-off of a deterministic sum, recorded at one
commit and compared at later ones (tests/test_gpu_loss_bits.py): per case the loss as a float32 hex
string and the SHA-256 of the gradient's bytes (the fused forward losses: of dL/dy and DC(y)).

    python tests/golden/make_golden_loss_bits.py [out.json]   # on the MI355X; default tests/golden/loss_bits.json

The file names the commit it was recorded at (git's HEAD, or LOSS_BITS_COMMIT where the tree has no .git).
The shapes are the smallest that reach each branch of the hand-off: one workgroup, a few, and more
workgroups than the last workgroup has threads. Inputs come from seeded CPU generators. Every case is
run twice in a row with fresh output tensors and both runs must agree (the second one shows that the
first re-armed the hand-off's counter). Only calls the package has had since the losses were added.
"""
import hashlib
import json
import os
import struct
import subprocess
import sys

import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
OUT = os.path.join(GOLDEN, "loss_bits.json")

KINDS = {"asinh": "image_asinh", "cubic": "image_mse_cubic", "smape": "image_smape", "l1": "kspace_l1",
         "perp": "image_perp", "log": "image_mse_log"}
SSE_SIZES = (1000, 3 * 4096 + 5, 256 * 4096 + 4097)    # 1, 4, 258 workgroups of 16 x 256 elements
KSPACE_SHAPES = ((1, 64, 2), (3, 1024, 2), (33, 16384, 2))  # 1, 2, 264 workgroups of 8 x 256 coordinates
IFT_CASES = ((1, 8), (3, 8), (3, 32), (300, 8))        # one workgroup per slice; 64 threads at side 8
DC_NOISE = {"nodc": None, "dc": 0.0, "dcnoise": 0.25}
STACK = [2, 256, 256, 256, 1]                          # tests/test_gpu_fused_loss.py's _net()
# (precision, weight sets, rows per set): the register forward's grid is min(ceil(rows / 256),
# max(1, 256 / sets)) x sets, the per-layer output kernel's min(ceil(rows / 8), max(1, 1024 / sets)) x sets
FUSED_CASES = {"fused_reg_wg2": ("bf16", 0, 300), "fused_reg_wg520": ("bf16", 520, 8),
               "fused_last_wg300": ("fp32", 0, 2400)}


def dev():
    return torch.device("cuda:0")


def f32_hex(t):
    return struct.pack(">f", float(t.detach().reshape(()).cpu())).hex()


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


_INPUTS = {}


def kspace_inputs(shape):
    """pred, tgt [B, N, C], k0 and mask [B, C, side, side] of a shape, on the device (made once)."""
    hit = _INPUTS.get(shape)
    if hit is None:
        b, n, c = shape
        side = int(round(n ** 0.5))
        g = torch.Generator().manual_seed(1000 * b + n)
        pred = torch.randn(b, n, c, generator=g)
        tgt = torch.randn(b, n, c, generator=g)
        pred[:, ::7] = tgt[:, ::7]  # ties: the zero cases of the family
        k0 = torch.randn(b, c, side, side, generator=g)
        mask = (torch.rand(b, c, side, side, generator=g) < 0.3).float()
        hit = _INPUTS[shape] = tuple(t.to(dev()) for t in (pred, tgt, mask * k0, mask))
    return hit


def dc_output(pred, k0, mask, noise):
    """pred, or the native DataConsistencyInKspace's output of it (which the losses fold in)."""
    from siren_mri_amd.data_consistency import DataConsistencyInKspace
    if noise is None:
        return pred
    return DataConsistencyInKspace(noise_lvl=noise or None)(pred, k0, mask)


def loss_and_grad(fn, pred):
    p = pred.clone().requires_grad_(True)
    loss = fn(p)
    loss.backward()
    return {"loss": f32_hex(loss), "grad": sha(p.grad)}


def run_sse(n, masked):
    from siren_mri_amd import loss_functions
    g = torch.Generator().manual_seed(n)
    pred, tgt = torch.randn(n, generator=g).to(dev()), torch.randn(n, generator=g).to(dev())
    mask = (torch.rand(4, generator=g) + 0.5).to(dev()) if masked else None  # element e takes m[e % 4]
    return loss_and_grad(lambda p: loss_functions.weighted_sse(p, tgt, mask=mask), pred)


def run_image_mse(shape, dc):
    from siren_mri_amd import loss_functions
    pred, tgt, k0, mask = kspace_inputs(shape)
    return loss_and_grad(lambda p: loss_functions.image_mse(
        None, {"model_out": dc_output(p, k0, mask, DC_NOISE[dc])}, {"img": tgt})["img_loss"], pred)


def run_kloss(kind, shape, dc):
    from siren_mri_amd import loss_functions
    pred, tgt, k0, mask = kspace_inputs(shape)
    fn = getattr(loss_functions, KINDS[kind])
    return loss_and_grad(lambda p: fn(None, {"model_out": dc_output(p, k0, mask, DC_NOISE[dc])}, {"img": tgt})["img_loss"],
                         pred)


def run_ift(batch, side, masked_dc):
    from siren_mri_amd import loss_functions
    pred, tgt, k0, mask = kspace_inputs((batch, side * side, 2))
    img_mask = None
    if masked_dc:
        img_mask = (torch.rand(batch, side, side, generator=torch.Generator().manual_seed(side)) < 0.6).float().to(dev())
    return loss_and_grad(lambda p: loss_functions.ift_image_mse(
        img_mask, {"model_out": dc_output(p, k0, mask, 0.25 if masked_dc else None)}, {"img": tgt})["img_loss"], pred)


def fused_grid(name):
    prec, sets, rows = FUSED_CASES[name]
    nb = max(sets, 1)
    per = min(-(-rows // 256), max(1, 256 // nb)) if prec == "bf16" else min(-(-rows // 8), max(1, 1024 // nb))
    return per * nb


def fused_inputs(name):
    hit = _INPUTS.get(name)
    if hit is None:
        from oracle import siren_oracle as orc
        prec, sets, rows = FUSED_CASES[name]
        nb = max(sets, 1)
        g = torch.Generator().manual_seed(rows + sets)
        lead = (sets,) if sets else ()
        ws, bs = [], []
        for W, b in orc.siren_init(STACK, seed=3):
            # per-set weights: the initialisation, scaled a little differently for every set
            ws.append((W * (1 + 0.05 * torch.rand(lead + (1, 1), generator=g))).contiguous().to(dev()))
            bs.append((b * (1 + 0.05 * torch.rand(lead + (1,), generator=g))).contiguous().to(dev()))
        x = (torch.rand(nb, rows, 2, generator=g) * 2 - 1).to(dev())
        tgt = torch.randn(nb, rows, 1, generator=g).to(dev())
        k0 = torch.randn(nb, 1, rows, 1, generator=g)
        mask = (torch.rand(nb, 1, rows, 1, generator=g) < 0.3).float()
        hit = _INPUTS[name] = (x, ws, bs, tgt, (mask * k0).to(dev()), mask.to(dev()))
    return hit


def run_fused(name):
    from siren_mri_amd import _native
    import siren_mri_amd.ops  # noqa: F401  (registers the op)
    prec, sets, rows = FUSED_CASES[name]
    x, ws, bs, tgt, k0, mask = fused_inputs(name)
    y, y_dc, loss, dy, _ = torch.ops.siren_mri_amd.sine_mlp_fwd_loss(
        x, ws, bs, 30.0, _native.precision_code(prec), bool(sets), tgt, k0, mask, None, 0.25, 1.0 / (128 * 128))
    return {"loss": f32_hex(loss), "dy": sha(dy), "y_dc": sha(y_dc)}


def cases():
    """name -> a function that runs the case once and returns its record."""
    out = {}
    for n in SSE_SIZES:
        for masked in (False, True):
            out[f"sse_n{n}_{'masked' if masked else 'plain'}"] = lambda n=n, masked=masked: run_sse(n, masked)
    for shape in KSPACE_SHAPES:
        tag = "x".join(map(str, shape))
        for dc in DC_NOISE:
            out[f"image_mse_{tag}_{dc}"] = lambda shape=shape, dc=dc: run_image_mse(shape, dc)
        for kind in KINDS:
            for dc in ("nodc", "dcnoise"):
                out[f"kloss_{kind}_{tag}_{dc}"] = lambda kind=kind, shape=shape, dc=dc: run_kloss(kind, shape, dc)
    for batch, side in IFT_CASES:
        out[f"ift_b{batch}_side{side}"] = lambda batch=batch, side=side: run_ift(batch, side, False)
    out["ift_b3_side32_masked_dc"] = lambda: run_ift(3, 32, True)
    for name in FUSED_CASES:
        out[name] = lambda name=name: run_fused(name)
    return out


def main():
    sys.path.insert(0, ROOT)
    for name in FUSED_CASES:
        print(f"{name}: {fused_grid(name)} workgroups")
    for n in SSE_SIZES:
        print(f"sse n={n}: {min(1024, -(-n // 4096))} workgroups")
    for b, n, _ in KSPACE_SHAPES:
        print(f"kspace [{b}, {n}]: {min(1024, -(-b * n // 2048))} workgroups")
    for b, side in IFT_CASES:
        print(f"ift side {side}: {b} workgroups of {min(side * side, 1024)} threads")
    rec = {}
    for name, fn in cases().items():
        first, second = fn(), fn()
        if first != second:
            raise SystemExit(f"{name}: two runs in a row differ: {first} / {second}")
        rec[name] = first
        print(name, first["loss"])
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    out = {"commit": os.environ.get("LOSS_BITS_COMMIT") or commit, "cases": rec}
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(rec)} cases")


if __name__ == "__main__":
    main()
