"""Writes priors.npz: the reference's image_mse_TV_prior, image_mse_FH_prior
(loss_functions.py:238-272) and diff_operators.hessian (diff_operators.py:5-24) on the CPU, for a
2-64-64-1 SIREN on a 16^2 grid with fixed seeds. Only data goes in:

  init/<name>        the model's state_dict
  coords             the grid [1, 256, 2]
  img, mask          ground truth [1, 256, 1] and inpainting mask [256, 1]
  coords_rand        the priors' random coordinates [1, 128, 2] (torch.manual_seed(SEED_RAND))
  hessian            hessian(model_out, model_in) on the grid [1, 256, 1, 2, 2]
  tv/<key>, fh/<key> the two loss dicts
  tv_grad/<name>, fh_grad/<name>  parameter gradients of the summed loss dict

Run from the repository root: python tests/golden/make_golden_priors.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference  # noqa: E402

SEED_INIT, SEED_DATA, SEED_RAND, SIDE, K1 = 0, 1, 2, 16, 0.5


def main():
    ref = import_reference()
    torch.manual_seed(SEED_INIT)
    model = ref.modules.SingleBVPNet(type="sine", mode="mlp", sidelength=(SIDE, SIDE), hidden_features=64,
                                     num_hidden_layers=1)
    out = {"init/" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    coords = ref.dataio.get_mgrid(SIDE)[None]
    g = torch.Generator().manual_seed(SEED_DATA)
    img = torch.randn(1, SIDE * SIDE, 1, generator=g)
    mask = (torch.rand(SIDE * SIDE, 1, generator=g) < 0.5).float()
    out.update(coords=coords.numpy(), img=img.numpy(), mask=mask.numpy())
    torch.manual_seed(SEED_RAND)
    out["coords_rand"] = (2 * (torch.rand((1, SIDE * SIDE // 2, 2)) - 0.5)).numpy()

    o = model({"coords": coords})
    h, status = ref.diff_operators.hessian(o["model_out"], o["model_in"])
    assert status == 0
    out["hessian"] = h.detach().numpy()

    for tag, fn in (("tv", ref.loss_functions.image_mse_TV_prior), ("fh", ref.loss_functions.image_mse_FH_prior)):
        model.zero_grad()
        o = model({"coords": coords})
        torch.manual_seed(SEED_RAND)
        losses = fn(mask, K1, model, o, {"img": img})
        sum(losses.values()).backward()
        for k, v in losses.items():
            out[f"{tag}/{k}"] = v.detach().numpy()
        for k, p in model.named_parameters():
            out[f"{tag}_grad/{k}"] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "priors.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
