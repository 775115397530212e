"""Dense evaluation of a fitted wave-equation model: the field at one time on the spatial grid, which
the reference's summary plots start from (the counterpart of sdf_meshing.sdf_volume).

wave_field(model, t, N, max_batch)   u(t, ., .) on the N^2 grid of [-1, 1]^2 as an [N, N] float32 CPU
    tensor: field[i0, i1] is the model at (t, -1 + 2 i0 / (N - 1), -1 + 2 i1 / (N - 1)), the order of
    dataio.get_mgrid(N). Runs under no_grad through the model's own forward (the native stack on a
    GPU) in chunks of max_batch rows, each moved to the model's device.
"""
from __future__ import annotations

import torch

from .dataio import get_mgrid


def wave_field(model, t, N=256, max_batch=128 ** 2):
    """[N, N] float32 CPU tensor of the model's output at time t on get_mgrid(N)."""
    dev = next(model.parameters()).device
    grid = get_mgrid(N)
    rows = torch.cat((torch.full((grid.shape[0], 1), float(t)), grid), dim=1)
    out = torch.empty(rows.shape[0], dtype=torch.float32)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for head in range(0, rows.shape[0], max_batch):
                chunk = rows[head:head + max_batch].to(dev)
                y = model({"coords": chunk[None]})["model_out"]
                out[head:head + chunk.shape[0]] = y.reshape(-1).float().cpu()
    finally:
        model.train(was_training)
    return out.view(N, N)
