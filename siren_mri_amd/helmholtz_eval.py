"""Dense evaluation of a fitted Helmholtz model and its comparison with the closed-form solution, which
the reference's summary plots start from (the counterpart of wave_eval.wave_field).

helmholtz_field(model, sidelength, chunk)   the complex field u = y[..., 0] + i y[..., 1] on the
    sidelength^2 grid of [-1, 1]^2 as an [S, S] complex64 CPU tensor: field[i0, i1] is the model at
    (-1 + 2 i0 / (S - 1), -1 + 2 i1 / (S - 1)), the order of dataio.get_mgrid(S). Runs under no_grad
    through the model's own forward (the native stack on a GPU) in chunks of `chunk` rows, each moved to
    the model's device.
relative_error(field, reference)   ||field - reference|| / ||reference|| over the grid points outside the
    perfectly matched layer (|x0|, |x1| <= 0.5): inside the layer the fitted field is damped and the
    closed form is not, so only there are the two comparable. reference: [S, S] complex, or the [S^2, 2]
    real / imaginary columns of dataio.SingleHelmholtzSource.field.
"""
from __future__ import annotations

import torch

from .dataio import get_mgrid


def helmholtz_field(model, sidelength, chunk=128 ** 2):
    """[S, S] complex64 CPU tensor of the model's output on get_mgrid(sidelength)."""
    dev = next(model.parameters()).device
    rows = get_mgrid(sidelength)
    out = torch.empty(rows.shape[0], 2, dtype=torch.float32)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for head in range(0, rows.shape[0], chunk):
                part = rows[head:head + chunk].to(dev)
                y = model({"coords": part[None]})["model_out"]
                out[head:head + part.shape[0]] = y.reshape(-1, 2).float().cpu()
    finally:
        model.train(was_training)
    return torch.complex(out[:, 0], out[:, 1]).view(sidelength, sidelength)


def _as_complex_grid(t, sidelength):
    if torch.is_complex(t):
        return t.reshape(sidelength, sidelength).to(torch.complex128)
    t = t.reshape(sidelength * sidelength, 2).double()
    return torch.complex(t[:, 0], t[:, 1]).view(sidelength, sidelength)


def relative_error(field, reference):
    """Norm-relative difference of two fields on the same grid over |x0|, |x1| <= 0.5, as a float."""
    side = field.shape[0]
    a, b = _as_complex_grid(field.cpu(), side), _as_complex_grid(reference.cpu(), side)
    grid = get_mgrid(side).view(side, side, 2)
    inner = (grid[..., 0].abs() <= 0.5) & (grid[..., 1].abs() <= 0.5)
    den = torch.linalg.vector_norm(b[inner]).item()
    return torch.linalg.vector_norm(a[inner] - b[inner]).item() / (den if den > 0 else 1.0)
