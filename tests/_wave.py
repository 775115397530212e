"""What the wave-equation tests share (a plain helper module, imported by name after tests/ is put on
sys.path, as _sdf.py is): the fixture, the loss as a float64 formula, and seeded operands."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("dirichlet", "neumann", "diff_constraint_hom")
C = (1.0, 2.0, 3.0)  # the upstream weights the fixture's gradients were recorded with
MARGIN = 1e-3        # every row that is not planted keeps |pred - src|, |u_t| and |e| above it
OPERANDS = ("pred", "jac", "hess", "src", "slow", "mask")


def load_golden():
    return np.load(os.path.join(G, "wave.npz"), allow_pickle=False)


def formula64(pred, jac, hess, src, slow, mask):
    """The three terms [3] in float64 torch: pred, src, slow, mask [B, N, 1]; jac [B, N, 1, 3]; hess
    [B, N, 1, 3, 3] or None (term 2 is then 0). N = pred.shape[1], the reference's batch_size. An unmasked
    row's src is replaced before use, so nothing of it (NaN included) reaches a term or a gradient."""
    pred, jac, slow = pred.double(), jac.double(), slow.double()
    n = pred.shape[1]
    zero = torch.zeros_like(pred)
    clean = torch.where(mask, src.double(), zero)
    dirichlet = torch.where(mask, (pred - clean).abs(), zero).sum() * n / 1e1
    neumann = torch.where(mask, jac[..., 0].abs(), zero).sum() * n / 1e2
    if hess is None:
        hom = torch.zeros((), dtype=torch.float64)
    else:
        h = hess.double()
        hom = (h[..., 0, 0] - 1 / slow * (h[..., 1, 1] + h[..., 2, 2])).abs().sum()
    return torch.stack([dirichlet, neumann, hom])


def formula64_grads(pred, jac, hess, src, slow, mask, g):
    """(terms [3], d(sum_k g_k term_k)/dpred, .../djac, .../dhess or None) of formula64 by float64 autograd."""
    p, j = pred.double().clone().requires_grad_(True), jac.double().clone().requires_grad_(True)
    h = hess.double().clone().requires_grad_(True) if hess is not None else None
    terms = formula64(p, j, h, src, slow, mask)
    (terms * torch.as_tensor(g, dtype=torch.float64)).sum().backward()
    return terms.detach(), p.grad, j.grad, (h.grad if h is not None else None)


def operands(batch, n, seed, mask="mixed"):
    """Seeded operands [batch, n, .]: (pred, jac, hess, src, slow, mask), float32 and bool. mask: 'mixed'
    (the first half of each batch element, rounded up, is masked), 'none' or 'all'. slow is 1 or 0.25.
    Every row keeps |pred - src|, |u_t| and |e| = |u_tt - lap / slow| above 0.01 in float32 and float64
    alike, except the planted rows, flat rows 0..2 when there are that many: pred == src, u_t == 0 and
    e == 0 exactly (with 'mixed' and 'all' these rows are masked). Unmasked rows carry src = 7, which no
    term reads."""
    g = torch.Generator().manual_seed(seed)
    rows = batch * n
    m = torch.zeros(batch, n, dtype=torch.bool)
    if mask == "mixed":
        m[:, : (n + 1) // 2] = True
    elif mask == "all":
        m[:] = True
    else:
        assert mask == "none", mask
    m = m.reshape(rows)

    def away(k):  # [k] values with magnitude in [0.01, ...), either sign
        sign = torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
        return sign * (0.01 + torch.randn(k, generator=g).abs())

    src = torch.rand(rows, generator=g)
    pred = src + away(rows)
    jac = torch.randn(rows, 3, generator=g)
    jac[:, 0] = away(rows)
    slow = torch.where(torch.rand(rows, generator=g) < 0.5, 1.0, 0.25)
    hess = torch.randn(rows, 3, 3, generator=g)
    # multiples of 1/64 below 4: lap / slow and h00 = lap / slow + e are then exact in float32 for e on the same grid
    hess[:, 1, 1] = torch.round(hess[:, 1, 1].clamp(-3, 3) * 64) / 64
    hess[:, 2, 2] = torch.round(hess[:, 2, 2].clamp(-3, 3) * 64) / 64
    e = torch.round(away(rows).clamp(-3, 3) * 64) / 64
    e = torch.where(e.abs() < 1 / 64, torch.full_like(e, 1 / 64), e)
    hess[:, 0, 0] = (hess[:, 1, 1] + hess[:, 2, 2]) / slow + e
    if rows >= 3:
        pred[0] = src[0]
        jac[1, 0] = 0.0
        hess[2, 0, 0] = (hess[2, 1, 1] + hess[2, 2, 2]) / slow[2]
    src = torch.where(m, src, torch.full_like(src, 7.0))
    return (pred.view(batch, n, 1), jac.view(batch, n, 1, 3), hess.view(batch, n, 1, 3, 3), src.view(batch, n, 1),
            slow.view(batch, n, 1), m.view(batch, n, 1))


def golden_operands(d):
    """The fixture's synthetic operand set (R = 514 as [2, 257, .]) in the order of OPERANDS."""
    return tuple(torch.from_numpy(d["op/" + k]) for k in OPERANDS)


def golden_model(d, precision=None, device=None):
    """The fixture's end-to-end model (3-64-64-64-1) with its recorded initial parameters."""
    from siren_mri_amd import modules
    kw = {} if precision is None else {"precision": precision}
    m = modules.SingleBVPNet(type="sine", in_features=3, hidden_features=64, num_hidden_layers=2, **kw)
    m.load_state_dict({k[len("e2e/init/"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("e2e/init/")})
    return m if device is None else m.to(device)


def golden_item(d, mode, item):
    """({'coords'}, gt) of the reference's WaveSource(sidelength=48) item `item` (0 or 1) in `mode` ('pre',
    'train'), without a batch dimension."""
    p = f"ws/{mode}/{item}/"
    return ({"coords": torch.from_numpy(d[p + "coords"])},
            {"source_boundary_values": torch.from_numpy(d[p + "src"]), "dirichlet_mask": torch.from_numpy(d[p + "mask"]),
             "squared_slowness": torch.from_numpy(d[p + "slow"])})


def golden_batch(d, device=None, mode="train"):
    """The fixture's end-to-end batch [1, 2304, .]: item 1 of the training mode (a mixed mask; item 0's
    time window is empty, so its mask is all true), or of the pretraining mode (an all-true mask)."""
    inp, gt = golden_item(d, mode, 1)
    inp = {k: v[None] for k, v in inp.items()}
    gt = {k: v[None] for k, v in gt.items()}
    if device is not None:
        inp = {k: v.to(device) for k, v in inp.items()}
        gt = {k: v.to(device) for k, v in gt.items()}
    return inp, gt
