"""Losses on the SIREN hot path (drop-in for loss_functions.py of jonbmartin/siren_mri).

  image_mse                loss_functions.py:66-101
  latent_loss              loss_functions.py:275-276
  hypo_weight_loss         loss_functions.py:279-287
  image_hypernetwork_loss  loss_functions.py:290-293
  image_mse_log, image_mse_cubic, image_smape, image_asinh, image_perp, kspace_l1
                           loss_functions.py:12-64, 103-190 (the k-space loss family)
  ift_image_mse, image_l1  loss_functions.py:192-235
  image_mse_TV_prior, image_mse_FH_prior  loss_functions.py:238-272 (the inpainting priors: the
                           analytic gradient / Hessian at random coordinates)
  image_hypernetwork_{perp,asinh,l1,log,cubic,ift}_loss  loss_functions.py:295-323
  function_mse             loss_functions.py:326-327
  gradients_mse            loss_functions.py:330-335
  laplace_mse              loss_functions.py:350-355
  sdf                      loss_functions.py:460-484 (signed-distance fitting: four terms on the
                           output and its analytic gradient; siren_mri_amd::sdf_loss, siren_sdf.hip)
  wave_pml                 loss_functions.py:358-382 (wave-equation fitting: three terms on the output,
                           its analytic Jacobian and Hessian; siren_mri_amd::wave_loss, siren_wave.hip)
  helmholtz_pml            loss_functions.py:385-457, the forward problem (Helmholtz fitting with a perfectly
                           matched layer: two sums on the complex output, its analytic Jacobian and
                           Hessian; siren_mri_amd::helmholtz_loss, siren_helmholtz.hip)

image_mse runs on the native k-space op (siren_kspace.hip), with the data consistency of a native
DataConsistencyInKspace output folded in. The six k-space losses of the
family run on siren_mri_amd::kspace_loss (siren_kloss.hip: one forward and one backward launch, the
DC folded in the same way); ift_image_mse runs on siren_mri_amd::kspace_ift_loss (siren_kfft.hip: the
two ifft2 and the three sums in one forward launch, one backward launch) for square slices of side
8 to 128, and is a PyTorch composition otherwise, as image_l1 is. This module holds the reference's
expressions, the switches and the decision which native op applies; the ops themselves and the
autograd functions on the kernels are bound in loss_ops.py.

Deliberate deviation (bug 0.2): the reference builds its high-frequency mask
on a fixed 128x128 grid, so image_mse(high_freq=True) raises for any other image size; here the
mask applies when the image is 128x128 and the loss is the plain SSE otherwise.

Deliberate deviation: image_mse_log does not print its two partial sums on every call
(loss_functions.py:37); that print forces a host synchronisation per step.

Deliberate deviation (in the style of bug 0.4): the two priors draw their random coordinates with
torch.rand(shape) on the CPU default generator, as the reference does, and then move them to
model_in's device instead of calling `.cuda()`: the random stream is the reference's, and the
losses run on a CPU device too.
"""
from __future__ import annotations

import torch

from . import _native, diff_operators, fusion
from .data_consistency import dc_source
from .dataio import lin2img
# the native kernels' autograd functions and custom ops (importing it registers the ops)
from .loss_ops import _kfft_side, _kift_max_batch, _SumSquares, _WeightedSSE  # noqa: F401
from .utils import create_circular_mask_torch

_KSPACE_WEIGHT = 1.0 / (128 * 128)
KSPACE_WEIGHT = _KSPACE_WEIGHT  # image_mse's normalisation (loss_functions.py:101)
_MASKS: dict = {}


def _high_freq_mask(device):
    m = _MASKS.get(device)
    if m is None:
        # float32 (the reference's mask is int64; 1 - mask promotes the product with pred to float
        # either way), so the native weighted-SSE kernel takes it
        m = (1 - create_circular_mask_torch(129, 129, center=None, radius=20)).to(torch.float32)
        m = m.to(device)
        _MASKS[device] = m
    return m


_FUSE_DC = True


def set_kspace_fusion(enabled: bool) -> None:
    """Fold a native DataConsistencyInKspace output's DC into image_mse's loss op (default on)."""
    global _FUSE_DC
    _FUSE_DC = bool(enabled)


def high_freq_flat(device):
    """image_mse's 128x128 high-frequency mask, flattened to the SIREN's [N] row order."""
    return _hf_flat(device)


def _staged_loss(out, tgt, hf_applied, weight):
    """The forward's fused loss (fusion.py) when `out` is its output (DC(y) with data consistency),
    `tgt` the staged target and the reduction the same; None otherwise."""
    st = fusion.staged(out.device)
    if st is None or st.result is None:
        return None
    y, y_dc, loss, st_hf, _dc = st.result
    if out is not (y_dc if y_dc is not None else y) or tgt is not st.tgt:
        return None
    if bool(hf_applied) != bool(st_hf) or float(weight) != st.weight:
        return None
    return loss


def _hf_flat(device):
    key = ("flat", device)
    m = _MASKS.get(key)
    if m is None:
        m = _high_freq_mask(device).reshape(-1).contiguous()
        _MASKS[key] = m
    return m


def _native_operands(out, tgt):
    """What every native k-space loss op takes: a float32 [B, N, C] prediction on the GPU and a target of
    its shape on its device that needs no gradient."""
    return (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and tgt.shape == out.shape
            and tgt.dtype == torch.float32 and tgt.device == out.device and not tgt.requires_grad)


def _fold_dc(out):
    """(pred, k0, mask, noise) of a native DataConsistencyInKspace output, whose DC the loss ops then
    compute themselves; (out, None, None, 0.0) for anything else or with set_kspace_fusion(False)."""
    src = dc_source(out) if _FUSE_DC else None
    if src is not None and src[0].shape == out.shape:
        return src
    return out, None, None, 0.0


def _kspace_image_mse(out, tgt, high_freq):
    """image_mse on [B, N, C] (N a square): the native k-space op, or None when not applicable."""
    if not (_native_operands(out, tgt) and out.shape[-1] <= 8):
        return None
    n = out.shape[1]
    side = int(round(n ** 0.5))
    if side * side != n:
        return None
    hf = _hf_flat(out.device) if (high_freq and side == 128) else None
    pred, k0, mask, noise = _fold_dc(out)
    return torch.ops.siren_mri_amd.kspace_sse(pred, k0, mask, tgt, hf, noise, _KSPACE_WEIGHT)[0]


def weighted_sse(pred, tgt, weight=_KSPACE_WEIGHT, mask=None):
    """sum |m (pred - tgt)|^2 * weight over any shape (image_mse's reduction without the
    lin2img reshape): the loss of a coordinate shard of an image in a sharded fit, whose partial
    sums over the ranks' shards add up to image_mse of the whole image."""
    if mask is None:
        staged = _staged_loss(pred, tgt, False, weight)
        if staged is not None:
            return staged
    if pred.is_cuda and pred.dtype == torch.float32 and tgt.dtype == torch.float32 and not tgt.requires_grad:
        return _WeightedSSE.apply(pred, tgt.to(pred.device), mask, weight)
    diff = pred - tgt
    if mask is not None:
        diff = mask * diff
    return (diff.abs() ** 2).sum() * weight


def image_mse(mask, model_output, gt, high_freq=True):
    """Weighted k-space SSE: sum |m * (pred - gt)|^2 / 128^2 (a sum over the batch). On the GPU
    the native k-space op reads model_out / gt in their [B, N, C] layout (no lin2img copies); a
    model_out produced by the native DataConsistencyInKspace has the DC folded into the op."""
    out, tgt = model_output["model_out"], gt["img"]
    if out.dim() == 3:
        side = int(round(out.shape[1] ** 0.5))
        staged = _staged_loss(out, tgt, high_freq and side * side == out.shape[1] and side == 128, _KSPACE_WEIGHT)
        if staged is not None:
            return {"img_loss": staged}
    fused = _kspace_image_mse(model_output["model_out"], gt["img"], high_freq)
    if fused is not None:
        return {"img_loss": fused}
    pred = lin2img(model_output["model_out"])
    tgt = lin2img(gt["img"])
    hf = _high_freq_mask(pred.device) if (high_freq and pred.shape[-2:] == (128, 128)) else None
    if (pred.is_cuda and pred.dtype == torch.float32 and tgt.dtype == torch.float32 and not tgt.requires_grad
            and pred.shape == tgt.shape and tgt.device == pred.device
            and (hf is None or (hf.dtype == torch.float32 and pred.shape[-hf.dim():] == hf.shape))):
        return {"img_loss": _WeightedSSE.apply(pred, tgt, hf, _KSPACE_WEIGHT)}
    diff = pred - tgt
    if hf is not None:
        diff = hf * diff
    loss = (diff.abs() ** 2).sum() * _KSPACE_WEIGHT
    return {"img_loss": loss}


def latent_loss(model_output):
    return torch.mean(model_output["latent_vec"] ** 2)


def hypo_weight_loss(model_output):
    """loss_functions.py:279-287: the mean of the squared hypo-parameters; on CUDA fp32 the sum of
    squares is one native launch (and its gradient one more)."""
    ws = list(model_output["hypo_params"].values())
    total = sum(w.numel() for w in ws)
    if ws and 0 < len(ws) <= 32 and all(w.is_cuda and w.dtype == torch.float32 and w.device == ws[0].device
                                        for w in ws):
        return _SumSquares.apply(*ws) * (1 / total)
    weight_sum = 0
    for w in ws:
        weight_sum = weight_sum + torch.sum(w ** 2)
    return weight_sum * (1 / total)


def image_hypernetwork_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": image_mse(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


_KLOSS_NATIVE = True


def set_kspace_loss_native(enabled: bool) -> None:
    """Run the k-space loss family on the native op where it applies (default on); off: the
    reference's expression in PyTorch everywhere (A/B tests)."""
    global _KLOSS_NATIVE
    _KLOSS_NATIVE = bool(enabled)


def _kspace_loss_native(out, tgt, kind):
    """A loss of the family on [B, N, C] through the native op, or None when it does not apply."""
    if not (_KLOSS_NATIVE and _native_operands(out, tgt) and 1 <= out.shape[-1] <= 8):
        return None
    if kind in (_native.KLOSS_PERP, _native.KLOSS_LOG) and out.shape[-1] != 2:
        return None
    pred, k0, mask, noise = _fold_dc(out)
    return torch.ops.siren_mri_amd.kspace_loss(pred, k0, mask, tgt, kind, noise)


# ift_image_mse's constants (loss_functions.py:207-229): image SSE, 1e-8 sum |y|, 0.0025 k-space SSE
_IFT_WEIGHTS = (1.0, 1e-8, 0.0025)


def _ift_native_applies(mask, out, tgt):
    """Whether ift_image_mse of these operands runs on siren_mri_amd::kspace_ift_loss."""
    if not (_KLOSS_NATIVE and torch.is_tensor(out) and _native_operands(out, tgt) and out.shape[-1] == 2):
        return False
    b, side = out.shape[0], _kfft_side(out.shape[1])
    if side is None or not 1 <= b <= _kift_max_batch():
        return False
    return mask is None or (torch.is_tensor(mask) and mask.dtype == torch.float32 and mask.device == out.device
                            and not mask.requires_grad
                            and tuple(mask.shape) in ((side, side), (1, side, side), (b, side, side)))


def _ift_loss_native(mask, out, tgt):
    """ift_image_mse on [B, side^2, 2] through the native op, or None when it does not apply."""
    if not _ift_native_applies(mask, out, tgt):
        return None
    pred, k0, planes, noise = _fold_dc(out)
    return torch.ops.siren_mri_amd.kspace_ift_loss(pred, k0, planes, tgt, mask, noise, *_IFT_WEIGHTS)


def _complex_planes(t):
    """[B, N, 2] -> the complex [B, H, W] image of its two channels (loss_functions.py:15-16)."""
    real = lin2img(t)
    return real, real[:, 0, :, :] + 1j * real[:, 1, :, :]


def image_mse_log(mask, model_output, gt):
    """loss_functions.py:12-44: squared difference of log magnitudes plus 2 - cos of the phase
    difference, summed over the pixels (without the reference's per-call print of the two sums)."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_LOG)
    if fused is not None:
        return {"img_loss": fused}
    _, kspace_output = _complex_planes(model_output["model_out"])
    _, kspace_gt = _complex_planes(gt["img"])
    eps = 1e-3
    pred_log = torch.log(torch.abs(kspace_output) + eps)
    gt_log = torch.log(torch.abs(kspace_gt) + eps)
    mag_weight = 0.0001
    phase_weight = 0.0001
    loss = (mag_weight * (pred_log - gt_log) ** 2
            + phase_weight * (2 - torch.cos(torch.angle(kspace_output) - torch.angle(kspace_gt)))).sum()
    return {"img_loss": loss}


def image_mse_cubic(mask, model_output, gt):
    """loss_functions.py:46-64: SSE of the signed cube roots sign(x) (|x| + 1e-3)^(1/3), times 1e-6."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_CUBIC)
    if fused is not None:
        return {"img_loss": fused}
    pred, tgt = lin2img(model_output["model_out"]), lin2img(gt["img"])
    eps = 1e-3
    pred_tx = torch.sign(pred) * torch.pow(torch.abs(pred) + eps, 1 / 3)
    gt_tx = torch.sign(tgt) * torch.pow(torch.abs(tgt) + eps, 1 / 3)
    return {"img_loss": 0.000001 * ((pred_tx - gt_tx) ** 2).sum()}


def image_smape(mask, model_output, gt):
    """loss_functions.py:103-117: sum |p - t| / (1e-3 + |t| + |p|) / 128^2."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_SMAPE)
    if fused is not None:
        return {"img_loss": fused}
    pred, tgt = lin2img(model_output["model_out"]), lin2img(gt["img"])
    eps = 1e-3
    return {"img_loss": _KSPACE_WEIGHT * (torch.abs(pred - tgt) / (eps + torch.abs(tgt) + torch.abs(pred))).sum()}


def image_asinh(mask, model_output, gt):
    """loss_functions.py:119-141: SSE of asinh(400 x) / 6.7, over 128^2."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_ASINH)
    if fused is not None:
        return {"img_loss": fused}
    pred = torch.asinh(400 * lin2img(model_output["model_out"])) / 6.7
    tgt = torch.asinh(400 * lin2img(gt["img"])) / 6.7
    return {"img_loss": _KSPACE_WEIGHT * ((pred - tgt) ** 2).sum()}


def image_perp(mask, model_output, gt):
    """loss_functions.py:143-167: the component of the target perpendicular to the prediction,
    |Im(conj(p) t)| / (|p| + 1e-8), summed over the pixels, times 1000 / 128^2."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_PERP)
    if fused is not None:
        return {"img_loss": fused}
    _, kspace_pred = _complex_planes(model_output["model_out"])
    _, kspace_gt = _complex_planes(gt["img"])
    eps = 1e-8
    loss = torch.abs(torch.real(kspace_pred) * torch.imag(kspace_gt)
                     - torch.imag(kspace_pred) * torch.real(kspace_gt)) / (torch.abs(kspace_pred) + eps)
    return {"img_loss": 1 / (128 * 128) * 1000 * loss.sum()}


def kspace_l1(mask, model_output, gt):
    """loss_functions.py:169-190: sum |p - t| / 128^2 (the reference's sparsity term has weight 0)."""
    fused = _kspace_loss_native(model_output["model_out"], gt["img"], _native.KLOSS_L1)
    if fused is not None:
        return {"img_loss": fused}
    pred, tgt = lin2img(model_output["model_out"]), lin2img(gt["img"])
    return {"img_loss": _KSPACE_WEIGHT * torch.abs(pred - tgt).sum()}


def ift_image_mse(mask, model_output, gt):
    """loss_functions.py:192-229: SSE of the magnitude images (ifft2 of the complex k-space, with the
    optional mask), plus 1e-8 of the k-space magnitude sum, plus 0.0025 of the k-space SSE. On the
    GPU, [B, side^2, 2] float32 with side 8 to 128 runs on siren_mri_amd::kspace_ift_loss (both
    transforms and the three sums in one launch, the backward in one more, the data consistency of a
    native DataConsistencyInKspace output folded in); everything else on the expression below, with
    the native weighted SSE for its last term."""
    out, tgt = model_output["model_out"], gt["img"]
    fused = _ift_loss_native(mask, out, tgt)
    if fused is not None:
        return {"img_loss": fused}
    _, kspace_output = _complex_planes(out)
    _, kspace_gt = _complex_planes(tgt)
    img_output = torch.abs(torch.fft.ifft2(kspace_output))
    img_gt = torch.abs(torch.fft.ifft2(kspace_gt))
    l1_cost = 1e-8 * torch.abs(kspace_output).sum()
    kspace_loss = weighted_sse(out, tgt, weight=0.0025)
    img = (img_output - img_gt) ** 2
    if mask is not None:
        img = mask * img
    return {"img_loss": img.sum() + l1_cost + kspace_loss}


def image_l1(mask, model_output, gt):
    """loss_functions.py:231-235: mean |p - t|, with the optional mask."""
    diff = torch.abs(model_output["model_out"] - gt["img"])
    if mask is not None:
        diff = mask * diff
    return {"img_loss": diff.mean()}


def _prior_coords(model_in):
    """Half as many uniform random coordinates in [-1, 1) as model_in has rows
    (loss_functions.py:239-241, 256-258): drawn on the CPU default generator, then moved."""
    shape = (model_in.shape[0], model_in.shape[1] // 2, model_in.shape[2])
    return (2 * (torch.rand(shape) - 0.5)).to(model_in.device)


def _masked_image_mse(mask, model_output, gt):
    sq = (model_output["model_out"] - gt["img"]) ** 2
    if mask is not None:
        sq = mask * sq
    return sq.mean()


def image_mse_TV_prior(mask, k1, model, model_output, gt):
    """loss_functions.py:238-252: the masked image MSE plus k1 times the mean absolute gradient
    of the model at random coordinates (total variation)."""
    rand_output = model({"coords": _prior_coords(model_output["model_in"])})
    g = diff_operators.gradient(rand_output["model_out"], rand_output["model_in"])
    return {"img_loss": _masked_image_mse(mask, model_output, gt),
            "prior_loss": k1 * torch.abs(g).mean()}


def image_mse_FH_prior(mask, k1, model, model_output, gt):
    """loss_functions.py:255-272: the masked image MSE plus k1 times the mean Frobenius norm of
    the model's Hessian at random coordinates."""
    rand_output = model({"coords": _prior_coords(model_output["model_in"])})
    h, _ = diff_operators.hessian(rand_output["model_out"], rand_output["model_in"])
    h = h.view(*h.shape[0:2], -1)
    hessian_norm = h.norm(dim=-1, keepdim=True)
    return {"img_loss": _masked_image_mse(mask, model_output, gt),
            "prior_loss": k1 * torch.abs(hessian_norm).mean()}


def image_hypernetwork_perp_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": image_perp(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def image_hypernetwork_asinh_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": image_asinh(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def image_hypernetwork_l1_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": kspace_l1(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def image_hypernetwork_log_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": image_mse_log(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def image_hypernetwork_cubic_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": image_mse_cubic(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def image_hypernetwork_ift_loss(mask, kl, fw, model_output, gt):
    return {"img_loss": ift_image_mse(mask, model_output, gt)["img_loss"],
            "latent_loss": kl * latent_loss(model_output),
            "hypo_weight_loss": fw * hypo_weight_loss(model_output)}


def function_mse(model_output, gt):
    return {"func_loss": ((model_output["model_out"] - gt["func"]) ** 2).mean()}


def gradients_mse(model_output, gt):
    """mean_n sum_k (dy/dx_k - gt_k)^2 with the analytic SIREN gradient (config 3)."""
    g = diff_operators.gradient(model_output["model_out"], model_output["model_in"])
    return {"gradients_loss": torch.mean((g - gt["gradients"]).pow(2).sum(-1))}


def laplace_mse(model_output, gt):
    lap = diff_operators.laplace(model_output["model_out"], model_output["model_in"])
    return {"laplace_loss": torch.mean((lap - gt["laplace"]) ** 2)}


_SDF_NATIVE = True
_SDF_KEYS = ("sdf", "inter", "normal_constraint", "grad_constraint")


def set_sdf_loss_native(enabled: bool) -> None:
    """Run sdf on the native op where it applies (default on); off: the reference's expression in
    PyTorch everywhere (A/B tests)."""
    global _SDF_NATIVE
    _SDF_NATIVE = bool(enabled)


def _sdf_native_applies(pred, gradient, gt_sdf, gt_normals):
    """Whether sdf of these operands runs on siren_mri_amd::sdf_loss: float32 [B, N, 1] / [B, N, D] on
    one GPU, D 2 or 3, ground truth that needs no gradient."""
    if not (_SDF_NATIVE and pred.is_cuda and pred.dim() == 3 and pred.shape[-1] == 1 and gradient.dim() == 3
            and gradient.shape[-1] in (2, 3) and gradient.shape[:2] == pred.shape[:2]):
        return False
    if gt_sdf.shape != pred.shape or gt_normals.shape != gradient.shape:
        return False
    return all(t.dtype == torch.float32 and t.device == pred.device for t in (pred, gradient, gt_sdf, gt_normals)) \
        and not (gt_sdf.requires_grad or gt_normals.requires_grad)


def sdf(model_output, gt):
    """loss_functions.py:460-484: the four terms of signed-distance fitting on a batch of on-surface
    (gt sdf != -1) and off-surface (gt sdf == -1) points: |y| on the surface, exp(-1e2 |y|) off it,
    1 - cos(grad y, normal) on the surface, | |grad y| - 1 | everywhere, each a mean over all points
    times the reference's constant. On the GPU, a float32 one-channel output with 2 or 3 input
    dimensions runs on siren_mri_amd::sdf_loss (siren_sdf.hip: one forward and one backward launch
    behind diff_operators.gradient); everything else on the expression below."""
    gt_sdf = gt["sdf"]
    gt_normals = gt["normals"]
    coords = model_output["model_in"]
    pred_sdf = model_output["model_out"]

    gradient = diff_operators.gradient(pred_sdf, coords)

    if _sdf_native_applies(pred_sdf, gradient, gt_sdf, gt_normals):
        terms = torch.ops.siren_mri_amd.sdf_loss(pred_sdf, gradient, gt_sdf, gt_normals)
        # terms[0..3] through one unbind: its backward stacks the four upstream scalars in one launch
        return dict(zip(_SDF_KEYS, terms.unbind(0)))
    return _sdf_expression(pred_sdf, gradient, gt_sdf, gt_normals)


def _sdf_expression(pred_sdf, gradient, gt_sdf, gt_normals):
    """The reference's expression (loss_functions.py:474-484) in PyTorch ops, on any device and dtype."""
    on = gt_sdf != -1
    sdf_constraint = torch.where(on, pred_sdf, torch.zeros_like(pred_sdf))
    inter_constraint = torch.where(on, torch.zeros_like(pred_sdf), torch.exp(-1e2 * torch.abs(pred_sdf)))
    cos = torch.nn.functional.cosine_similarity(gradient, gt_normals, dim=-1)[..., None]
    normal_constraint = torch.where(on, 1 - cos, torch.zeros_like(gradient[..., :1]))
    grad_constraint = torch.abs(gradient.norm(dim=-1) - 1)
    return {"sdf": torch.abs(sdf_constraint).mean() * 3e3,
            "inter": inter_constraint.mean() * 1e2,
            "normal_constraint": normal_constraint.mean() * 1e2,
            "grad_constraint": grad_constraint.mean() * 5e1}


_WAVE_NATIVE = True
_WAVE_KEYS = ("dirichlet", "neumann", "diff_constraint_hom")


def set_wave_loss_native(enabled: bool) -> None:
    """Run wave_pml on the native op where it applies (default on); off: the reference's expression in
    PyTorch everywhere (A/B tests)."""
    global _WAVE_NATIVE
    _WAVE_NATIVE = bool(enabled)


def _wave_native_applies(pred, du, hess, src, slowness, mask):
    """Whether wave_pml of these operands runs on siren_mri_amd::wave_loss: float32 [B, N, 1] with its
    [B, N, 1, 3] Jacobian (and [B, N, 1, 3, 3] Hessian, or None) on one GPU, a bool mask, ground truth
    that needs no gradient."""
    if not (_WAVE_NATIVE and pred.is_cuda and pred.dim() == 3 and pred.shape[-1] == 1
            and tuple(du.shape) == (*pred.shape, 3) and (hess is None or tuple(hess.shape) == (*pred.shape, 3, 3))):
        return False
    if not (src.shape == pred.shape and slowness.shape == pred.shape and mask.shape == pred.shape):
        return False
    floats = [t for t in (pred, du, hess, src, slowness) if t is not None]
    return all(t.dtype == torch.float32 and t.device == pred.device for t in floats) \
        and mask.dtype == torch.bool and mask.device == pred.device \
        and not (src.requires_grad or slowness.requires_grad)


def wave_pml(model_output, gt):
    """loss_functions.py:358-382: the three terms of fitting the wave equation u_tt = lap u / slowness on
    a batch of (t, x, y) rows: |u - source| and |u_t| on the rows of the Dirichlet mask (the initial
    condition), times N / 10 and N / 100 with N the rows of a batch element, and |u_tt - lap u / slowness|
    on every row. While the mask is all true (pretraining; one host read per call, as in the reference)
    no second derivative is taken and the third term is 0. For a SIREN output the Hessian is
    diff_operators.hessian's one native pass, differentiable to the parameters; otherwise the
    reference's jacobian of the Jacobian's first row, by autograd. On the GPU, a float32 one-channel
    output of 3 inputs runs on siren_mri_amd::wave_loss (siren_wave.hip: one forward and one backward
    launch); everything else on the expression below."""
    src = gt["source_boundary_values"]
    x = model_output["model_in"]
    y = model_output["model_out"]
    slowness = gt["squared_slowness"]
    mask = gt["dirichlet_mask"]

    du, _ = diff_operators.jacobian(y, x)
    if torch.all(mask):
        hess = None
    elif diff_operators.siren_source(y, x) is not None:
        hess, _ = diff_operators.hessian(y, x)
    else:
        hess, _ = diff_operators.jacobian(du[..., 0, :], x)
        hess = hess.unsqueeze(2)  # [B, N, 3, 3] of output channel 0, in hessian's layout

    if _wave_native_applies(y, du, hess, src, slowness, mask):
        terms = torch.ops.siren_mri_amd.wave_loss(y, du, hess, src, slowness, mask)
        # terms[0..2] through one unbind: its backward stacks the three upstream scalars in one launch
        return dict(zip(_WAVE_KEYS, terms.unbind(0)))
    return _wave_expression(y, du, hess, src, slowness, mask, x.shape[1])


def _wave_expression(y, du, hess, src, slowness, mask, batch_size):
    """The reference's expression (loss_functions.py:366-382) in PyTorch ops, on any device and dtype:
    y [B, N, C], du [B, N, C, D], hess [B, N, C, D, D] or None, D >= 2 (time first, the Laplacian over
    the other dimensions)."""
    dudt = du[..., 0]
    if hess is None:
        diff_constraint_hom = torch.zeros(1, dtype=y.dtype, device=y.device)
    else:
        lap = hess[..., 1:, 1:].diagonal(dim1=-2, dim2=-1).sum(-1)
        dudt2 = hess[..., 0, 0]
        diff_constraint_hom = dudt2 - 1 / slowness * lap
    m = mask.expand_as(y)
    dirichlet = y[m] - src.expand_as(y)[m]
    neumann = dudt[m]
    return {"dirichlet": torch.abs(dirichlet).sum() * batch_size / 1e1,
            "neumann": torch.abs(neumann).sum() * batch_size / 1e2,
            "diff_constraint_hom": torch.abs(diff_constraint_hom).sum()}


_HELMHOLTZ_NATIVE = True
_HELMHOLTZ_KEYS = ("diff_constraint_on", "diff_constraint_off", "data_term")


def set_helmholtz_loss_native(enabled: bool) -> None:
    """Run helmholtz_pml on the native op where it applies (default on); off: the same formulas in PyTorch
    ops everywhere (A/B tests, double backward)."""
    global _HELMHOLTZ_NATIVE
    _HELMHOLTZ_NATIVE = bool(enabled)


def _helmholtz_native_applies(x, y, du, hess, src, slowness, wavenumber):
    """Whether helmholtz_pml of these operands runs on siren_mri_amd::helmholtz_loss: float32 x, y [B, N, 2]
    with the [B, N, 2, 2] Jacobian and [B, N, 2, 2, 2] Hessian on one GPU, a one-element wavenumber, ground
    truth that needs no gradient."""
    if not (_HELMHOLTZ_NATIVE and y.is_cuda and y.dim() == 3 and y.shape[-1] == 2 and x.shape == y.shape
            and tuple(du.shape) == (*y.shape, 2) and tuple(hess.shape) == (*y.shape, 2, 2)):
        return False
    if not (src.shape == y.shape and slowness.shape == y.shape and wavenumber.numel() == 1):
        return False
    return all(t.dtype == torch.float32 and t.device == y.device for t in (x, y, du, hess, src, slowness, wavenumber)) \
        and not (src.requires_grad or slowness.requires_grad or wavenumber.requires_grad)


def helmholtz_pml(model_output, gt):
    """The forward problem of loss_functions.py:385-457: the terms of fitting the Helmholtz equation with a
    perfectly matched layer, div(S grad u) + k^2 C m u = source for the complex field u = y[..., 0] + i y[..., 1]
    of (x0, x1): |e - source| on the elements whose source value is nonzero, times N / 1e3 with N the rows of
    a batch element; |e| on the others; and a data term that the forward problem leaves 0 (on the operands'
    device; the reference's is a CPU tensor).

    The reference takes jacobian(compl_mul(A, u_0), x) by autograd through the layer's coefficients A(x),
    B(x); here the product rule is written out, e = A_x0 u_0 + A u_00 + B_x1 u_1 + B u_11 + k^2 C m u, so the
    loss is linear in y, diff_operators.jacobian(y, x) and the diagonal of diff_operators.hessian(y, x): for
    a SIREN output two native passes, differentiable to the parameters. The loss is differentiable in y and
    its derivatives only: no gradient reaches x through the coefficients (training discards it, model_in
    being a detached leaf). On the GPU, a float32 two-channel output of 2 inputs with a one-element
    wavenumber runs on siren_mri_amd::helmholtz_loss (siren_helmholtz.hip: one forward and one backward
    launch); everything else on _helmholtz_expression below. The inverse problem ('pretrain' or
    'rec_boundary_values' in gt) is out of scope."""
    if "pretrain" in gt or "rec_boundary_values" in gt:
        raise NotImplementedError("helmholtz_pml: the inverse problem (full-waveform inversion: 'pretrain' / "
                                  "'rec_boundary_values' in gt) is out of scope; the forward problem is provided")
    src = gt["source_boundary_values"]
    x = model_output["model_in"]
    y = model_output["model_out"]
    slowness = gt["squared_slowness"]
    wavenumber = torch.as_tensor(gt["wavenumber"], device=y.device)
    wavenumber = wavenumber.to(y.dtype if y.dtype == torch.float64 else torch.float32)

    du, _ = diff_operators.jacobian(y, x)
    hess, _ = diff_operators.hessian(y, x)

    if _helmholtz_native_applies(x, y, du, hess, src, slowness, wavenumber):
        terms = torch.ops.siren_mri_amd.helmholtz_loss(x.detach(), y, du, hess, src, slowness, wavenumber)
        # terms[0..2] through one unbind: its backward stacks the three upstream scalars in one launch
        return dict(zip(_HELMHOLTZ_KEYS, terms.unbind(0)))
    return _helmholtz_expression(x, y, du, hess, src, slowness, wavenumber)


def _helmholtz_expression(x, y, du, hess, src, slowness, wavenumber):
    """helmholtz_pml's formulas in PyTorch ops, on any device and dtype: x [B, N, 2]; y, src [B, N, C] with
    C = 2 P interleaved real / imaginary channels; du [B, N, C, 2]; hess [B, N, C, 2, 2]; slowness [B, N, 2].
    The coefficients and the slowness are repeated over the P fields, as the reference's .repeat does."""
    from . import modules
    a0, lpml = 5.0, 0.5
    pairs = y.shape[-1] // 2
    batch_size = x.shape[1]
    xd = x.detach()
    zero = torch.zeros_like(xd[..., :1])
    one = torch.ones_like(zero)

    def layer(t):  # a0 (lo^2 + hi^2) / L^2 and its derivative, [B, N, 1]
        lo = -torch.clamp(t + (1.0 - lpml), max=0)
        hi = torch.clamp(t - (1.0 - lpml), min=0)
        return a0 * (lo ** 2 + hi ** 2) / lpml ** 2, 2 * a0 * (hi - lo) / lpml ** 2

    px, dpx = layer(xd[..., 0:1])
    py, dpy = layer(xd[..., 1:2])
    ex, ey = torch.cat((one, -px), dim=-1), torch.cat((one, -py), dim=-1)
    A, B, C = modules.compl_div(ey, ex), modules.compl_div(ex, ey), modules.compl_mul(ex, ey)
    Ax = modules.compl_mul(torch.cat((zero, dpx), dim=-1), modules.compl_div(A, ex))  # i px' ey / ex^2
    Bx = modules.compl_mul(torch.cat((zero, dpy), dim=-1), modules.compl_div(B, ey))
    A, B, C, Ax, Bx, m = (t.repeat(1, 1, pairs) for t in (A, B, C, Ax, Bx, slowness))

    e = (modules.compl_mul(Ax, du[..., 0]) + modules.compl_mul(A, hess[..., 0, 0])
         + modules.compl_mul(Bx, du[..., 1]) + modules.compl_mul(B, hess[..., 1, 1])
         + modules.compl_mul(modules.compl_mul(C, m), wavenumber ** 2 * y))
    off = torch.zeros_like(e)
    diff_constraint_on = torch.where(src != 0., e - src, off)
    diff_constraint_off = torch.where(src == 0., e, off)
    data_term = torch.zeros(1, dtype=y.dtype, device=y.device)
    return {"diff_constraint_on": torch.abs(diff_constraint_on).sum() * batch_size / 1e3,
            "diff_constraint_off": torch.abs(diff_constraint_off).sum(),
            "data_term": torch.abs(data_term).sum() * batch_size / 1}
