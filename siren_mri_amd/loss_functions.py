"""Losses on the SIREN hot path (drop-in for loss_functions.py of jonbmartin/siren_mri).

  image_mse                loss_functions.py:66-101
  latent_loss              loss_functions.py:275-276
  hypo_weight_loss         loss_functions.py:279-287
  image_hypernetwork_loss  loss_functions.py:290-293
  image_mse_log, image_mse_cubic, image_smape, image_asinh, image_perp, kspace_l1
                           loss_functions.py:12-64, 103-190 (the k-space loss family)
  ift_image_mse, image_l1  loss_functions.py:192-235
  image_hypernetwork_{perp,asinh,l1,log,cubic,ift}_loss  loss_functions.py:295-323
  function_mse             loss_functions.py:326-327
  gradients_mse            loss_functions.py:330-335
  laplace_mse              loss_functions.py:350-355

image_mse runs on the native k-space op (siren_kspace.hip), with the data consistency of a native
DataConsistencyInKspace output folded in. The six k-space losses of the
family run on siren_mri_amd::kspace_loss (siren_kloss.hip: one forward and one backward launch, the
DC folded in the same way); ift_image_mse runs on siren_mri_amd::kspace_ift_loss (siren_kfft.hip: the
two ifft2 and the three sums in one forward launch, one backward launch) for square slices of side
8 to 128, and is a PyTorch composition otherwise, as image_l1 is.

Deliberate deviation (bug 0.2): the reference builds its high-frequency mask
on a fixed 128x128 grid, so image_mse(high_freq=True) raises for any other image size; here the
mask applies when the image is 128x128 and the loss is the plain SSE otherwise.

Deliberate deviation: image_mse_log does not print its two partial sums on every call
(loss_functions.py:37); that print forces a host synchronisation per step.
"""
from __future__ import annotations

import torch

from . import _native, diff_operators, fusion
from .data_consistency import dc_source
from .dataio import lin2img
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


def _sse_workspace(device):
    # one workspace per (device, stream): its block sums and ticket must not be shared by two
    # launches that may run concurrently
    return _native.sse_workspace(device)


class _WeightedSSE(torch.autograd.Function):
    """sum((m * (pred - tgt))^2) * w for real pred and a constant target on the native kernels
    (siren_sse_forward / siren_sse_backward, siren_loss.hip): forward = one launch (d = m (pred -
    tgt) and the deterministic weighted sum), backward = one launch, 2 w m^2 (pred - tgt) g — the
    values of the autograd chain of (diff.abs() ** 2).sum() * w in 2 launches instead of ~6."""

    @staticmethod
    def forward(ctx, pred, tgt, mask, weight):
        predc, tgtc = pred.contiguous(), tgt.contiguous()
        maskc = mask.contiguous() if mask is not None else None
        n = predc.numel()
        d = torch.empty_like(predc)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = _sse_workspace(pred.device)
        rc = _native.lib().siren_sse_forward(
            predc.data_ptr(), tgtc.data_ptr(), maskc.data_ptr() if maskc is not None else None, n,
            maskc.numel() if maskc is not None else 0, float(weight), d.data_ptr(), loss.data_ptr(),
            ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
        _native.check(rc, "siren_sse_forward")
        ctx.save_for_backward(d, maskc)
        ctx.weight = weight
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        d, mask = ctx.saved_tensors
        gc = g.contiguous().to(torch.float32)
        out = torch.empty_like(d)
        rc = _native.lib().siren_sse_backward(
            d.data_ptr(), mask.data_ptr() if mask is not None else None, d.numel(),
            mask.numel() if mask is not None else 0, gc.data_ptr(), float(2.0 * ctx.weight), out.data_ptr(),
            _native.stream_handle(d.device))
        _native.check(rc, "siren_sse_backward")
        return out.view(ctx.shape), None, None, None


# image_mse on the SIREN output layout [B, N, C], optionally with data consistency folded in
# (siren_kspace.hip): siren_mri_amd::kspace_sse(pred, k0?, mask?, tgt, hf?, noise, weight) -> (loss, d)
from .ops import _LIB  # noqa: E402

_LIB.define("kspace_sse(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? hf, float noise, float weight) "
            "-> (Tensor, Tensor)")
_LIB.define("kspace_sse_bwd(Tensor d, Tensor? mask, Tensor? hf, Tensor g, float noise, float scale) -> Tensor")


def _kspace_sse_cuda(pred, k0, mask, tgt, hf, noise, weight):
    b, n, c = pred.shape
    pc, tc = pred.contiguous(), tgt.contiguous()
    kc = k0.contiguous() if k0 is not None else None
    mc = mask.contiguous() if mask is not None else None
    hc = hf.contiguous() if hf is not None else None
    d = torch.empty_like(pc)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = _sse_workspace(pred.device)
    rc = _native.lib().siren_kspace_sse_forward(
        pc.data_ptr(), kc.data_ptr() if kc is not None else None, mc.data_ptr() if mc is not None else None,
        tc.data_ptr(), hc.data_ptr() if hc is not None else None, b, n, c, float(noise), float(weight), d.data_ptr(),
        loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_sse_forward")
    return loss, d


def _kspace_sse_bwd_cuda(d, mask, hf, g, noise, scale):
    b, n, c = d.shape
    out = torch.empty_like(d)
    mc = mask.contiguous() if mask is not None else None
    hc = hf.contiguous() if hf is not None else None
    gc = g.contiguous().to(torch.float32)
    rc = _native.lib().siren_kspace_sse_backward(d.data_ptr(), mc.data_ptr() if mc is not None else None,
                                                 hc.data_ptr() if hc is not None else None, b, n, c, float(noise),
                                                 gc.data_ptr(), float(scale), out.data_ptr(),
                                                 _native.stream_handle(d.device))
    _native.check(rc, "siren_kspace_sse_backward")
    return out


class _KspaceSSEAutograd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, k0, mask, tgt, hf, noise, weight):
        with torch._C._AutoDispatchBelowAutograd():
            loss, d = torch.ops.siren_mri_amd.kspace_sse(pred, k0, mask, tgt, hf, noise, weight)
        ctx.save_for_backward(d, mask, hf)
        ctx.noise, ctx.weight = noise, weight
        ctx.mark_non_differentiable(d)
        ctx.set_materialize_grads(False)
        return loss, d

    @staticmethod
    def backward(ctx, g, _gd):
        if g is None:
            return (None,) * 7
        d, mask, hf = ctx.saved_tensors
        dpred = torch.ops.siren_mri_amd.kspace_sse_bwd(d, mask, hf, g, ctx.noise, 2.0 * ctx.weight)
        return dpred, None, None, None, None, None, None


_LIB.impl("kspace_sse", _kspace_sse_cuda, "CUDA")
_LIB.impl("kspace_sse_bwd", _kspace_sse_bwd_cuda, "CUDA")
_LIB.impl("kspace_sse", lambda pred, k0, mask, tgt, hf, noise, weight:
          _KspaceSSEAutograd.apply(pred, k0, mask, tgt, hf, noise, weight), "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_sse", lambda pred, k0, mask, tgt, hf, noise, weight:
                            (pred.new_empty(()), torch.empty_like(pred)), lib=_LIB)
torch.library.register_fake("siren_mri_amd::kspace_sse_bwd", lambda d, mask, hf, g, noise, scale: torch.empty_like(d),
                            lib=_LIB)

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


def _kspace_image_mse(out, tgt, high_freq):
    """image_mse on [B, N, C] (N a square): the native k-space op, or None when not applicable."""
    if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and tgt.shape == out.shape
            and tgt.dtype == torch.float32 and tgt.device == out.device and not tgt.requires_grad
            and out.shape[-1] <= 8):
        return None
    n = out.shape[1]
    side = int(round(n ** 0.5))
    if side * side != n:
        return None
    hf = _hf_flat(out.device) if (high_freq and side == 128) else None
    src = dc_source(out) if _FUSE_DC else None
    if src is not None and src[0].shape == out.shape:
        pred, k0, mask, noise = src
        return torch.ops.siren_mri_amd.kspace_sse(pred, k0, mask, tgt, hf, noise, _KSPACE_WEIGHT)[0]
    return torch.ops.siren_mri_amd.kspace_sse(out, None, None, tgt, hf, 0.0, _KSPACE_WEIGHT)[0]


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


_SUMSQ_WS = {}


def _sumsq_workspace(device, total):
    """Per-(device, stream) zeroed workspace of siren_sumsq_forward (left zeroed by every launch)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    need = int(_native.lib().siren_sumsq_workspace_bytes(total))
    ws = _SUMSQ_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        _SUMSQ_WS[key] = ws
    return ws


class _SumSquares(torch.autograd.Function):
    """sum over tensors of torch.sum(w ** 2) in one native launch (siren_sumsq_forward), its
    gradient 2 g w in one more (siren_sumsq_backward)."""

    @staticmethod
    def forward(ctx, *ws):
        import ctypes
        ts = [w.detach().contiguous() for w in ws]
        n = len(ts)
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
        out = torch.empty((), dtype=torch.float32, device=ts[0].device)
        work = _sumsq_workspace(ts[0].device, sum(t.numel() for t in ts))
        _native.check(_native.lib().siren_sumsq_forward(n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]), numel,
                                                        out.data_ptr(), work.data_ptr(), work.numel(),
                                                        _native.stream_handle(ts[0].device)), "siren_sumsq_forward")
        ctx.save_for_backward(*ws)  # the inputs: a create_graph backward differentiates through them
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        if torch.is_grad_enabled():
            # create_graph=True: the exact gradient 2 g w in differentiable PyTorch
            return tuple(2 * g * w if need else None for w, need in zip(ctx.saved_tensors, ctx.needs_input_grad))
        ts = [w.detach().contiguous() for w in ctx.saved_tensors]
        n = len(ts)
        gc = g.detach().reshape(()).to(torch.float32).contiguous()
        outs = [torch.empty_like(t) for t in ts]
        _native.check(_native.lib().siren_sumsq_backward(n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]),
                                                         (ctypes.c_int64 * n)(*[t.numel() for t in ts]), gc.data_ptr(),
                                                         (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                                         _native.stream_handle(ts[0].device)), "siren_sumsq_backward")
        return tuple(o if need else None for o, need in zip(outs, ctx.needs_input_grad))


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


# The k-space loss family on the SIREN output layout [B, N, C], optionally with data consistency
# folded in (siren_kloss.hip):
#   siren_mri_amd::kspace_loss(pred, k0?, mask?, tgt, kind, noise) -> loss
#   siren_mri_amd::kspace_loss_bwd(pred, k0?, mask?, tgt, g, kind, noise) -> dpred
# The backward recomputes dL/dy from its inputs: the forward saves no residual tensor.
_LIB.define("kspace_loss(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, int kind, float noise) -> Tensor")
_LIB.define("kspace_loss_bwd(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor g, int kind, float noise) "
            "-> Tensor")


def _kloss_desc(weight=1.0, eps=0.0, scale=0.0, divisor=1.0, mag_weight=0.0, phase_weight=0.0):
    return _native.SirenKlossDesc(weight, eps, scale, divisor, mag_weight, phase_weight)


# the reference's constants, per kind (loss_functions.py:25-35, 52-57, 110-111, 127-135, 156-161, 183)
_KLOSS_DESCS = {
    _native.KLOSS_ASINH: _kloss_desc(weight=1 / (128 * 128), scale=400.0, divisor=6.7),
    _native.KLOSS_CUBIC: _kloss_desc(weight=0.000001, eps=1e-3),
    _native.KLOSS_SMAPE: _kloss_desc(weight=1 / (128 * 128), eps=1e-3),
    _native.KLOSS_L1: _kloss_desc(weight=1 / (128 * 128)),
    _native.KLOSS_PERP: _kloss_desc(weight=1 / (128 * 128) * 1000, eps=1e-8),
    _native.KLOSS_LOG: _kloss_desc(weight=1.0, eps=1e-3, mag_weight=0.0001, phase_weight=0.0001),
}


def _kloss_desc_ref(kind):
    import ctypes
    desc = _KLOSS_DESCS.get(int(kind))
    # an unknown kind goes to the library with some descriptor: its argument check reports it
    return ctypes.byref(desc if desc is not None else _KLOSS_DESCS[_native.KLOSS_L1])


def _kloss_operands(pred, k0, mask, tgt):
    """Contiguous fp32 operands of the two ops, shapes checked (the kernels index by pred's shape)."""
    if pred.dim() != 3 or tgt.shape != pred.shape:
        raise RuntimeError(f"siren_mri_amd.kspace_loss: pred {tuple(pred.shape)} must be [B, N, C] and tgt "
                           f"{tuple(tgt.shape)} of the same shape")
    b, n, c = pred.shape
    for name, t in (("k0", k0), ("mask", mask)):
        if t is not None and (t.dim() < 3 or t.shape[0] != b or t.shape[1] != c or t.numel() != pred.numel()):
            raise RuntimeError(f"siren_mri_amd.kspace_loss: {name} planes {tuple(t.shape)} do not match the "
                               f"prediction {tuple(pred.shape)}")
    for name, t in (("pred", pred), ("k0", k0), ("mask", mask), ("tgt", tgt)):
        if t is not None and (t.dtype != torch.float32 or t.device != pred.device):
            raise RuntimeError(f"siren_mri_amd.kspace_loss: {name} must be float32 on {pred.device}")
    return (b, n, c, pred.contiguous(), k0.contiguous() if k0 is not None else None,
            mask.contiguous() if mask is not None else None, tgt.contiguous())


def _kspace_loss_cuda(pred, k0, mask, tgt, kind, noise):
    b, n, c, pc, kc, mc, tc = _kloss_operands(pred, k0, mask, tgt)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = _sse_workspace(pred.device)
    rc = _native.lib().siren_kspace_loss_forward(
        int(kind), _kloss_desc_ref(kind), pc.data_ptr(), kc.data_ptr() if kc is not None else None,
        mc.data_ptr() if mc is not None else None, tc.data_ptr(), b, n, c, float(noise), loss.data_ptr(),
        ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_loss_forward")
    return loss


def _kspace_loss_bwd_cuda(pred, k0, mask, tgt, g, kind, noise):
    b, n, c, pc, kc, mc, tc = _kloss_operands(pred, k0, mask, tgt)
    if g.numel() != 1 or g.device != pred.device:
        raise RuntimeError("siren_mri_amd.kspace_loss_bwd: g must be one element on the prediction's device")
    gc = g.contiguous().to(torch.float32)
    out = torch.empty_like(pc)
    rc = _native.lib().siren_kspace_loss_backward(
        int(kind), _kloss_desc_ref(kind), pc.data_ptr(), kc.data_ptr() if kc is not None else None,
        mc.data_ptr() if mc is not None else None, tc.data_ptr(), b, n, c, float(noise), gc.data_ptr(),
        out.data_ptr(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_loss_backward")
    return out


class _KspaceLossAutograd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, k0, mask, tgt, kind, noise):
        with torch._C._AutoDispatchBelowAutograd():
            loss = torch.ops.siren_mri_amd.kspace_loss(pred, k0, mask, tgt, kind, noise)
        ctx.save_for_backward(pred, k0, mask, tgt)  # the op's own inputs: no residual is kept
        ctx.kind, ctx.noise = kind, noise
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 6
        if torch.is_grad_enabled():
            raise RuntimeError("siren_mri_amd: double backward through the native k-space loss is not provided; "
                               "run it on the expression path (siren_mri_amd.loss_functions."
                               "set_kspace_loss_native(False))")
        pred, k0, mask, tgt = ctx.saved_tensors
        dpred = torch.ops.siren_mri_amd.kspace_loss_bwd(pred, k0, mask, tgt, g, ctx.kind, ctx.noise)
        return dpred, None, None, None, None, None


_LIB.impl("kspace_loss", _kspace_loss_cuda, "CUDA")
_LIB.impl("kspace_loss_bwd", _kspace_loss_bwd_cuda, "CUDA")
_LIB.impl("kspace_loss", lambda pred, k0, mask, tgt, kind, noise:
          _KspaceLossAutograd.apply(pred, k0, mask, tgt, kind, noise), "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_loss", lambda pred, k0, mask, tgt, kind, noise: pred.new_empty(()),
                            lib=_LIB)
torch.library.register_fake("siren_mri_amd::kspace_loss_bwd",
                            lambda pred, k0, mask, tgt, g, kind, noise: torch.empty_like(pred), lib=_LIB)

_KLOSS_NATIVE = True


def set_kspace_loss_native(enabled: bool) -> None:
    """Run the k-space loss family on the native op where it applies (default on); off: the
    reference's expression in PyTorch everywhere (A/B tests)."""
    global _KLOSS_NATIVE
    _KLOSS_NATIVE = bool(enabled)


def _kspace_loss_native(out, tgt, kind):
    """A loss of the family on [B, N, C] through the native op, or None when it does not apply."""
    if not (_KLOSS_NATIVE and out.is_cuda and out.dtype == torch.float32 and out.dim() == 3
            and tgt.shape == out.shape and tgt.dtype == torch.float32 and tgt.device == out.device
            and not tgt.requires_grad and 1 <= out.shape[-1] <= 8):
        return None
    if kind in (_native.KLOSS_PERP, _native.KLOSS_LOG) and out.shape[-1] != 2:
        return None
    src = dc_source(out) if _FUSE_DC else None
    if src is not None and src[0].shape == out.shape:
        pred, k0, mask, noise = src
        return torch.ops.siren_mri_amd.kspace_loss(pred, k0, mask, tgt, kind, noise)
    return torch.ops.siren_mri_amd.kspace_loss(out, None, None, tgt, kind, 0.0)


# The image-domain member of the family and the transform it runs on (siren_kfft.hip), on [B, side^2, 2]
# (real, imaginary; pixels row-major as lin2img lays them out), side 8, 16, 32, 64 or 128:
#   siren_mri_amd::kspace_fft2(x, inverse) -> torch.fft.fft2 / ifft2 of the complex slices, as [B, side^2, 2]
#   siren_mri_amd::kspace_ift_loss(pred, k0?, mask?, tgt, img_mask?, noise, img_weight, l1_weight, kspace_weight)
#       -> img_weight sum m (|ifft2 y| - |ifft2 t|)^2 + l1_weight sum |y| + kspace_weight sum (y - t)^2
#   siren_mri_amd::kspace_ift_loss_bwd(the same operands, g, ...) -> dpred
# One launch each; the backward recomputes everything from its inputs, so the forward saves no residual.
_LIB.define("kspace_fft2(Tensor x, bool inverse) -> Tensor")
_LIB.define("kspace_ift_loss(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? img_mask, float noise, "
            "float img_weight, float l1_weight, float kspace_weight) -> Tensor")
_LIB.define("kspace_ift_loss_bwd(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? img_mask, Tensor g, "
            "float noise, float img_weight, float l1_weight, float kspace_weight) -> Tensor")

# ift_image_mse's constants (loss_functions.py:207-229): image SSE, 1e-8 sum |y|, 0.0025 k-space SSE
_IFT_WEIGHTS = (1.0, 1e-8, 0.0025)


def _kfft_side(n):
    """The side of an n-pixel slice the transform kernels take, or None."""
    side = int(round(n ** 0.5))
    return side if side * side == n and side in _native.KFFT_SIDES else None


def _kift_max_batch():
    """Slices per launch of the loss ops: one slot of the SSE workspace each."""
    return (int(_native.lib().siren_sse_workspace_bytes()) - 256) // 4


def _kfft2_cuda(x, inverse):
    if x.dim() != 3 or x.shape[-1] != 2 or _kfft_side(x.shape[1]) is None or x.dtype != torch.float32:
        raise RuntimeError(f"siren_mri_amd.kspace_fft2: x {tuple(x.shape)} {x.dtype} must be float32 [B, side^2, 2] "
                           f"with side in {_native.KFFT_SIDES}")
    xc = x.contiguous()
    out = torch.empty_like(xc)
    rc = _native.lib().siren_kspace_fft2(xc.data_ptr(), out.data_ptr(), xc.shape[0], _kfft_side(xc.shape[1]),
                                         1 if inverse else 0, _native.stream_handle(x.device))
    _native.check(rc, "siren_kspace_fft2")
    return out


def _kfft2_autograd(x, inverse):
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("siren_mri_amd.kspace_fft2 is not differentiable: detach its input (the image-domain "
                           "loss with a gradient is siren_mri_amd.kspace_ift_loss), or use torch.fft")
    with torch._C._AutoDispatchBelowAutograd():
        return torch.ops.siren_mri_amd.kspace_fft2(x, inverse)


def _kift_operands(pred, k0, mask, tgt, img_mask):
    """Contiguous fp32 operands of the two loss ops; img_mask as (tensor or None, its batch stride)."""
    b, n, c, pc, kc, mc, tc = _kloss_operands(pred, k0, mask, tgt)
    side = _kfft_side(n)
    if c != 2 or side is None:
        raise RuntimeError(f"siren_mri_amd.kspace_ift_loss: pred {tuple(pred.shape)} must be [B, side^2, 2] with side "
                           f"in {_native.KFFT_SIDES}")
    stride = 0
    if img_mask is not None:
        if img_mask.dtype != torch.float32 or img_mask.device != pred.device:
            raise RuntimeError(f"siren_mri_amd.kspace_ift_loss: img_mask must be float32 on {pred.device}")
        if tuple(img_mask.shape) == (b, side, side) and b > 1:
            stride = n
        elif tuple(img_mask.shape) not in ((side, side), (1, side, side)):
            raise RuntimeError(f"siren_mri_amd.kspace_ift_loss: img_mask {tuple(img_mask.shape)} is neither "
                               f"[{side}, {side}] nor [{b}, {side}, {side}]")
        img_mask = img_mask.contiguous()
    return b, side, pc, kc, mc, tc, img_mask, stride


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _kspace_ift_loss_cuda(pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight):
    import ctypes
    b, side, pc, kc, mc, tc, ic, stride = _kift_operands(pred, k0, mask, tgt, img_mask)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = _sse_workspace(pred.device)
    desc = _native.SirenKiftDesc(img_weight, l1_weight, kspace_weight)
    rc = _native.lib().siren_kspace_ift_loss_forward(
        ctypes.byref(desc), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), _ptr(ic), stride, b, side, float(noise),
        loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_ift_loss_forward")
    return loss


def _kspace_ift_loss_bwd_cuda(pred, k0, mask, tgt, img_mask, g, noise, img_weight, l1_weight, kspace_weight):
    import ctypes
    b, side, pc, kc, mc, tc, ic, stride = _kift_operands(pred, k0, mask, tgt, img_mask)
    if g.numel() != 1 or g.device != pred.device:
        raise RuntimeError("siren_mri_amd.kspace_ift_loss_bwd: g must be one element on the prediction's device")
    gc = g.contiguous().to(torch.float32)
    out = torch.empty_like(pc)
    desc = _native.SirenKiftDesc(img_weight, l1_weight, kspace_weight)
    rc = _native.lib().siren_kspace_ift_loss_backward(
        ctypes.byref(desc), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), _ptr(ic), stride, b, side, float(noise),
        gc.data_ptr(), out.data_ptr(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_ift_loss_backward")
    return out


class _KspaceIftLossAutograd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight):
        with torch._C._AutoDispatchBelowAutograd():
            loss = torch.ops.siren_mri_amd.kspace_ift_loss(pred, k0, mask, tgt, img_mask, noise, img_weight,
                                                           l1_weight, kspace_weight)
        ctx.save_for_backward(pred, k0, mask, tgt, img_mask)  # the op's own inputs: no residual is kept
        ctx.consts = (noise, img_weight, l1_weight, kspace_weight)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 9
        if torch.is_grad_enabled():
            raise RuntimeError("siren_mri_amd: double backward through the native image-domain k-space loss is not "
                               "provided; run it on the expression path (siren_mri_amd.loss_functions."
                               "set_kspace_loss_native(False))")
        pred, k0, mask, tgt, img_mask = ctx.saved_tensors
        dpred = torch.ops.siren_mri_amd.kspace_ift_loss_bwd(pred, k0, mask, tgt, img_mask, g, *ctx.consts)
        return (dpred,) + (None,) * 8


_LIB.impl("kspace_fft2", _kfft2_cuda, "CUDA")
_LIB.impl("kspace_fft2", _kfft2_autograd, "Autograd")
_LIB.impl("kspace_ift_loss", _kspace_ift_loss_cuda, "CUDA")
_LIB.impl("kspace_ift_loss_bwd", _kspace_ift_loss_bwd_cuda, "CUDA")
_LIB.impl("kspace_ift_loss", lambda pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight:
          _KspaceIftLossAutograd.apply(pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight),
          "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_fft2", lambda x, inverse: torch.empty_like(x), lib=_LIB)
torch.library.register_fake(
    "siren_mri_amd::kspace_ift_loss",
    lambda pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight: pred.new_empty(()), lib=_LIB)
torch.library.register_fake(
    "siren_mri_amd::kspace_ift_loss_bwd",
    lambda pred, k0, mask, tgt, img_mask, g, noise, img_weight, l1_weight, kspace_weight: torch.empty_like(pred),
    lib=_LIB)


def _ift_native_applies(mask, out, tgt):
    """Whether ift_image_mse of these operands runs on siren_mri_amd::kspace_ift_loss."""
    if not (_KLOSS_NATIVE and torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 3
            and out.shape[-1] == 2 and tgt.shape == out.shape and tgt.dtype == torch.float32
            and tgt.device == out.device and not tgt.requires_grad):
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
    src = dc_source(out) if _FUSE_DC else None
    if src is not None and src[0].shape == out.shape:
        pred, k0, planes, noise = src
        return torch.ops.siren_mri_amd.kspace_ift_loss(pred, k0, planes, tgt, mask, noise, *_IFT_WEIGHTS)
    return torch.ops.siren_mri_amd.kspace_ift_loss(out, None, None, tgt, mask, 0.0, *_IFT_WEIGHTS)


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
