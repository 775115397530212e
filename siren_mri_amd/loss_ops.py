"""What binds the native loss kernels (rt_loss.hip, rt_encoder.hip's sum of squares) to PyTorch: the
autograd functions on the C entry points and the siren_mri_amd:: custom ops. loss_functions.py holds
the reference-shaped losses and decides when these apply.

  _WeightedSSE         siren_sse_forward / backward (siren_loss.hip)
  _SumSquares          siren_sumsq_forward / backward
  kspace_sse(pred, k0?, mask?, tgt, hf?, noise, weight) -> (loss, d), kspace_sse_bwd  (siren_kspace.hip)
  kspace_loss(pred, k0?, mask?, tgt, kind, noise) -> loss, kspace_loss_bwd             (siren_kloss.hip)
  kspace_fft2(x, inverse), kspace_ift_loss(pred, k0?, mask?, tgt, img_mask?, noise, img_weight,
      l1_weight, kspace_weight) -> loss, kspace_ift_loss_bwd                           (siren_kfft.hip)
  sdf_loss(pred, grad, sdf, normals) -> terms [4], sdf_loss_bwd -> (dpred, dgrad)      (siren_sdf.hip)
  wave_loss(pred, jac, hess?, src, slowness, mask) -> terms [3], wave_loss_bwd -> (dpred, djac, dhess)
                                                                                       (siren_wave.hip)
  helmholtz_loss(x, pred, jac, hess, src, slowness, wavenumber) -> terms [3], helmholtz_loss_bwd ->
      (dpred, djac, dhess)                                                        (siren_helmholtz.hip)

pred, tgt are [B, N, C]; k0, mask the [B, C, H, W] planes of a data consistency folded into the loss.
kspace_sse keeps its residual d for the backward; kspace_loss and kspace_ift_loss recompute dL/dy
from their own inputs, so their forwards save no tensor.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from .ops import _LIB


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _contig(t):
    return t.contiguous() if t is not None else None


def _loss_and_workspace(device):
    """The scalar a loss forward writes, and the hand-off workspace of (device, current stream): its
    block sums and ticket must not be shared by two launches that may run concurrently."""
    return torch.empty((), dtype=torch.float32, device=device), _native.sse_workspace(device)


def _g32(g):
    return g.contiguous().to(torch.float32)


def _upstream(g, pred, op):
    """The upstream gradient of a scalar loss as the backward kernels read it."""
    if g.numel() != 1 or g.device != pred.device:
        raise RuntimeError(f"siren_mri_amd.{op}: g must be one element on the prediction's device")
    return _g32(g)


class _WeightedSSE(torch.autograd.Function):
    """sum((m * (pred - tgt))^2) * w for real pred and a constant target on the native kernels
    (siren_sse_forward / siren_sse_backward, siren_loss.hip): forward = one launch (d = m (pred -
    tgt) and the deterministic weighted sum), backward = one launch, 2 w m^2 (pred - tgt) g — the
    values of the autograd chain of (diff.abs() ** 2).sum() * w in 2 launches instead of ~6."""

    @staticmethod
    def forward(ctx, pred, tgt, mask, weight):
        predc, tgtc, maskc = pred.contiguous(), tgt.contiguous(), _contig(mask)
        d = torch.empty_like(predc)
        loss, ws = _loss_and_workspace(pred.device)
        rc = _native.lib().siren_sse_forward(
            predc.data_ptr(), tgtc.data_ptr(), _ptr(maskc), predc.numel(), maskc.numel() if maskc is not None else 0,
            float(weight), d.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
        _native.check(rc, "siren_sse_forward")
        ctx.save_for_backward(d, maskc)
        ctx.weight = weight
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        d, mask = ctx.saved_tensors
        gc = _g32(g)
        out = torch.empty_like(d)
        rc = _native.lib().siren_sse_backward(
            d.data_ptr(), _ptr(mask), d.numel(), mask.numel() if mask is not None else 0, gc.data_ptr(),
            float(2.0 * ctx.weight), out.data_ptr(), _native.stream_handle(d.device))
        _native.check(rc, "siren_sse_backward")
        return out.view(ctx.shape), None, None, None


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


# ------------------------------------------------------------------ kspace_sse: image_mse on [B, N, C]
_LIB.define("kspace_sse(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? hf, float noise, float weight) "
            "-> (Tensor, Tensor)")
_LIB.define("kspace_sse_bwd(Tensor d, Tensor? mask, Tensor? hf, Tensor g, float noise, float scale) -> Tensor")


def _kspace_sse_cuda(pred, k0, mask, tgt, hf, noise, weight):
    b, n, c = pred.shape
    pc, tc, kc, mc, hc = pred.contiguous(), tgt.contiguous(), _contig(k0), _contig(mask), _contig(hf)
    d = torch.empty_like(pc)
    loss, ws = _loss_and_workspace(pred.device)
    rc = _native.lib().siren_kspace_sse_forward(
        pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), _ptr(hc), b, n, c, float(noise), float(weight), d.data_ptr(),
        loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_sse_forward")
    return loss, d


def _kspace_sse_bwd_cuda(d, mask, hf, g, noise, scale):
    b, n, c = d.shape
    out = torch.empty_like(d)
    mc, hc, gc = _contig(mask), _contig(hf), _g32(g)
    rc = _native.lib().siren_kspace_sse_backward(d.data_ptr(), _ptr(mc), _ptr(hc), b, n, c, float(noise), gc.data_ptr(),
                                                 float(scale), out.data_ptr(), _native.stream_handle(d.device))
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
_LIB.impl("kspace_sse", _KspaceSSEAutograd.apply, "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_sse", lambda pred, k0, mask, tgt, hf, noise, weight:
                            (pred.new_empty(()), torch.empty_like(pred)), lib=_LIB)
torch.library.register_fake("siren_mri_amd::kspace_sse_bwd", lambda d, mask, hf, g, noise, scale: torch.empty_like(d),
                            lib=_LIB)


def _recompute_autograd(name, op, tensors, what):
    """The autograd function `name` of an op whose backward, `op`_bwd, recomputes dL/dpred from the op's
    own inputs: its first `tensors` arguments (saved as they are: no residual is kept), the upstream
    gradient, then the op's constants."""
    fwd = getattr(torch.ops.siren_mri_amd, op)
    bwd = getattr(torch.ops.siren_mri_amd, op + "_bwd")

    def forward(ctx, *args):
        with torch._C._AutoDispatchBelowAutograd():
            loss = fwd(*args)
        ctx.save_for_backward(*args[:tensors])
        ctx.consts = args[tensors:]
        ctx.set_materialize_grads(False)
        return loss

    def backward(ctx, g):
        nargs = tensors + len(ctx.consts)
        if g is None:
            return (None,) * nargs
        if torch.is_grad_enabled():
            raise RuntimeError(f"siren_mri_amd: double backward through the native {what} is not provided; run it on "
                               "the expression path (siren_mri_amd.loss_functions.set_kspace_loss_native(False))")
        return (bwd(*ctx.saved_tensors, g, *ctx.consts),) + (None,) * (nargs - 1)

    return type(name, (torch.autograd.Function,), {"forward": staticmethod(forward), "backward": staticmethod(backward)})


# ------------------------------------------------------------------ kspace_loss: the k-space loss family
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
    desc = _KLOSS_DESCS.get(int(kind))
    # an unknown kind goes to the library with some descriptor: its argument check reports it
    return ctypes.byref(desc if desc is not None else _KLOSS_DESCS[_native.KLOSS_L1])


def _kloss_operands(pred, k0, mask, tgt):
    """Contiguous fp32 operands of the loss ops, shapes checked (the kernels index by pred's shape)."""
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
    return b, n, c, pred.contiguous(), _contig(k0), _contig(mask), tgt.contiguous()


def _kspace_loss_cuda(pred, k0, mask, tgt, kind, noise):
    b, n, c, pc, kc, mc, tc = _kloss_operands(pred, k0, mask, tgt)
    loss, ws = _loss_and_workspace(pred.device)
    rc = _native.lib().siren_kspace_loss_forward(
        int(kind), _kloss_desc_ref(kind), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), b, n, c, float(noise),
        loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_loss_forward")
    return loss


def _kspace_loss_bwd_cuda(pred, k0, mask, tgt, g, kind, noise):
    b, n, c, pc, kc, mc, tc = _kloss_operands(pred, k0, mask, tgt)
    gc = _upstream(g, pred, "kspace_loss_bwd")
    out = torch.empty_like(pc)
    rc = _native.lib().siren_kspace_loss_backward(
        int(kind), _kloss_desc_ref(kind), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), b, n, c, float(noise),
        gc.data_ptr(), out.data_ptr(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_loss_backward")
    return out


_LIB.impl("kspace_loss", _kspace_loss_cuda, "CUDA")
_LIB.impl("kspace_loss_bwd", _kspace_loss_bwd_cuda, "CUDA")
_LIB.impl("kspace_loss", _recompute_autograd("_KspaceLossAutograd", "kspace_loss", 4, "k-space loss").apply, "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_loss", lambda pred, k0, mask, tgt, kind, noise: pred.new_empty(()),
                            lib=_LIB)
torch.library.register_fake("siren_mri_amd::kspace_loss_bwd",
                            lambda pred, k0, mask, tgt, g, kind, noise: torch.empty_like(pred), lib=_LIB)


# ------------------------------------------------- kspace_fft2 and kspace_ift_loss, on [B, side^2, 2]
# (real, imaginary; pixels row-major as lin2img lays them out), side 8, 16, 32, 64 or 128:
#   kspace_fft2(x, inverse) -> torch.fft.fft2 / ifft2 of the complex slices, as [B, side^2, 2]
#   kspace_ift_loss -> img_weight sum m (|ifft2 y| - |ifft2 t|)^2 + l1_weight sum |y| + kspace_weight sum (y - t)^2
_LIB.define("kspace_fft2(Tensor x, bool inverse) -> Tensor")
_LIB.define("kspace_ift_loss(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? img_mask, float noise, "
            "float img_weight, float l1_weight, float kspace_weight) -> Tensor")
_LIB.define("kspace_ift_loss_bwd(Tensor pred, Tensor? k0, Tensor? mask, Tensor tgt, Tensor? img_mask, Tensor g, "
            "float noise, float img_weight, float l1_weight, float kspace_weight) -> Tensor")


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


def _kspace_ift_loss_cuda(pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight):
    b, side, pc, kc, mc, tc, ic, stride = _kift_operands(pred, k0, mask, tgt, img_mask)
    loss, ws = _loss_and_workspace(pred.device)
    desc = _native.SirenKiftDesc(img_weight, l1_weight, kspace_weight)
    rc = _native.lib().siren_kspace_ift_loss_forward(
        ctypes.byref(desc), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), _ptr(ic), stride, b, side, float(noise),
        loss.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_ift_loss_forward")
    return loss


def _kspace_ift_loss_bwd_cuda(pred, k0, mask, tgt, img_mask, g, noise, img_weight, l1_weight, kspace_weight):
    b, side, pc, kc, mc, tc, ic, stride = _kift_operands(pred, k0, mask, tgt, img_mask)
    gc = _upstream(g, pred, "kspace_ift_loss_bwd")
    out = torch.empty_like(pc)
    desc = _native.SirenKiftDesc(img_weight, l1_weight, kspace_weight)
    rc = _native.lib().siren_kspace_ift_loss_backward(
        ctypes.byref(desc), pc.data_ptr(), _ptr(kc), _ptr(mc), tc.data_ptr(), _ptr(ic), stride, b, side, float(noise),
        gc.data_ptr(), out.data_ptr(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_kspace_ift_loss_backward")
    return out


_LIB.impl("kspace_fft2", _kfft2_cuda, "CUDA")
_LIB.impl("kspace_fft2", _kfft2_autograd, "Autograd")
_LIB.impl("kspace_ift_loss", _kspace_ift_loss_cuda, "CUDA")
_LIB.impl("kspace_ift_loss_bwd", _kspace_ift_loss_bwd_cuda, "CUDA")
_LIB.impl("kspace_ift_loss", _recompute_autograd("_KspaceIftLossAutograd", "kspace_ift_loss", 5,
                                                 "image-domain k-space loss").apply, "Autograd")
torch.library.register_fake("siren_mri_amd::kspace_fft2", lambda x, inverse: torch.empty_like(x), lib=_LIB)
torch.library.register_fake(
    "siren_mri_amd::kspace_ift_loss",
    lambda pred, k0, mask, tgt, img_mask, noise, img_weight, l1_weight, kspace_weight: pred.new_empty(()), lib=_LIB)
torch.library.register_fake(
    "siren_mri_amd::kspace_ift_loss_bwd",
    lambda pred, k0, mask, tgt, img_mask, g, noise, img_weight, l1_weight, kspace_weight: torch.empty_like(pred),
    lib=_LIB)


# ------------------------------------------------------------------ sdf_loss: the signed-distance fitting loss
# pred, sdf [B, N, 1]; grad, normals [B, N, D], D = 2 or 3. The four terms of loss_functions.sdf as one [4]
# tensor (sdf, inter, normal_constraint, grad_constraint); the backward recomputes from the same inputs.
_LIB.define("sdf_loss(Tensor pred, Tensor grad, Tensor sdf, Tensor normals) -> Tensor")
_LIB.define("sdf_loss_bwd(Tensor pred, Tensor grad, Tensor sdf, Tensor normals, Tensor g) -> (Tensor, Tensor)")

SDF_TERMS = 4


def _sdf_operands(pred, grad, sdf, normals):
    """Contiguous fp32 operands of the SDF loss ops, shapes checked (the kernels index by grad's shape)."""
    if grad.dim() != 3 or grad.shape[-1] not in (2, 3) or normals.shape != grad.shape:
        raise RuntimeError(f"siren_mri_amd.sdf_loss: grad {tuple(grad.shape)} must be [B, N, D] with D 2 or 3 and "
                           f"normals {tuple(normals.shape)} of the same shape")
    b, n, d = grad.shape
    for name, t in (("pred", pred), ("sdf", sdf)):
        if tuple(t.shape) != (b, n, 1):
            raise RuntimeError(f"siren_mri_amd.sdf_loss: {name} {tuple(t.shape)} must be [{b}, {n}, 1] (one output "
                               f"channel; the gradient is {tuple(grad.shape)})")
    for name, t in (("pred", pred), ("grad", grad), ("sdf", sdf), ("normals", normals)):
        if t.dtype != torch.float32 or t.device != pred.device:
            raise RuntimeError(f"siren_mri_amd.sdf_loss: {name} must be float32 on {pred.device}")
    return b * n, d, pred.contiguous(), grad.contiguous(), sdf.contiguous(), normals.contiguous()


def _sdf_loss_cuda(pred, grad, sdf, normals):
    rows, d, pc, gc, sc, nc = _sdf_operands(pred, grad, sdf, normals)
    out = torch.empty(SDF_TERMS, dtype=torch.float32, device=pred.device)
    ws = _native.sse_workspace(pred.device)
    rc = _native.lib().siren_sdf_loss_forward(pc.data_ptr(), gc.data_ptr(), sc.data_ptr(), nc.data_ptr(), rows, d,
                                              out.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _native.stream_handle(pred.device))
    _native.check(rc, "siren_sdf_loss_forward")
    return out


def _sdf_loss_bwd_cuda(pred, grad, sdf, normals, g):
    rows, d, pc, gc, sc, nc = _sdf_operands(pred, grad, sdf, normals)
    if g.numel() != SDF_TERMS or g.device != pred.device:
        raise RuntimeError(f"siren_mri_amd.sdf_loss_bwd: g must be {SDF_TERMS} elements on the prediction's device")
    g4 = _g32(g)
    dpred, dgrad = torch.empty_like(pc), torch.empty_like(gc)
    rc = _native.lib().siren_sdf_loss_backward(pc.data_ptr(), gc.data_ptr(), sc.data_ptr(), nc.data_ptr(), rows, d,
                                               g4.data_ptr(), dpred.data_ptr(), dgrad.data_ptr(),
                                               _native.stream_handle(pred.device))
    _native.check(rc, "siren_sdf_loss_backward")
    return dpred, dgrad


class _SdfLossAutograd(torch.autograd.Function):
    """sdf_loss with sdf_loss_bwd as its backward: two differentiable inputs (pred, grad), a [4] upstream;
    the inputs are saved as they are (no residual is kept)."""

    @staticmethod
    def forward(ctx, pred, grad, sdf, normals):
        with torch._C._AutoDispatchBelowAutograd():
            terms = torch.ops.siren_mri_amd.sdf_loss(pred, grad, sdf, normals)
        ctx.save_for_backward(pred, grad, sdf, normals)
        ctx.set_materialize_grads(False)
        return terms

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        if torch.is_grad_enabled():
            raise RuntimeError("siren_mri_amd: double backward through the native SDF loss is not provided; run it on "
                               "the expression path (siren_mri_amd.loss_functions.set_sdf_loss_native(False))")
        dpred, dgrad = torch.ops.siren_mri_amd.sdf_loss_bwd(*ctx.saved_tensors, g)
        return dpred, dgrad, None, None


_LIB.impl("sdf_loss", _sdf_loss_cuda, "CUDA")
_LIB.impl("sdf_loss_bwd", _sdf_loss_bwd_cuda, "CUDA")
_LIB.impl("sdf_loss", _SdfLossAutograd.apply, "Autograd")
torch.library.register_fake("siren_mri_amd::sdf_loss", lambda pred, grad, sdf, normals: pred.new_empty((SDF_TERMS,)),
                            lib=_LIB)
torch.library.register_fake("siren_mri_amd::sdf_loss_bwd", lambda pred, grad, sdf, normals, g:
                            (torch.empty_like(pred), torch.empty_like(grad)), lib=_LIB)


# ------------------------------------------------------------------ wave_loss: the wave-equation fitting loss
# pred, src, slowness, mask [B, N, 1] (mask torch.bool); jac [B, N, 1, 3]; hess [B, N, 1, 3, 3] or None (the
# pretraining batches, whose mask is all true). The three terms of loss_functions.wave_pml as one [3]
# tensor (dirichlet, neumann, diff_constraint_hom); the backward recomputes from the same inputs.
_LIB.define("wave_loss(Tensor pred, Tensor jac, Tensor? hess, Tensor src, Tensor slowness, Tensor mask) -> Tensor")
_LIB.define("wave_loss_bwd(Tensor pred, Tensor jac, Tensor? hess, Tensor src, Tensor slowness, Tensor mask, Tensor g) "
            "-> (Tensor, Tensor, Tensor)")

WAVE_TERMS = 3


def _wave_operands(pred, jac, hess, src, slowness, mask):
    """Contiguous operands of the wave loss ops, shapes checked (the kernels index by pred's shape); the
    bool mask as a uint8 view of the same storage."""
    if pred.dim() != 3 or pred.shape[-1] != 1:
        raise RuntimeError(f"siren_mri_amd.wave_loss: pred {tuple(pred.shape)} must be [B, N, 1] (one output channel)")
    b, n, _ = pred.shape
    if tuple(jac.shape) != (b, n, 1, 3):
        raise RuntimeError(f"siren_mri_amd.wave_loss: jac {tuple(jac.shape)} must be [{b}, {n}, 1, 3] (inputs t, x, y)")
    if hess is not None and tuple(hess.shape) != (b, n, 1, 3, 3):
        raise RuntimeError(f"siren_mri_amd.wave_loss: hess {tuple(hess.shape)} must be [{b}, {n}, 1, 3, 3]")
    for name, t in (("src", src), ("slowness", slowness), ("mask", mask)):
        if tuple(t.shape) != (b, n, 1):
            raise RuntimeError(f"siren_mri_amd.wave_loss: {name} {tuple(t.shape)} must be [{b}, {n}, 1]")
    for name, t in (("pred", pred), ("jac", jac), ("hess", hess), ("src", src), ("slowness", slowness)):
        if t is not None and (t.dtype != torch.float32 or t.device != pred.device):
            raise RuntimeError(f"siren_mri_amd.wave_loss: {name} must be float32 on {pred.device}")
    if mask.dtype != torch.bool or mask.device != pred.device:
        raise RuntimeError(f"siren_mri_amd.wave_loss: mask must be bool on {pred.device}")
    return (b * n, n, pred.contiguous(), jac.contiguous(), _contig(hess), src.contiguous(), slowness.contiguous(),
            mask.contiguous().view(torch.uint8))


def _wave_loss_cuda(pred, jac, hess, src, slowness, mask):
    rows, n, pc, jc, hc, sc, lc, mc = _wave_operands(pred, jac, hess, src, slowness, mask)
    out = torch.empty(WAVE_TERMS, dtype=torch.float32, device=pred.device)
    ws = _native.sse_workspace(pred.device)
    rc = _native.lib().siren_wave_loss_forward(pc.data_ptr(), jc.data_ptr(), _ptr(hc), sc.data_ptr(), lc.data_ptr(),
                                               mc.data_ptr(), rows, n, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _native.stream_handle(pred.device))
    _native.check(rc, "siren_wave_loss_forward")
    return out


def _wave_loss_bwd_cuda(pred, jac, hess, src, slowness, mask, g):
    rows, n, pc, jc, hc, sc, lc, mc = _wave_operands(pred, jac, hess, src, slowness, mask)
    if g.numel() != WAVE_TERMS or g.device != pred.device:
        raise RuntimeError(f"siren_mri_amd.wave_loss_bwd: g must be {WAVE_TERMS} elements on the prediction's device")
    g3 = _g32(g)
    dpred, djac = torch.empty_like(pc), torch.empty_like(jc)
    dhess = torch.empty_like(hc) if hc is not None else pred.new_empty((0,))
    rc = _native.lib().siren_wave_loss_backward(pc.data_ptr(), jc.data_ptr(), _ptr(hc), sc.data_ptr(), lc.data_ptr(),
                                                mc.data_ptr(), rows, n, g3.data_ptr(), dpred.data_ptr(),
                                                djac.data_ptr(), dhess.data_ptr() if hc is not None else None,
                                                _native.stream_handle(pred.device))
    _native.check(rc, "siren_wave_loss_backward")
    return dpred, djac, dhess


class _WaveLossAutograd(torch.autograd.Function):
    """wave_loss with wave_loss_bwd as its backward: three differentiable inputs (pred, jac, hess), a [3]
    upstream; the inputs are saved as they are (no residual is kept)."""

    @staticmethod
    def forward(ctx, pred, jac, hess, src, slowness, mask):
        with torch._C._AutoDispatchBelowAutograd():
            terms = torch.ops.siren_mri_amd.wave_loss(pred, jac, hess, src, slowness, mask)
        ctx.save_for_backward(pred, jac, hess, src, slowness, mask)
        ctx.set_materialize_grads(False)
        return terms

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 6
        if torch.is_grad_enabled():
            raise RuntimeError("siren_mri_amd: double backward through the native wave loss is not provided; run it on "
                               "the expression path (siren_mri_amd.loss_functions.set_wave_loss_native(False))")
        dpred, djac, dhess = torch.ops.siren_mri_amd.wave_loss_bwd(*ctx.saved_tensors, g)
        return dpred, djac, (dhess if ctx.saved_tensors[2] is not None else None), None, None, None


def _wave_loss_bwd_fake(pred, jac, hess, src, slowness, mask, g):
    return (torch.empty_like(pred), torch.empty_like(jac),
            torch.empty_like(hess) if hess is not None else pred.new_empty((0,)))


_LIB.impl("wave_loss", _wave_loss_cuda, "CUDA")
_LIB.impl("wave_loss_bwd", _wave_loss_bwd_cuda, "CUDA")
_LIB.impl("wave_loss", _WaveLossAutograd.apply, "Autograd")
torch.library.register_fake("siren_mri_amd::wave_loss",
                            lambda pred, jac, hess, src, slowness, mask: pred.new_empty((WAVE_TERMS,)), lib=_LIB)
torch.library.register_fake("siren_mri_amd::wave_loss_bwd", _wave_loss_bwd_fake, lib=_LIB)


# ------------------------------------------------------------------ helmholtz_loss: the Helmholtz fitting loss
# x, pred, src, slowness [B, N, 2] (pred, src and slowness as real / imaginary channels); jac [B, N, 2, 2];
# hess [B, N, 2, 2, 2]; wavenumber one element on the device. The three terms of loss_functions.helmholtz_pml
# as one [3] tensor (diff_constraint_on, diff_constraint_off, data_term = 0); the backward recomputes from the
# same inputs.
_LIB.define("helmholtz_loss(Tensor x, Tensor pred, Tensor jac, Tensor hess, Tensor src, Tensor slowness, "
            "Tensor wavenumber) -> Tensor")
_LIB.define("helmholtz_loss_bwd(Tensor x, Tensor pred, Tensor jac, Tensor hess, Tensor src, Tensor slowness, "
            "Tensor wavenumber, Tensor g) -> (Tensor, Tensor, Tensor)")

HELMHOLTZ_TERMS = 3


def _helmholtz_operands(x, pred, jac, hess, src, slowness, wavenumber):
    """Contiguous operands of the Helmholtz loss ops, shapes checked (the kernels index by pred's shape)."""
    if pred.dim() != 3 or pred.shape[-1] != 2:
        raise RuntimeError(f"siren_mri_amd.helmholtz_loss: pred {tuple(pred.shape)} must be [B, N, 2] (one complex "
                           "field as two output channels)")
    b, n, _ = pred.shape
    for name, t, shape in (("x", x, (b, n, 2)), ("jac", jac, (b, n, 2, 2)), ("hess", hess, (b, n, 2, 2, 2)),
                           ("src", src, (b, n, 2)), ("slowness", slowness, (b, n, 2))):
        if tuple(t.shape) != shape:
            raise RuntimeError(f"siren_mri_amd.helmholtz_loss: {name} {tuple(t.shape)} must be {list(shape)}")
    if wavenumber.numel() != 1:
        raise RuntimeError(f"siren_mri_amd.helmholtz_loss: wavenumber {tuple(wavenumber.shape)} must be one element")
    for name, t in (("x", x), ("pred", pred), ("jac", jac), ("hess", hess), ("src", src), ("slowness", slowness),
                    ("wavenumber", wavenumber)):
        if t.dtype != torch.float32 or t.device != pred.device:
            raise RuntimeError(f"siren_mri_amd.helmholtz_loss: {name} must be float32 on {pred.device}")
    return (b * n, n, x.contiguous(), pred.contiguous(), jac.contiguous(), hess.contiguous(), src.contiguous(),
            slowness.contiguous(), wavenumber.contiguous())


def _helmholtz_loss_cuda(x, pred, jac, hess, src, slowness, wavenumber):
    rows, n, *ops = _helmholtz_operands(x, pred, jac, hess, src, slowness, wavenumber)
    out = torch.empty(HELMHOLTZ_TERMS, dtype=torch.float32, device=pred.device)
    ws = _native.sse_workspace(pred.device)
    rc = _native.lib().siren_helmholtz_loss_forward(*(t.data_ptr() for t in ops), rows, n, out.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), _native.stream_handle(pred.device))
    _native.check(rc, "siren_helmholtz_loss_forward")
    return out


def _helmholtz_loss_bwd_cuda(x, pred, jac, hess, src, slowness, wavenumber, g):
    rows, n, *ops = _helmholtz_operands(x, pred, jac, hess, src, slowness, wavenumber)
    if g.numel() != HELMHOLTZ_TERMS or g.device != pred.device:
        raise RuntimeError(f"siren_mri_amd.helmholtz_loss_bwd: g must be {HELMHOLTZ_TERMS} elements on the "
                           "prediction's device")
    g3 = _g32(g)
    dpred, djac, dhess = torch.empty_like(ops[1]), torch.empty_like(ops[2]), torch.empty_like(ops[3])
    rc = _native.lib().siren_helmholtz_loss_backward(*(t.data_ptr() for t in ops), rows, n, g3.data_ptr(),
                                                     dpred.data_ptr(), djac.data_ptr(), dhess.data_ptr(),
                                                     _native.stream_handle(pred.device))
    _native.check(rc, "siren_helmholtz_loss_backward")
    return dpred, djac, dhess


class _HelmholtzLossAutograd(torch.autograd.Function):
    """helmholtz_loss with helmholtz_loss_bwd as its backward: three differentiable inputs (pred, jac, hess), a
    [3] upstream; the inputs are saved as they are (no residual is kept). x, src, slowness and wavenumber get
    None: the path from x through the layer's coefficients is not provided (training discards that gradient,
    model_in being a detached leaf)."""

    @staticmethod
    def forward(ctx, x, pred, jac, hess, src, slowness, wavenumber):
        with torch._C._AutoDispatchBelowAutograd():
            terms = torch.ops.siren_mri_amd.helmholtz_loss(x, pred, jac, hess, src, slowness, wavenumber)
        ctx.save_for_backward(x, pred, jac, hess, src, slowness, wavenumber)
        ctx.set_materialize_grads(False)
        return terms

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        if torch.is_grad_enabled():
            raise RuntimeError("siren_mri_amd: double backward through the native Helmholtz loss is not provided; run "
                               "it on the expression path (siren_mri_amd.loss_functions.set_helmholtz_loss_native(False))")
        dpred, djac, dhess = torch.ops.siren_mri_amd.helmholtz_loss_bwd(*ctx.saved_tensors, g)
        return None, dpred, djac, dhess, None, None, None


_LIB.impl("helmholtz_loss", _helmholtz_loss_cuda, "CUDA")
_LIB.impl("helmholtz_loss_bwd", _helmholtz_loss_bwd_cuda, "CUDA")
_LIB.impl("helmholtz_loss", _HelmholtzLossAutograd.apply, "Autograd")
torch.library.register_fake("siren_mri_amd::helmholtz_loss", lambda x, pred, jac, hess, src, slowness, wavenumber:
                            pred.new_empty((HELMHOLTZ_TERMS,)), lib=_LIB)
torch.library.register_fake("siren_mri_amd::helmholtz_loss_bwd", lambda x, pred, jac, hess, src, slowness, wavenumber, g:
                            (torch.empty_like(pred), torch.empty_like(jac), torch.empty_like(hess)), lib=_LIB)
