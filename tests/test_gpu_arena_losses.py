"""GPU: the loss and k-space entry points on a poisoned arena (tests/_arena.py): siren_sse_*, siren_dc_*,
siren_kspace_sse_*, siren_kspace_loss_*, siren_kspace_fft2, siren_kspace_ift_loss_*,
siren_fourier_features and siren_sincos_f32, each with every operand on the allocator's alignment and
with every float operand 4 bytes off it (the scalar branches of the alignment-gated kernels).

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs), I3 (outputs written in full), I4 (the loss workspace, "zeroed once and left zeroed by every
launch", is zero again) hold and I5 every output is bit-equal to the plain run (the suite asserts
run-to-run bit equality of all of these: deterministic summation orders). I7: a loss workspace one byte
short is refused with SIREN_ENOSPACE before any launch. The values themselves are held to their float64
references by test_gpu_loss.py, test_gpu_kspace*.py and test_gpu_sincos.py; a coarse float64 check of
the arena run here keeps the two runs from being wrong together."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _arena import Plain, same_bits  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
F32, U8 = torch.float32, torch.uint8
OFFSETS = [0, 4]


def both(driver, *args):
    plain = Plain(DEV)
    a = driver(plain, *args)
    plain.verify()
    arena = plain.arena()
    b = driver(arena, *args)
    arena.verify()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"I5: {k} differs between the plain and the arena run"
    return {k: v.cpu() for k, v in b.items()}


def refused(driver, *args):
    """I7: the driver with its workspace one byte short, on an arena."""
    plain = Plain(DEV)
    driver(plain, *args)
    arena = plain.arena()
    assert driver(arena, *args, short=True) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()


class Taker:
    """take() with one offset for every float operand."""

    def __init__(self, alloc, off):
        self.alloc, self.off = alloc, off

    def inp(self, name, t):
        return self.alloc.take(t.shape, t.dtype, role="input", fill=t, name=name, offset_bytes=self.off) if t is not None else None

    def out(self, name, shape, dtype=F32):
        return self.alloc.take(shape, dtype, role="output", name=name, offset_bytes=self.off)

    def loss_ws(self):
        n = int(_native.lib().siren_sse_workspace_bytes())
        return self.alloc.take((n,), U8, role="zeroed", name="loss_ws"), n


def ptr(t):
    return t.data_ptr() if t is not None else None


def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def stream():
    return _native.stream_handle(DEV)


def ok(rc):
    assert rc == 0, _native.last_error()


# ---------------------------------------------------------------------- siren_sse_forward / backward
def run_sse(alloc, n, mask_n, off, short=False):
    lib, t = _native.lib(), Taker(alloc, off)
    pred, tgt, g = t.inp("pred", rand(n, seed=1)), t.inp("tgt", rand(n, seed=2)), t.inp("g", torch.tensor([1.5]))
    mask = t.inp("mask", (rand(mask_n, seed=3) > 0).float()) if mask_n else None
    out = {"d": t.out("d", (n,)), "loss": t.out("loss", (1,))}
    ws, wsn = t.loss_ws()
    rc = lib.siren_sse_forward(ptr(pred), ptr(tgt), ptr(mask), n, mask_n, 0.25, ptr(out["d"]), ptr(out["loss"]), ptr(ws),
                               wsn - short, stream())
    if short:
        return rc
    ok(rc)
    alloc.freeze("d")
    out["dpred"] = t.out("dpred", (n,))
    ok(lib.siren_sse_backward(ptr(out["d"]), ptr(mask), n, mask_n, ptr(g), 0.5, ptr(out["dpred"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n,mask_n", [(1001, 0), (1001, 1001), (1001, 143), (1001, 7), (3, 0), (3, 3), (3, 1)])
def test_sse(n, mask_n, off):
    o = both(run_sse, n, mask_n, off)
    m = (rand(mask_n, seed=3) > 0).double().repeat(n // mask_n) if mask_n else torch.ones(n).double()
    d = m * (rand(n, seed=1).double() - rand(n, seed=2).double())
    assert orc.norm_rel(o["d"], d) <= 1e-6
    assert float(o["loss"]) == pytest.approx(0.25 * float((d ** 2).sum()), rel=1e-5, abs=1e-30)
    assert orc.norm_rel(o["dpred"], m * d * 1.5 * 0.5) <= 1e-6


def test_sse_short_workspace_is_refused_before_any_launch():
    refused(run_sse, 1001, 143, 0)


# ---------------------------------------------------------------------- data consistency, k-space SSE
def kspace_inputs(batch, npix, channels, dc=True):
    pred, tgt = rand(batch, npix, channels, seed=4), rand(batch, npix, channels, seed=5)
    k0 = rand(batch, channels, npix, seed=6) if dc else None
    mask = (rand(batch, channels, npix, seed=7) > 0.3).float() if dc else None
    return pred, tgt, k0, mask


def dc64(pred, k0, mask, noise):
    y = pred.double()
    if k0 is None:
        return y, torch.ones_like(y)
    m, k = mask.double().permute(0, 2, 1), k0.double().permute(0, 2, 1)
    if noise <= 0:
        return (1 - m) * y + m * k, 1 - m
    return (1 - m) * y + m * (y + noise * k) / (1 + noise), (1 - m) + m / (1 + noise)


def run_dc(alloc, channels, noise, off):
    lib, t = _native.lib(), Taker(alloc, off)
    pred, _, k0, mask = kspace_inputs(3, 333, channels)
    p, k, m, g = t.inp("pred", pred), t.inp("k0", k0), t.inp("mask", mask), t.inp("g", rand(3, 333, channels, seed=8))
    out = {"out": t.out("out", pred.shape), "dpred": t.out("dpred", pred.shape)}
    ok(lib.siren_dc_forward(ptr(p), ptr(k), ptr(m), 3, 333, channels, noise, ptr(out["out"]), stream()))
    ok(lib.siren_dc_backward(ptr(g), ptr(m), 3, 333, channels, noise, ptr(out["dpred"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("noise", [0.0, 0.25])
@pytest.mark.parametrize("channels", [1, 2])
def test_dc(channels, noise, off):
    o = both(run_dc, channels, noise, off)
    pred, _, k0, mask = kspace_inputs(3, 333, channels)
    y, coef = dc64(pred, k0, mask, noise)
    assert orc.norm_rel(o["out"], y) <= 1e-6
    assert orc.norm_rel(o["dpred"], rand(3, 333, channels, seed=8).double() * coef) <= 1e-6


def run_ksse(alloc, channels, dc, hf, noise, off, short=False):
    lib, t = _native.lib(), Taker(alloc, off)
    pred, tgt, k0, mask = kspace_inputs(3, 333, channels, dc)
    p, tg, k, m = t.inp("pred", pred), t.inp("tgt", tgt), t.inp("k0", k0), t.inp("mask", mask)
    h = t.inp("hf", (rand(333, seed=9) > -0.5).float()) if hf else None
    g = t.inp("g", torch.tensor([1.5]))
    out = {"d": t.out("d", pred.shape), "loss": t.out("loss", (1,))}
    ws, wsn = t.loss_ws()
    rc = lib.siren_kspace_sse_forward(ptr(p), ptr(k), ptr(m), ptr(tg), ptr(h), 3, 333, channels, noise, 0.25,
                                      ptr(out["d"]), ptr(out["loss"]), ptr(ws), wsn - short, stream())
    if short:
        return rc
    ok(rc)
    alloc.freeze("d")
    out["dpred"] = t.out("dpred", pred.shape)
    ok(lib.siren_kspace_sse_backward(ptr(out["d"]), ptr(m), ptr(h), 3, 333, channels, noise, ptr(g), 0.5,
                                     ptr(out["dpred"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("dc,hf,noise", [(False, False, 0.0), (True, True, 0.0), (True, False, 0.25), (False, True, 0.0)])
@pytest.mark.parametrize("channels", [1, 2])
def test_kspace_sse(channels, dc, hf, noise, off):
    o = both(run_ksse, channels, dc, hf, noise, off)
    pred, tgt, k0, mask = kspace_inputs(3, 333, channels, dc)
    y, coef = dc64(pred, k0, mask, noise)
    h = (rand(333, seed=9) > -0.5).double().reshape(1, -1, 1) if hf else 1.0
    d = h * (y - tgt.double())
    assert orc.norm_rel(o["d"], d) <= 1e-6
    assert float(o["loss"]) == pytest.approx(0.25 * float((d ** 2).sum()), rel=1e-5)
    assert orc.norm_rel(o["dpred"], 1.5 * 0.5 * h * d * coef) <= 1e-6


def test_kspace_sse_short_workspace_is_refused_before_any_launch():
    refused(run_ksse, 2, True, True, 0.0, 0)


# ---------------------------------------------------------------------- the k-space loss family
KDESC = (1.0 / 128 ** 2, 1e-3, 400.0, 6.7, 1e-4, 1e-4)


def run_kloss(alloc, kind, channels, dc, off, short=False):
    lib, t = _native.lib(), Taker(alloc, off)
    pred, tgt, k0, mask = kspace_inputs(3, 333, channels, dc)
    pred, tgt = 0.3 * pred, 0.3 * tgt
    p, tg, k, m = t.inp("pred", pred), t.inp("tgt", tgt), t.inp("k0", k0), t.inp("mask", mask)
    g = t.inp("g", torch.tensor([1.5]))
    out = {"loss": t.out("loss", (1,)), "dpred": t.out("dpred", pred.shape)}
    ws, wsn = t.loss_ws()
    desc = _native.SirenKlossDesc(*KDESC)
    rc = lib.siren_kspace_loss_forward(kind, ctypes.byref(desc), ptr(p), ptr(k), ptr(m), ptr(tg), 3, 333, channels, 0.25,
                                       ptr(out["loss"]), ptr(ws), wsn - short, stream())
    if short:
        return rc
    ok(rc)
    ok(lib.siren_kspace_loss_backward(kind, ctypes.byref(desc), ptr(p), ptr(k), ptr(m), ptr(tg), 3, 333, channels, 0.25,
                                      ptr(g), ptr(out["dpred"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("dc", [False, True])
@pytest.mark.parametrize("kind", range(_native.KLOSS_KINDS))
def test_kspace_loss(kind, dc, off):
    channel_sets = (2,) if kind in (_native.KLOSS_PERP, _native.KLOSS_LOG) else (1, 2)
    for channels in channel_sets:
        o = both(run_kloss, kind, channels, dc, off)
        assert torch.isfinite(o["loss"]).all() and float(o["loss"]) > 0 and torch.isfinite(o["dpred"]).all()
        if kind == _native.KLOSS_L1:  # the one whose float64 value is a line: weight sum |y - t|
            pred, tgt, k0, mask = kspace_inputs(3, 333, channels, dc)
            y, coef = dc64(0.3 * pred, k0, mask, 0.25)
            assert float(o["loss"]) == pytest.approx(KDESC[0] * float((y - 0.3 * tgt.double()).abs().sum()), rel=1e-5)
            assert orc.norm_rel(o["dpred"], 1.5 * KDESC[0] * torch.sign(y - 0.3 * tgt.double()) * coef) <= 1e-6


def test_kspace_loss_short_workspace_is_refused_before_any_launch():
    refused(run_kloss, _native.KLOSS_L1, 2, True, 0)


# ---------------------------------------------------------------------- FFT and the image-domain loss
def run_fft2(alloc, side, inverse, off):
    t = Taker(alloc, off)
    x = t.inp("x", rand(3, side * side, 2, seed=10))
    out = {"out": t.out("out", (3, side * side, 2))}
    ok(_native.lib().siren_kspace_fft2(ptr(x), ptr(out["out"]), 3, side, inverse, stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("side", _native.KFFT_SIDES)
def test_fft2(side, inverse, off):
    o = both(run_fft2, side, inverse, off)
    x = rand(3, side * side, 2, seed=10).double()
    c = torch.complex(x[..., 0], x[..., 1]).reshape(3, side, side)
    r = torch.view_as_real((torch.fft.ifft2 if inverse else torch.fft.fft2)(c)).reshape(3, side * side, 2)
    assert orc.norm_rel(o["out"], r) <= 1e-6


def ift_inputs(batch, side, mask_kind, dc):
    n = side * side
    amp = 0.5 * torch.exp(-3.0 * torch.rand(batch, n, 1, generator=torch.Generator().manual_seed(side)))
    pred, tgt = amp * rand(batch, n, 2, seed=11), amp * rand(batch, n, 2, seed=12)
    k0 = amp.permute(0, 2, 1) * rand(batch, 2, n, seed=13) if dc else None
    mask = (rand(batch, 2, n, seed=14) > 0.4).float() if dc else None
    im = {"none": None, "hw": (rand(side, side, seed=15) > -0.3).float(),
          "bhw": (rand(batch, side, side, seed=16) > -0.3).float()}[mask_kind]
    return pred, tgt, k0, mask, im


def run_ift(alloc, batch, side, mask_kind, dc, off, short=False):
    lib, t = _native.lib(), Taker(alloc, off)
    pred, tgt, k0, mask, im = ift_inputs(batch, side, mask_kind, dc)
    p, tg, k, m, i = t.inp("pred", pred), t.inp("tgt", tgt), t.inp("k0", k0), t.inp("mask", mask), t.inp("img_mask", im)
    g = t.inp("g", torch.tensor([1.5]))
    stride = side * side if mask_kind == "bhw" else 0
    out = {"loss": t.out("loss", (1,)), "dpred": t.out("dpred", pred.shape)}
    ws, wsn = t.loss_ws()
    desc = _native.SirenKiftDesc(1.0, 1e-8, 0.0025)
    rc = lib.siren_kspace_ift_loss_forward(ctypes.byref(desc), ptr(p), ptr(k), ptr(m), ptr(tg), ptr(i), stride, batch, side,
                                           0.25 if dc else 0.0, ptr(out["loss"]), ptr(ws), wsn - short, stream())
    if short:
        return rc
    ok(rc)
    ok(lib.siren_kspace_ift_loss_backward(ctypes.byref(desc), ptr(p), ptr(k), ptr(m), ptr(tg), ptr(i), stride, batch, side,
                                          0.25 if dc else 0.0, ptr(g), ptr(out["dpred"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("mask_kind", ["none", "hw", "bhw"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("side", [8, 128])
def test_ift_loss(side, batch, mask_kind, off):
    for dc in (False, True):
        o = both(run_ift, batch, side, mask_kind, dc, off)
        pred, tgt, k0, mask, im = ift_inputs(batch, side, mask_kind, dc)
        p = pred.double().requires_grad_(True)
        y = dc64(p, k0, mask, 0.25)[0] if dc else p
        cy = torch.complex(y[..., 0], y[..., 1]).reshape(batch, side, side)
        ct = torch.complex(tgt.double()[..., 0], tgt.double()[..., 1]).reshape(batch, side, side)
        img = (torch.fft.ifft2(cy).abs() - torch.fft.ifft2(ct).abs()) ** 2
        img = img * im.double() if im is not None else img
        loss = img.sum() + 1e-8 * cy.abs().sum() + 0.0025 * ((y - tgt.double()) ** 2).sum()
        (1.5 * loss).backward()
        assert float(o["loss"]) == pytest.approx(float(loss.detach()), rel=1e-4)
        assert orc.norm_rel(o["dpred"], p.grad) <= 1e-4


def test_ift_loss_short_workspace_is_refused_before_any_launch():
    refused(run_ift, 3, 8, "hw", True, 0)


# ---------------------------------------------------------------------- Fourier features, sin / cos probe
def run_fourier(alloc, off):
    t = Taker(alloc, off)
    x, B = t.inp("x", torch.rand(333, 2, generator=torch.Generator().manual_seed(1)) * 2 - 1), t.inp("B", rand(2, 60, seed=17))
    out = {"out": t.out("out", (333, 120))}
    ok(_native.lib().siren_fourier_features(ptr(x), ptr(B), 333, 2, 60, ptr(out["out"]), stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
def test_fourier_features(off):
    o = both(run_fourier, off)
    x = (torch.rand(333, 2, generator=torch.Generator().manual_seed(1)) * 2 - 1).double()
    ref = orc.fourier_features(x[None], rand(2, 60, seed=17).double())[0]
    # fp32 arguments |2 pi x B| below 64 (ulp 7.6e-6): a few roundings of the argument, in absolute terms
    assert float((o["out"].double() - ref).abs().max()) <= 3e-5


def run_sincos(alloc, impl, off):
    t = Taker(alloc, off)
    x = t.inp("x", 40.0 * rand(1001, seed=18))
    out = {"s": t.out("s", (1001,)), "c": t.out("c", (1001,))}
    ok(_native.lib().siren_sincos_f32(ptr(x), ptr(out["s"]), ptr(out["c"]), 1001, impl, stream()))
    return out


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("impl", [0, 1])
def test_sincos(impl, off):
    o = both(run_sincos, impl, off)
    x = (40.0 * rand(1001, seed=18)).double()
    assert float((o["s"].double() - torch.sin(x)).abs().max()) <= 1e-6
    assert float((o["c"].double() - torch.cos(x)).abs().max()) <= 1e-6
