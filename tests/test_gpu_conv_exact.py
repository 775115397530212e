"""GPU: the conv encoder's MFMA kernels (siren_conv.hip) on data where every summation order gives the
same bits (tests/_exact.py; the conditions are asserted on the CPU by tests/test_exact_cpu.py). The fp64
convolution followed by the roundings include/siren_mri_amd.h documents must equal the kernel's output
element for element: every assertion in this file is torch.equal, and a failure says where the differing
elements lie (mismatch_report: per image, row, column, channel).

  forward, 64 / 128 input channels  siren_conv_fwd_k5 (conv_fwd_k5_kernel: conv_dma 0, 1, 2) and
      siren_conv_fwd (conv_fwd_gen_kernel: conv_dma 0 and 2) at (N, H) = (3, 10): a workgroup whose
      input rows all lie inside the image, top and bottom halos, two image boundaries, and (1, 2): every
      stage holds rows outside the image; 1, 2 or 3 tiles of output channels
  forward, 2 input channels         conv_t_fwd_kernel at (3, 5) (15 rows, 4 a workgroup: a ragged last
      workgroup, workgroups that straddle images), (1, 1) and (2, 8)
  fused epilogues                   siren_conv_fwd_k5_res and siren_conv_dgrad_k5_fused against torch, with
      masks that hold zeros; at (129, 4) the 258 partial rows take conv_chan_reduce_kernel round its loop
  weight gradients                  siren_conv_wrw_k5 / siren_conv_wrw in every wrw_dma form at W = 256 (two
      128-pixel chunks per row) and W = 192 (the 64-pixel form)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact as E  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


class option:
    """A process-wide option for the length of a with block."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = _native.get_option(self.key)
        _native.set_option(self.key, self.value)

    def __exit__(self, *exc):
        _native.set_option(self.key, self.old)
        return False


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream():
    return _native.stream_handle(DEV)


def ok(rc):
    assert rc == 0, _native.last_error()


def dev(t):
    return t.contiguous().to(DEV)


def poisoned(shape, dtype=BF16):
    """An output buffer of NaNs: an element the kernel leaves out cannot equal the reference."""
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_forward(c, N, H, bias, relu, k5):
    lib = _native.lib()
    y = poisoned((N, H, E.W_FWD, c.co))
    x, w, b = dev(c.x), dev(c.w), dev(c.bias) if bias else None
    if k5:
        ok(lib.siren_conv_fwd_k5(ptr(x), ptr(w), ptr(b), int(relu), ptr(y), N, H, E.W_FWD, 128, stream()))
    else:
        ok(lib.siren_conv_fwd(ptr(x), ptr(w), ptr(b), int(relu), ptr(y), N, H, E.W_FWD, c.ci, c.co, c.k, stream()))
    return y


# ---------------------------------------------------------------------- forward, 64 / 128 input channels
@pytest.mark.parametrize("bias,relu", E.BIAS_RELU)
@pytest.mark.parametrize("recipe", E.RECIPES)
@pytest.mark.parametrize("N,H", E.FWD_NH)
def test_conv_fwd_k5_exact(N, H, recipe, bias, relu):
    c = E.forward_case(recipe, *E.FWD_K5, N, H)
    ref = E.forward_ref(c.acc, c.bias if bias else None, relu)
    for dma in (0, 1, 2):
        with option("conv_dma", dma):
            y = run_forward(c, N, H, bias, relu, k5=True)
        E.assert_equal(y, ref, f"siren_conv_fwd_k5, conv_dma {dma}, {recipe}")


@pytest.mark.parametrize("bias,relu", E.BIAS_RELU)
@pytest.mark.parametrize("recipe", E.RECIPES)
@pytest.mark.parametrize("N,H", E.FWD_NH)
@pytest.mark.parametrize("k,ci,co", E.FWD_GEN)
def test_conv_fwd_exact(k, ci, co, N, H, recipe, bias, relu):
    assert _native.lib().siren_conv_check(0, N, H, E.W_FWD, ci, co, k) == 0, _native.last_error()
    c = E.forward_case(recipe, k, ci, co, N, H)
    ref = E.forward_ref(c.acc, c.bias if bias else None, relu)
    for dma in (0, 2):  # the two stage fills conv_fwd_gen_kernel has
        with option("conv_dma", dma):
            y = run_forward(c, N, H, bias, relu, k5=False)
        E.assert_equal(y, ref, f"siren_conv_fwd {k}x{k} {ci} -> {co}, conv_dma {dma}, {recipe}")


# ---------------------------------------------------------------------- forward, 2 input channels
@pytest.mark.parametrize("bias,relu", E.BIAS_RELU)
@pytest.mark.parametrize("recipe", E.RECIPES)
@pytest.mark.parametrize("N,H", E.FWD_T_NH)
@pytest.mark.parametrize("k,ci,co", E.FWD_T)
def test_conv_theta_fwd_exact(k, ci, co, N, H, recipe, bias, relu):
    assert _native.lib().siren_conv_check(0, N, H, E.W_FWD, ci, co, k) == 0, _native.last_error()
    c = E.forward_case(recipe, k, ci, co, N, H)
    ref = E.forward_ref(c.acc, c.bias if bias else None, relu)
    y = run_forward(c, N, H, bias, relu, k5=False)
    E.assert_equal(y, ref, f"siren_conv_fwd {k}x{k} 2 -> {co}, {recipe}")


# ---------------------------------------------------------------------- fused epilogues
def run_res(c, N, H):
    a, out = poisoned((N, H, E.W_FWD, 128)), poisoned((N, H, E.W_FWD, 128))
    x, w, cb, t = dev(c.x), dev(c.w), dev(c.cb), dev(c.t)
    ok(_native.lib().siren_conv_fwd_k5_res(ptr(x), ptr(w), ptr(cb), ptr(t), ptr(a), ptr(out), N, H, E.W_FWD, 128, stream()))
    return a, out


@pytest.mark.parametrize("dma", [0, 1, 2])
@pytest.mark.parametrize("recipe", E.RECIPES)
def test_conv_fwd_k5_res_exact(recipe, dma):
    N, H = E.EPI_NH
    c = E.epilogue_case(recipe, N, H)
    a_ref, out_ref = E.res_ref(c)
    with option("conv_dma", dma):
        a, out = run_res(c, N, H)
    E.assert_equal(a, a_ref, f"siren_conv_fwd_k5_res a_out, conv_dma {dma}, {recipe}")
    E.assert_equal(out, out_ref, f"siren_conv_fwd_k5_res out, conv_dma {dma}, {recipe}")


def run_dgrad(c, N, H, mode, with_g2):
    shape = (N, H, E.W_FWD, 128)
    nblk = N * (H // 2)
    ws = torch.full((nblk * 128 * 4,), 0xFF, dtype=U8, device=DEV)  # nblk * 128 floats, as the header says
    o = {"out": poisoned(shape), "db": poisoned((128,), F32)}
    if mode == 2:
        o["out2"] = poisoned(shape)
    dy, w, m = dev(c.x), dev(c.w), dev(c.m)
    g2 = dev(c.g2) if (with_g2 or mode == 2) else None
    pa, cb = (dev(c.pa), dev(c.cb)) if mode == 2 else (None, None)
    ok(_native.lib().siren_conv_dgrad_k5_fused(mode, ptr(dy), ptr(w), ptr(g2), ptr(m), ptr(pa), ptr(cb), ptr(o["out"]),
                                               ptr(o.get("out2")), ptr(o["db"]), N, H, E.W_FWD, 128, ptr(ws), ws.numel(),
                                               stream()))
    return o


def check_dgrad(c, N, H, mode, with_g2, what):
    ref = E.dgrad_ref(c, mode, with_g2)
    o = run_dgrad(c, N, H, mode, with_g2)
    E.assert_equal(o["out"], ref["out"], f"{what}: out")
    if mode == 2:
        E.assert_equal(o["out2"], ref["out2"], f"{what}: out2")
    E.assert_equal(o["db"], ref["db"].float(), f"{what}: db", dims=("c",))


@pytest.mark.parametrize("dma", [0, 1, 2])
@pytest.mark.parametrize("mode,with_g2", [(1, False), (1, True), (2, True)])
@pytest.mark.parametrize("recipe", E.RECIPES)
def test_conv_dgrad_k5_fused_exact(recipe, mode, with_g2, dma):
    N, H = E.EPI_NH
    c = E.epilogue_case(recipe, N, H)
    with option("conv_dma", dma):
        check_dgrad(c, N, H, mode, with_g2, f"siren_conv_dgrad_k5_fused mode {mode}, g2 {with_g2}, conv_dma {dma}, {recipe}")


@pytest.mark.parametrize("mode", [1, 2])
def test_conv_dgrad_k5_fused_258_workgroups_exact(mode):
    """(N, H) = (129, 4): conv_chan_reduce_kernel's threads 0 and 1 add a second partial row."""
    N, H = E.EPI_BIG_NH
    c = E.epilogue_case("lossless", N, H)
    check_dgrad(c, N, H, mode, True, f"siren_conv_dgrad_k5_fused mode {mode} at 258 workgroups")


# ---------------------------------------------------------------------- weight gradients
@pytest.mark.parametrize("N,H,W", E.WRW_NHW)
def test_conv_wrw_k5_exact(N, H, W):
    lib = _native.lib()
    c = E.wrw_case("rounding", *E.FWD_K5, N, H, W)
    x, dy, ref = dev(c.x), dev(c.dy), c.dw.float()
    wsn = int(lib.siren_conv_wrw_workspace_bytes(N, H, W))
    for dma in (0, 1, 2):
        ws = torch.full((wsn,), 0xFF, dtype=U8, device=DEV)
        dw = poisoned((128, 5, 5, 128), F32)
        with option("wrw_dma", dma):
            ok(lib.siren_conv_wrw_k5(ptr(x), ptr(dy), N, H, W, 128, ptr(dw), ptr(ws), wsn, stream()))
        E.assert_equal(dw, ref, f"siren_conv_wrw_k5, wrw_dma {dma}, W {W}", dims=("co", "kh", "kw", "ci"))


@pytest.mark.parametrize("N,H,W", E.WRW_NHW)
@pytest.mark.parametrize("k,ci,co", E.WRW_GEN)
def test_conv_wrw_exact(k, ci, co, N, H, W):
    lib = _native.lib()
    assert lib.siren_conv_check(1, N, H, W, ci, co, k) == 0, _native.last_error()
    c = E.wrw_case("rounding", k, ci, co, N, H, W)
    x, dy, ref = dev(c.x), dev(c.dy), c.dw.float()
    wsn = int(lib.siren_conv_wrw_ws_bytes(N, H, W, ci, co, k))
    for dma in (_native.get_option("wrw_dma"), 3):  # the default, and the 128-pixel LDS-DMA form
        ws = torch.full((wsn,), 0xFF, dtype=U8, device=DEV)
        dw = poisoned((co, k, k, ci), F32)
        with option("wrw_dma", dma):
            ok(lib.siren_conv_wrw(ptr(x), ptr(dy), N, H, W, ci, co, k, ptr(dw), ptr(ws), wsn, stream()))
        E.assert_equal(dw, ref, f"siren_conv_wrw {k}x{k} {ci} -> {co}, wrw_dma {dma}, W {W}", dims=("co", "kh", "kw", "ci"))
