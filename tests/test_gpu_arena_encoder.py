"""GPU: the encoder passes and convolutions (siren_enc_*, siren_conv_*), the hypernetwork heads
(siren_hyper_*), the sum of squares (siren_sumsq_*) and Adam (siren_adam_step and its scalar launches) on
a poisoned arena (tests/_arena.py): every operand exactly as long as the ABI says, the workspaces exactly
their *_bytes() queries, NaN bytes and 64 KiB guards all round.

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs), I3 (outputs written in full), I4 (the encoder workspace's ticket word and the whole
sum-of-squares workspace are zero again) hold, and I5 every output is bit-equal to the plain run (all of
these sum in fixed orders: test_native_passes_deterministic, the run-to-run assertions of
test_gpu_encoder.py, test_native_heads_deterministic, test_hypo_weight_loss_native_sum_of_squares). I7: a
workspace one byte short is refused with SIREN_ENOSPACE before any launch, and a forward convolution
asked for a ReLU without a bias with SIREN_EINVAL. The arena run is also compared
with torch on the same operands, at the bounds of test_gpu_encoder.py / test_gpu_hyper.py /
test_gpu_optim.py, so the two runs cannot be wrong together; the fused convolution epilogues
(siren_conv_fwd_k5_res, siren_conv_dgrad_k5_fused) are compared with the separate passes bit for bit, as
test_fused_dgrad_epilogues_match_the_passes does end to end."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _arena import Plain, same_bits  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
EINVAL = -1
F32, BF16, U8, F64 = torch.float32, torch.bfloat16, torch.uint8, torch.float64


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
    return b


def refused(driver, *args):
    plain = Plain(DEV)
    driver(plain, *args)
    arena = plain.arena()
    assert driver(arena, *args, short=True) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream():
    return _native.stream_handle(DEV)


def ok(rc):
    assert rc == 0, _native.last_error()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def inp(alloc, name, t, off=0):
    return alloc.take(t.shape, t.dtype, role="input", fill=t, name=name, offset_bytes=off)


def enc_ws(alloc):
    """siren_enc_workspace_bytes: partial sums (scratch that launches overwrite), then the ticket word."""
    n = int(_native.lib().siren_enc_workspace_bytes())
    return alloc.take((n,), U8, role="zeroed", name="enc_ws", zero_check=(n - 256, n - 252)), n


class options:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: _native.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            _native.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _native.set_option(k, v)
        return False


# ---------------------------------------------------------------------- the [P, C] passes
def plane_inputs(C, P):
    g = gen(C + P)
    mk = lambda: torch.randn(P, C, generator=g).to(BF16)  # noqa: E731
    return {"g1": mk(), "g2": mk(), "y": mk(), "a": mk(), "x": mk(), "cb": torch.randn(C, generator=g).to(BF16)}


def run_planes(alloc, C, P, with_g2, short=False):
    lib, st = _native.lib(), stream()
    t = {k: inp(alloc, k, v) for k, v in plane_inputs(C, P).items()}
    g2 = t["g2"] if with_g2 else None
    ws, wsn = enc_ws(alloc)
    o = {k: alloc.take(s, d, role="output", name=k) for k, s, d in
         [("relu_out", (P, C), BF16), ("relu_db", (C,), F32)]}
    rc = lib.siren_enc_relu_bwd(ptr(t["g1"]), ptr(g2), ptr(t["y"]), ptr(o["relu_out"]), ptr(o["relu_db"]), P, C, ptr(ws),
                                wsn - short, st)
    if short:
        return rc
    ok(rc)
    o.update({k: alloc.take(s, d, role="output", name=k) for k, s, d in
              [("res_out", (P, C), BF16), ("gskip", (P, C), BF16), ("ga", (P, C), BF16), ("res_db", (C,), F32)]})
    ok(lib.siren_enc_res_fwd(ptr(t["a"]), ptr(t["cb"]), ptr(t["x"]), ptr(o["res_out"]), P, C, st))
    alloc.freeze("res_out")
    ok(lib.siren_enc_res_bwd(ptr(t["g1"]), ptr(g2), ptr(o["res_out"]), ptr(t["a"]), ptr(t["cb"]), ptr(o["gskip"]),
                             ptr(o["ga"]), ptr(o["res_db"]), P, C, ptr(ws), wsn, st))
    o["bias_relu"] = alloc.take((P, C), BF16, role="scratch", fill=plane_inputs(C, P)["a"], name="bias_relu")  # in place
    ok(lib.siren_enc_bias_relu(ptr(o["bias_relu"]), ptr(t["cb"]), P, C, st))
    return o


@pytest.mark.parametrize("with_g2", [True, False])
@pytest.mark.parametrize("C,P", [(8, 333), (128, 4097)])
def test_plane_passes(C, P, with_g2):
    o = both(run_planes, C, P, with_g2)
    t = {k: v.to(DEV) for k, v in plane_inputs(C, P).items()}
    gsum = t["g1"] + t["g2"] if with_g2 else t["g1"]
    ref = (gsum * (t["y"] > 0)).to(BF16)
    assert torch.equal(o["relu_out"], ref)
    torch.testing.assert_close(o["relu_db"], ref.float().sum(0), rtol=1e-5, atol=1e-4)
    ab = t["a"] + t["cb"]
    assert torch.equal(o["res_out"], torch.relu(torch.relu(ab) + t["x"]))
    s_ref = (gsum * (o["res_out"] > 0)).to(BF16)
    assert torch.equal(o["gskip"], s_ref) and torch.equal(o["ga"], s_ref * (ab > 0))
    torch.testing.assert_close(o["res_db"], o["ga"].float().sum(0), rtol=1e-5, atol=1e-4)
    assert torch.equal(o["bias_relu"], torch.relu(ab))


def test_plane_pass_short_workspace_is_refused_before_any_launch():
    refused(run_planes, 8, 333, True)


def pixfc_inputs(B, P, C):
    g = gen(B + P + C)
    return {"a": torch.randn(B, P, C, generator=g).to(BF16), "cb": torch.randn(C, generator=g).to(BF16),
            "w": torch.randn(P, generator=g) / 128, "bias": torch.randn(1, generator=g), "g": torch.randn(B, C, generator=g)}


def run_pixfc(alloc, B, P, C, short=False):
    lib, st = _native.lib(), stream()
    t = {k: inp(alloc, k, v) for k, v in pixfc_inputs(B, P, C).items()}
    ws, wsn = enc_ws(alloc)
    o = {"e": alloc.take((B, C), F32, role="output", name="e")}
    rc = lib.siren_enc_pixfc_fwd(ptr(t["a"]), ptr(t["cb"]), ptr(t["w"]), ptr(t["bias"]), ptr(o["e"]), B, P, C, ptr(ws),
                                 wsn - short, st)
    if short:
        return rc
    ok(rc)
    o.update({k: alloc.take(s, d, role="output", name=k) for k, s, d in
              [("ga", (B, P, C), BF16), ("db", (C,), F32), ("gw", (P,), F32)]})
    ok(lib.siren_enc_pixfc_bwd(ptr(t["g"]), ptr(t["a"]), ptr(t["cb"]), ptr(t["w"]), ptr(o["ga"]), ptr(o["db"]), ptr(o["gw"]),
                               B, P, C, ptr(ws), wsn, st))
    return o


@pytest.mark.parametrize("B,P,C", [(5, 333, 8), (2, 16384, 128)])
def test_pixfc_passes(B, P, C):
    o = both(run_pixfc, B, P, C)
    t = {k: v.to(DEV) for k, v in pixfc_inputs(B, P, C).items()}
    ab = t["a"] + t["cb"]
    r = torch.relu(ab.float())
    torch.testing.assert_close(o["e"], torch.einsum("bpc,p->bc", r, t["w"]) + t["bias"], rtol=1e-4, atol=1e-4)
    ga_ref = ((ab.float() > 0) * t["g"][:, None, :] * t["w"].reshape(1, P, 1)).to(BF16)
    assert torch.equal(o["ga"], ga_ref)
    torch.testing.assert_close(o["db"], ga_ref.float().sum((0, 1)), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(o["gw"], torch.einsum("bc,bpc->p", t["g"], r), rtol=1e-4, atol=1e-3)


def test_pixfc_short_workspace_is_refused_before_any_launch():
    refused(run_pixfc, 5, 333, 8)


# ---------------------------------------------------------------------- siren_enc_prep
PREP = [(64, 2, 7), (128, 64, 7), (128, 128, 5)]  # conv_theta, cnn[0], a residual block's convolution


def prep_inputs():
    g = gen(77)
    return [(torch.randn(co, ci, k, k, generator=g), torch.randn(co, generator=g)) for co, ci, k in PREP]


def run_prep(alloc):
    lib, n = _native.lib(), len(PREP)
    wb_in = [(inp(alloc, f"w{i}", w), inp(alloc, f"b{i}", b)) for i, (w, b) in enumerate(prep_inputs())]
    o = {}
    geom = (ctypes.c_int64 * (7 * n))()
    for i, (co, ci, k) in enumerate(PREP):
        geom[7 * i:7 * i + 7] = [co, ci, k, ci * k * k, k * k, k, 1]  # a contiguous [co][ci][kh][kw] filter
        o[f"wb{i}"] = alloc.take((co, k, k, ci), BF16, role="output", name=f"wb{i}")
        if i:  # no input gradient through conv_theta
            o[f"wf{i}"] = alloc.take((ci, k, k, co), BF16, role="output", name=f"wf{i}")
        o[f"bb{i}"] = alloc.take((co,), BF16, role="output", name=f"bb{i}")
    VP = ctypes.c_void_p * n
    ok(lib.siren_enc_prep(n, VP(*[ptr(w) for w, _ in wb_in]), VP(*[ptr(b) for _, b in wb_in]), geom,
                          VP(*[ptr(o[f"wb{i}"]) for i in range(n)]), VP(*[ptr(o.get(f"wf{i}")) for i in range(n)]),
                          VP(*[ptr(o[f"bb{i}"]) for i in range(n)]), stream()))
    return o


def test_enc_prep():
    o = both(run_prep)
    for i, (w, b) in enumerate(prep_inputs()):
        wb = w.to(DEV).to(BF16)
        assert torch.equal(o[f"wb{i}"], wb.permute(0, 2, 3, 1)) and torch.equal(o[f"bb{i}"], b.to(DEV).to(BF16))
        if i:  # [ci][k-1-kh][k-1-kw][co]
            assert torch.equal(o[f"wf{i}"], wb.flip(2, 3).permute(1, 2, 3, 0))


# ---------------------------------------------------------------------- convolutions (bf16 NHWC)
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_inputs(N, H, W, ci, co, k, seed=0):
    g = gen(1000 * k + ci + co + H + seed)
    x = torch.randn(N, ci, H, W, generator=g).to(BF16)
    w = (torch.randn(co, ci, k, k, generator=g) / (ci * k)).to(BF16)
    return x, w, torch.randn(co, generator=g).to(BF16), torch.randn(N, co, H, W, generator=g).to(BF16)


def run_conv_fwd(alloc, ci, co, k, bias, relu, k5, refuse=False):
    lib = _native.lib()
    N, H = (2, 5) if ci == 2 else (2, 6)
    x, w, b, _ = conv_inputs(N, H, 128, ci, co, k)
    xd, wd, bd = inp(alloc, "x", nhwc(x)), inp(alloc, "w", nhwc(w)), inp(alloc, "bias", b)
    o = {"y": alloc.take((N, H, 128, co), BF16, role="output", name="y")}
    if refuse:  # relu without a bias: the ReLU lives in the bias epilogue, so the call is refused
        return (lib.siren_conv_fwd_k5(ptr(xd), ptr(wd), None, 1, ptr(o["y"]), N, H, 128, 128, stream()) if k5 else
                lib.siren_conv_fwd(ptr(xd), ptr(wd), None, 1, ptr(o["y"]), N, H, 128, ci, co, k, stream()))
    if k5:
        ok(lib.siren_conv_fwd_k5(ptr(xd), ptr(wd), ptr(bd) if bias else None, int(relu), ptr(o["y"]), N, H, 128, 128, stream()))
    else:
        ok(lib.siren_conv_fwd(ptr(xd), ptr(wd), ptr(bd) if bias else None, int(relu), ptr(o["y"]), N, H, 128, ci, co, k,
                              stream()))
    return o


@pytest.mark.parametrize("dma", [0, 1, 2])
@pytest.mark.parametrize("bias,relu", [(False, False), (True, True)])
@pytest.mark.parametrize("ci,co,k,k5", [(128, 128, 5, True), (128, 128, 5, False), (64, 128, 7, False), (128, 64, 3, False),
                                        (2, 64, 7, False), (2, 96, 3, False)])
def test_conv_forward(ci, co, k, k5, bias, relu, dma):
    with options(conv_dma=dma):
        o = both(run_conv_fwd, ci, co, k, bias, relu, k5)
    N, H = (2, 5) if ci == 2 else (2, 6)
    x, w, b, _ = conv_inputs(N, H, 128, ci, co, k)
    ref = F.conv2d(x.double(), w.double(), padding=k // 2).to(BF16)
    if bias:
        ref = ref + b.view(1, -1, 1, 1)
        ref = torch.relu(ref) if relu else ref
    got = o["y"].cpu().permute(0, 3, 1, 2).float()
    assert orc.norm_rel(got, ref.float()) < 4e-3  # test_gpu_encoder.py: at most one bf16 rounding step apart
    assert ((got - ref.float()).abs() <= ref.float().abs() * 2 ** -7 + 1e-6).float().mean() > 0.999


@pytest.mark.parametrize("ci,co,k,k5", [(128, 128, 5, True), (128, 128, 5, False), (64, 128, 7, False), (2, 64, 7, False)])
def test_conv_forward_relu_without_bias_is_refused_before_any_launch(ci, co, k, k5):
    """include/siren_mri_amd.h: relu != 0 with a NULL bias is SIREN_EINVAL (the kernels would skip the
    ReLU silently), with a last_error text and nothing launched."""
    plain = Plain(DEV)
    run_conv_fwd(plain, ci, co, k, True, True, k5)
    arena = plain.arena()
    assert run_conv_fwd(arena, ci, co, k, False, True, k5, refuse=True) == EINVAL
    assert "relu needs a bias" in _native.last_error()
    arena.assert_nothing_launched()


def res_inputs():
    N, H = 2, 6
    x, w, cb, dy = conv_inputs(N, H, 128, 128, 128, 5, seed=3)
    g = gen(5)
    mk = lambda: torch.randn(N, H, 128, 128, generator=g).to(BF16)  # noqa: E731
    return {"x": nhwc(x), "w": nhwc(w / 4), "cb": cb, "dy": nhwc(dy), "t": mk(), "g2": mk(), "m": mk(), "pa": mk()}


def run_conv_res(alloc):
    """siren_conv_fwd_k5_res, and its two separate passes."""
    lib, st, shape = _native.lib(), stream(), (2, 6, 128, 128)
    t = {k: inp(alloc, k, v) for k, v in res_inputs().items() if k in ("x", "w", "cb", "t")}
    o = {k: alloc.take(shape, BF16, role="output", name=k) for k in ("a_fused", "out_fused", "a_sep", "out_sep")}
    ok(lib.siren_conv_fwd_k5_res(ptr(t["x"]), ptr(t["w"]), ptr(t["cb"]), ptr(t["t"]), ptr(o["a_fused"]), ptr(o["out_fused"]),
                                 2, 6, 128, 128, st))
    ok(lib.siren_conv_fwd_k5(ptr(t["x"]), ptr(t["w"]), None, 0, ptr(o["a_sep"]), 2, 6, 128, 128, st))
    alloc.freeze("a_sep")
    ok(lib.siren_enc_res_fwd(ptr(o["a_sep"]), ptr(t["cb"]), ptr(t["t"]), ptr(o["out_sep"]), 2 * 6 * 128, 128, st))
    return o


@pytest.mark.parametrize("dma", [0, 1, 2])
def test_conv_fwd_k5_res_equals_the_passes(dma):
    with options(conv_dma=dma):
        o = both(run_conv_res)
    assert torch.equal(o["a_fused"], o["a_sep"]) and torch.equal(o["out_fused"], o["out_sep"])
    assert bool((o["out_fused"] > 0).any()) and bool((o["out_fused"] == 0).any())


def run_dgrad(alloc, mode, with_g2, short=False):
    """siren_conv_dgrad_k5_fused, and the input-gradient convolution followed by the separate pass."""
    lib, st, shape, P = _native.lib(), stream(), (2, 6, 128, 128), 2 * 6 * 128
    t = {k: inp(alloc, k, v) for k, v in res_inputs().items() if k in ("dy", "w", "cb", "g2", "m", "pa")}
    g2 = t["g2"] if (with_g2 or mode == 2) else None
    wsn = 2 * 3 * 128 * 4  # N * H / 2 * 128 floats (include/siren_mri_amd.h)
    ws = alloc.take((wsn,), U8, role="scratch", name="dgrad_ws")
    o = {"out": alloc.take(shape, BF16, role="output", name="out"), "db": alloc.take((128,), F32, role="output", name="db")}
    if mode == 2:
        o["out2"] = alloc.take(shape, BF16, role="output", name="out2")
    rc = lib.siren_conv_dgrad_k5_fused(mode, ptr(t["dy"]), ptr(t["w"]), ptr(g2), ptr(t["m"]), ptr(t["pa"]), ptr(t["cb"]),
                                       ptr(o["out"]), ptr(o.get("out2")), ptr(o["db"]), 2, 6, 128, 128, ptr(ws), wsn - short, st)
    if short:
        return rc
    ok(rc)
    ews, ewsn = enc_ws(alloc)
    o["g_sep"] = alloc.take(shape, BF16, role="output", name="g_sep")
    ok(lib.siren_conv_fwd_k5(ptr(t["dy"]), ptr(t["w"]), None, 0, ptr(o["g_sep"]), 2, 6, 128, 128, st))
    alloc.freeze("g_sep")
    o["out_sep"] = alloc.take(shape, BF16, role="output", name="out_sep")
    o["db_sep"] = alloc.take((128,), F32, role="output", name="db_sep")
    if mode == 1:
        ok(lib.siren_enc_relu_bwd(ptr(o["g_sep"]), ptr(g2), ptr(t["m"]), ptr(o["out_sep"]), ptr(o["db_sep"]), P, 128, ptr(ews),
                                  ewsn, st))
    else:
        o["out2_sep"] = alloc.take(shape, BF16, role="output", name="out2_sep")
        ok(lib.siren_enc_res_bwd(ptr(o["g_sep"]), ptr(g2), ptr(t["m"]), ptr(t["pa"]), ptr(t["cb"]), ptr(o["out_sep"]),
                                 ptr(o["out2_sep"]), ptr(o["db_sep"]), P, 128, ptr(ews), ewsn, st))
    return o


@pytest.mark.parametrize("dma", [0, 1, 2])
@pytest.mark.parametrize("mode,with_g2", [(1, False), (1, True), (2, True)])
def test_conv_dgrad_k5_fused_equals_the_passes(mode, with_g2, dma):
    with options(conv_dma=dma):
        o = both(run_dgrad, mode, with_g2)
    assert torch.equal(o["out"], o["out_sep"])
    if mode == 2:
        assert torch.equal(o["out2"], o["out2_sep"])
    # channel sums in another fixed order (test_fused_dgrad_epilogues_match_the_passes: 1e-6)
    assert orc.norm_rel(o["db"].cpu(), o["db_sep"].cpu()) < 1e-6
    assert bool((o["out"] != 0).any())


def test_conv_dgrad_short_workspace_is_refused_before_any_launch():
    refused(run_dgrad, 2, True)


def run_wrw(alloc, N, H, W, ci, co, k, k5, short=False):
    lib = _native.lib()
    x, _, _, dy = conv_inputs(N, H, W, ci, co, k, seed=N)
    xd, dyd = inp(alloc, "x", nhwc(x)), inp(alloc, "dy", nhwc(dy))
    wsn = int(lib.siren_conv_wrw_workspace_bytes(N, H, W) if k5 else lib.siren_conv_wrw_ws_bytes(N, H, W, ci, co, k))
    ws = alloc.take((wsn,), U8, role="scratch", name="wrw_ws")
    o = {"dw": alloc.take((co, k, k, ci), F32, role="output", name="dw")}
    if k5:
        rc = lib.siren_conv_wrw_k5(ptr(xd), ptr(dyd), N, H, W, 128, ptr(o["dw"]), ptr(ws), wsn - short, stream())
    else:
        rc = lib.siren_conv_wrw(ptr(xd), ptr(dyd), N, H, W, ci, co, k, ptr(o["dw"]), ptr(ws), wsn - short, stream())
    if short:
        return rc
    ok(rc)
    return o


@pytest.mark.parametrize("dma", [0, 1, 2, 3])
@pytest.mark.parametrize("N,H,W", [(3, 7, 64), (1, 1, 128)])
@pytest.mark.parametrize("ci,co,k,k5", [(128, 128, 5, True), (128, 128, 5, False), (64, 128, 7, False), (128, 64, 3, False),
                                        (2, 64, 7, False), (2, 96, 5, False)])
def test_conv_weight_gradient(ci, co, k, k5, N, H, W, dma):
    with options(wrw_dma=dma):
        o = both(run_wrw, N, H, W, ci, co, k, k5)
    x, _, _, dy = conv_inputs(N, H, W, ci, co, k, seed=N)
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dy.double(), padding=k // 2)
    assert orc.norm_rel(o["dw"].cpu().permute(0, 3, 1, 2), ref) < 1e-6  # test_gpu_encoder.py's bound


@pytest.mark.parametrize("k5", [True, False])
def test_conv_wrw_short_workspace_is_refused_before_any_launch(k5):
    refused(run_wrw, 3, 7, 64, 128, 128, 5, k5)


# ---------------------------------------------------------------------- hypernetwork heads
HEADS, DEPTH, LATENT, HIDDEN = (4096, 256, 1030, 2, 513), 2, 128, 128


def hyper_inputs(rows):
    g = gen(rows)
    lin = lambda o, i: ((torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5, (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5)  # noqa: E731
    layers = [[lin(HIDDEN, LATENT)] + [lin(HIDDEN, HIDDEN) for _ in range(DEPTH - 1)] + [lin(of, HIDDEN)] for of in HEADS]
    return torch.randn(rows, LATENT, generator=g), layers, [torch.randn(rows, of, generator=g) for of in HEADS]


def run_hyper(alloc, rows, z_off, short=None):
    lib, st = _native.lib(), stream()
    z, layers, douts = hyper_inputs(rows)
    zd = inp(alloc, "z", z, z_off)
    d = _native.SirenHyperDesc()
    d.heads, d.depth, d.rows, d.in_features, d.hidden = len(HEADS), DEPTH, rows, LATENT, HIDDEN
    params = {}  # (kept alive: the descriptor holds only their addresses)
    for g, of in enumerate(HEADS):
        d.out_features[g] = of
        for l, (W, b) in enumerate(layers[g]):
            params[g, l] = (inp(alloc, f"W{g}_{l}", W), inp(alloc, f"b{g}_{l}", b))
            d.weight[g * 5 + l], d.bias[g * 5 + l] = ptr(params[g, l][0]), ptr(params[g, l][1])
    dd = [inp(alloc, f"dout{g}", t) for g, t in enumerate(douts)]
    sb, wb = int(lib.siren_hyper_saved_bytes(ctypes.byref(d))), int(lib.siren_hyper_workspace_bytes(ctypes.byref(d)))
    o = {f"out{g}": alloc.take((rows, of), F32, role="output", name=f"out{g}") for g, of in enumerate(HEADS)}
    saved = alloc.take((sb,), U8, role="scratch", name="saved")
    G = len(HEADS)
    VG = ctypes.c_void_p * G
    rc = lib.siren_hyper_forward(ctypes.byref(d), ptr(zd), VG(*[ptr(o[f"out{g}"]) for g in range(G)]), ptr(saved),
                                 sb - (short == "saved_fwd"), st)
    if short == "saved_fwd":
        return rc
    ok(rc)
    alloc.freeze("saved")
    work = alloc.take((wb,), U8, role="scratch", name="work")
    VL = ctypes.c_void_p * (_native.HYPER_MAXG * (_native.HYPER_MAXD + 1))
    dW, db = VL(), VL()
    for g in range(G):
        for l, (W, b) in enumerate(layers[g]):
            o[f"dW{g}_{l}"] = alloc.take(W.shape, F32, role="output", name=f"dW{g}_{l}")
            o[f"db{g}_{l}"] = alloc.take(b.shape, F32, role="output", name=f"db{g}_{l}")
            dW[g * 5 + l], db[g * 5 + l] = ptr(o[f"dW{g}_{l}"]), ptr(o[f"db{g}_{l}"])
    o["dz"] = alloc.take((rows, LATENT), F32, role="output", name="dz", offset_bytes=z_off)
    rc = lib.siren_hyper_backward(ctypes.byref(d), ptr(zd), VG(*[ptr(t) for t in dd]), ptr(saved), sb - (short == "saved_bwd"),
                                  ptr(work), wb - (short == "work_bwd"), dW, db, ptr(o["dz"]), st)
    if short:
        return rc
    ok(rc)
    return o


@pytest.mark.parametrize("rows,z_off", [(5, 0), (70, 0), (70, 4)])
def test_hyper_heads(rows, z_off):
    o = both(run_hyper, rows, z_off)
    z, layers, douts = hyper_inputs(rows)
    zz = z.double().requires_grad_(True)
    ref = {"dz": None}
    loss = 0
    for g, head in enumerate(layers):
        ps = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in head]
        h = zz
        for l, (W, b) in enumerate(ps):
            h = h @ W.T + b
            h = torch.relu(h) if l < DEPTH else h
        ref[f"out{g}"] = h.detach()
        loss = loss + (h * douts[g].double()).sum()
        ref[g] = ps
    loss.backward()
    for g in range(len(HEADS)):
        for l, (W, b) in enumerate(ref.pop(g)):
            ref[f"dW{g}_{l}"], ref[f"db{g}_{l}"] = W.grad, b.grad
    ref["dz"] = zz.grad
    for k, v in o.items():  # test_gpu_hyper.py: the fp32 paths agree with each other to 1e-5
        e = orc.norm_rel(v.cpu(), ref[k])
        assert e < 1e-5, (k, e)


@pytest.mark.parametrize("short", ["saved_fwd", "saved_bwd", "work_bwd"])
def test_hyper_short_buffer_is_refused_before_any_launch(short):
    plain = Plain(DEV)
    run_hyper(plain, 5, 0)
    arena = plain.arena()
    assert run_hyper(arena, 5, 0, short=short) == ENOSPACE, _native.last_error()
    for r in arena.regions:  # the (full-size) forward before a refused backward wrote its outputs
        if short != "saved_fwd" and r.name.startswith("out"):
            r.role = "scratch"
    arena.assert_nothing_launched()


# ---------------------------------------------------------------------- sum of squares
SUMSQ_SIZES = tuple(range(1, 60))


def split(t, sizes):
    return list(torch.split(t, list(sizes)))


def run_sumsq(alloc, sizes, short=False):
    """Tensors carved back to back: only 4-byte aligned. siren_sumsq_* take at most 32 per call."""
    lib, st, total = _native.lib(), stream(), sum(sizes)
    src = split(inp(alloc, "src", torch.randn(total, generator=gen(3))), sizes)
    g = inp(alloc, "g", torch.tensor([1.5]))
    dst_all = alloc.take((total,), F32, role="output", name="dst")
    dst = split(dst_all, sizes)
    o = {"dst": dst_all}
    for c0 in range(0, len(sizes), 32):
        n = min(32, len(sizes) - c0)
        numel = (ctypes.c_int64 * n)(*sizes[c0:c0 + n])
        VP = ctypes.c_void_p * n
        wsn = int(lib.siren_sumsq_workspace_bytes(sum(sizes[c0:c0 + n])))
        ws = alloc.take((wsn,), U8, role="zeroed", name=f"sumsq_ws{c0}")
        o[f"out{c0}"] = alloc.take((1,), F32, role="output", name=f"out{c0}")
        rc = lib.siren_sumsq_forward(n, VP(*[ptr(t) for t in src[c0:c0 + n]]), numel, ptr(o[f"out{c0}"]), ptr(ws), wsn - short, st)
        if short:
            return rc
        ok(rc)
        ok(lib.siren_sumsq_backward(n, VP(*[ptr(t) for t in src[c0:c0 + n]]), numel, ptr(g), VP(*[ptr(t) for t in dst[c0:c0 + n]]),
                                    st))
    return o


def test_sumsq():
    o = both(run_sumsq, SUMSQ_SIZES)
    src = torch.randn(sum(SUMSQ_SIZES), generator=gen(3)).double()
    parts = split(src, SUMSQ_SIZES)
    for c0 in range(0, len(SUMSQ_SIZES), 32):
        ref = sum(float((t ** 2).sum()) for t in parts[c0:c0 + 32])
        assert abs(float(o[f"out{c0}"]) - ref) <= 1e-6 * ref  # test_gpu_hyper.py's sum-of-squares bound
    assert orc.norm_rel(o["dst"].cpu(), 2 * 1.5 * src) < 1e-6


def test_sumsq_short_workspace_is_refused_before_any_launch():
    refused(run_sumsq, SUMSQ_SIZES)


# ---------------------------------------------------------------------- Adam
ADAM_SIZES = tuple(range(1, 60)) + (300, 77)
LR, BETAS, STEPS = 1e-2, (0.9, 0.999), 3


def adam_data():
    g = gen(9)
    total = sum(ADAM_SIZES)
    return torch.randn(total, generator=g), [torch.randn(total, generator=g) for _ in range(STEPS)]


def run_adam(alloc, form, graph=False):
    """STEPS steps of siren_adam_step over parameters, gradients and moments carved back to back, 48
    tensors per launch. form: "host" (the eager path: scalars in the descriptor), "computed"
    (siren_adam_scalars into dev_scalars), "scalars_table" (siren_adam_scalars_table into dev_scalars),
    "table" (per-workgroup step counters dev_steps reading dev_table: the graph mode's launch). graph: the
    first step eagerly, then one step captured into a hipGraph and replayed for the others, the gradient
    buffer rewritten in place before every replay (the device-counter forms only: that is what they are for)."""
    from siren_mri_amd.optim import Adam
    lib, st, total = _native.lib(), stream(), sum(ADAM_SIZES)
    p0, grads = adam_data()
    param = alloc.take((total,), F32, role="scratch", fill=p0, name="param")  # updated in place
    m = alloc.take((total,), F32, role="scratch", fill=0.0, name="exp_avg")
    v = alloc.take((total,), F32, role="scratch", fill=0.0, name="exp_avg_sq")
    gbuf = alloc.take((total,), F32, role="scratch", fill=0.0, name="grad")  # rewritten before every step
    ps, ms, vs, gs = (split(t, ADAM_SIZES) for t in (param, m, v, gbuf))
    o = {"param": param, "exp_avg": m, "exp_avg_sq": v}
    rows = Adam._scalar_rows(LR, *BETAS)
    table = inp(alloc, "table", rows) if form in ("table", "scalars_table") else None
    descs = []
    for c0 in range(0, len(ADAM_SIZES), _native.ADAM_MAX_TENSORS):
        d = _native.SirenAdamDesc()
        n = min(_native.ADAM_MAX_TENSORS, len(ADAM_SIZES) - c0)
        d.num_tensors, d.maximize = n, 0
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = LR, BETAS[0], BETAS[1], 1e-8, 0.0
        d.one_minus_beta1, d.one_minus_beta2 = 1 - BETAS[0], 1 - BETAS[1]
        for k in range(n):
            d.numel[k] = ADAM_SIZES[c0 + k]
            d.param[k], d.grad[k] = ptr(ps[c0 + k]), ptr(gs[c0 + k])
            d.exp_avg[k], d.exp_avg_sq[k] = ptr(ms[c0 + k]), ptr(vs[c0 + k])
        if form == "table":  # the step-counter array: updated in place, guarded
            nblk = max(int(lib.siren_adam_num_blocks(ctypes.byref(d))), 1)
            o[f"steps{c0}"] = alloc.take((nblk,), F64, role="scratch", fill=0.0, name=f"steps{c0}")
            d.dev_steps, d.dev_table, d.table_n = ptr(o[f"steps{c0}"]), ptr(table), rows.shape[0]
        descs.append(d)
    if form in ("computed", "scalars_table"):
        o["t"] = alloc.take((1,), F64, role="scratch", fill=0.0, name="t")
        o["scalars"] = alloc.take((2,), F32, role="output", name="scalars")
        for d in descs:
            d.dev_scalars = ptr(o["scalars"])
    def one_step(step):
        st = stream()  # (the capture stream inside a capture)
        if form == "computed":
            ok(lib.siren_adam_scalars(ptr(o["t"]), LR, BETAS[0], BETAS[1], ptr(o["scalars"]), st))
        elif form == "scalars_table":
            ok(lib.siren_adam_scalars_table(ptr(o["t"]), ptr(table), rows.shape[0], ptr(o["scalars"]), st))
        for d in descs:
            d.step_size = (LR / (1 - BETAS[0] ** step)) * -1  # (read by the "host" form only)
            d.bias_correction2_sqrt = (1 - BETAS[1] ** step) ** 0.5
            ok(lib.siren_adam_step(ctypes.byref(d), st))

    gdev = [gr.to(DEV) for gr in grads]
    captured = None
    for step, gr in enumerate(gdev, start=1):
        gbuf.copy_(gr)
        if not graph or step == 1:
            one_step(step)
        else:
            if captured is None:
                captured = torch.cuda.CUDAGraph()
                with torch.cuda.graph(captured):
                    one_step(step)
            captured.replay()
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("form,graph", [("host", False), ("computed", False), ("scalars_table", False), ("table", False),
                                        ("computed", True), ("scalars_table", True), ("table", True)])
def test_adam(form, graph):
    o = both(run_adam, form, graph)
    p0, grads = adam_data()
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = torch.optim.Adam([p], lr=LR, betas=BETAS, foreach=True)
    for gr in grads:
        p.grad = gr.to(DEV)
        opt.step()
    torch.testing.assert_close(o["param"], p.detach(), rtol=1e-6, atol=1e-7)  # test_gpu_optim.py's tolerances
    torch.testing.assert_close(o["exp_avg"], opt.state[p]["exp_avg"], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(o["exp_avg_sq"], opt.state[p]["exp_avg_sq"], rtol=1e-6, atol=1e-10)
    for k, t in o.items():
        if k.startswith("steps") or k == "t":
            assert bool((t == STEPS).all()), k
