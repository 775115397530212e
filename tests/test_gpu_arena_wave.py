"""GPU: siren_wave_loss_forward / siren_wave_loss_backward on a poisoned arena (tests/_arena.py), as
test_gpu_arena_sdf.py runs the signed-distance entry points: R = 1, 514 (a ragged third workgroup) and
70001 (more rows than the forward's 256 workgroups x 256 threads) with and without the Hessian, every
operand on the allocator's alignment and every float operand 4 bytes off it (the mask 1 byte off it).

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs), I3 (out[3], dpred, djac and dhess written in full), I4 (the loss workspace is zero again) hold
and I5 every output is bit-equal to the plain run. I7: a workspace one byte short is refused with
SIREN_ENOSPACE before any launch. The values are held to their float64 reference by test_gpu_wave.py; a
coarse float64 check of the arena run here keeps the two runs from being wrong together."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wave  # noqa: E402
from _arena import Plain, same_bits  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
F32, U8 = torch.float32, torch.uint8
G3 = (1.0, 2.0, 3.0)


def operands(rows, with_hess):
    pred, jac, hess, src, slow, mask = _wave.operands(1, rows, seed=60, mask="mixed" if with_hess else "all")
    return pred, jac, (hess if with_hess else None), src, slow, mask


def run_wave(alloc, rows, with_hess, off, short=False):
    lib = _native.lib()
    pred, jac, hess, src, slow, mask = operands(rows, with_hess)

    def inp(name, t, shape):
        return alloc.take(shape, F32, role="input", fill=t.reshape(shape), name=name, offset_bytes=off)

    p, j, s, l = inp("pred", pred, (rows,)), inp("jac", jac, (rows, 3)), inp("src", src, (rows,)), inp("slow", slow, (rows,))
    h = inp("hess", hess, (rows, 3, 3)) if with_hess else None
    m = alloc.take((rows,), U8, role="input", fill=mask.reshape(rows).to(U8), name="mask", offset_bytes=off // 4)
    g3 = inp("g3", torch.tensor(G3), (3,))
    out = {"out3": alloc.take((3,), F32, role="output", name="out3", offset_bytes=off)}
    wsn = int(lib.siren_sse_workspace_bytes())
    ws = alloc.take((wsn,), U8, role="zeroed", name="loss_ws")
    stream = _native.stream_handle(DEV)
    hp = h.data_ptr() if with_hess else None
    rc = lib.siren_wave_loss_forward(p.data_ptr(), j.data_ptr(), hp, s.data_ptr(), l.data_ptr(), m.data_ptr(), rows,
                                     rows, out["out3"].data_ptr(), ws.data_ptr(), wsn - short, stream)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    out["dpred"] = alloc.take((rows,), F32, role="output", name="dpred", offset_bytes=off)
    out["djac"] = alloc.take((rows, 3), F32, role="output", name="djac", offset_bytes=off)
    if with_hess:
        out["dhess"] = alloc.take((rows, 3, 3), F32, role="output", name="dhess", offset_bytes=off)
    rc = lib.siren_wave_loss_backward(p.data_ptr(), j.data_ptr(), hp, s.data_ptr(), l.data_ptr(), m.data_ptr(), rows,
                                      rows, g3.data_ptr(), out["dpred"].data_ptr(), out["djac"].data_ptr(),
                                      out["dhess"].data_ptr() if with_hess else None, stream)
    assert rc == 0, _native.last_error()
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("with_hess", [True, False])
@pytest.mark.parametrize("rows", [1, 514, 70001])
def test_wave_loss(rows, with_hess, off):
    plain = Plain(DEV)
    a = run_wave(plain, rows, with_hess, off)
    plain.verify()
    arena = plain.arena()
    b = run_wave(arena, rows, with_hess, off)
    arena.verify()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"I5: {k} differs between the plain and the arena run"
    terms, dpred, djac, dhess = _wave.formula64_grads(*operands(rows, with_hess), G3)
    for got, ref in zip(b["out3"].cpu().tolist(), terms.tolist()):
        assert got == pytest.approx(ref, rel=1e-5, abs=0.0)
    assert orc.norm_rel(b["dpred"].cpu(), dpred.reshape(rows)) <= 1e-6
    assert orc.norm_rel(b["djac"].cpu(), djac.reshape(rows, 3)) <= 1e-6
    if with_hess:
        assert orc.norm_rel(b["dhess"].cpu(), dhess.reshape(rows, 3, 3)) <= 1e-6


def test_wave_loss_short_workspace_is_refused_before_any_launch():
    plain = Plain(DEV)
    run_wave(plain, 514, True, 0)
    arena = plain.arena()
    assert run_wave(arena, 514, True, 0, short=True) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()
