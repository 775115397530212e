"""GPU: siren_helmholtz_loss_forward / siren_helmholtz_loss_backward on a poisoned arena (tests/_arena.py), as
test_gpu_arena_wave.py runs the wave entry points: R = 1, 257 (a ragged second workgroup) and 70001 (more
rows than the forward's 256 workgroups x 256 threads), every operand on the allocator's alignment and every
operand 4 bytes off it (the kernels use dword loads and stores only).

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs), I3 (out[3], dpred, djac and dhess written in full), I4 (the loss workspace is zero again) hold
and I5 every output is bit-equal to the plain run. I7: a workspace one byte short is refused with
SIREN_ENOSPACE before any launch. The values are held to their float64 reference by test_gpu_helmholtz.py;
a coarse float64 check of the arena run here keeps the two runs from being wrong together."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helmholtz as _h  # noqa: E402
from _arena import Plain, same_bits  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
F32, U8 = torch.float32, torch.uint8
G3 = (1.0, 2.0, 3.0)
SHAPES = {"x": (2,), "pred": (2,), "jac": (2, 2), "hess": (2, 2, 2), "src": (2,), "slow": (2,)}


def run_helmholtz(alloc, rows, off, short=False):
    lib = _native.lib()
    ops = dict(zip(_h.OPERANDS, _h.operands(1, rows, seed=70)))

    def inp(name, t, shape):
        return alloc.take(shape, F32, role="input", fill=t.reshape(shape), name=name, offset_bytes=off)

    bufs = [inp(name, ops[name], (rows, *tail)) for name, tail in SHAPES.items()]
    bufs.append(inp("k", ops["k"], (1,)))
    g3 = inp("g3", torch.tensor(G3), (3,))
    out = {"out3": alloc.take((3,), F32, role="output", name="out3", offset_bytes=off)}
    wsn = int(lib.siren_sse_workspace_bytes())
    ws = alloc.take((wsn,), U8, role="zeroed", name="loss_ws")
    stream = _native.stream_handle(DEV)
    ptrs = [b.data_ptr() for b in bufs]
    rc = lib.siren_helmholtz_loss_forward(*ptrs, rows, rows, out["out3"].data_ptr(), ws.data_ptr(), wsn - short, stream)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    for name in ("pred", "jac", "hess"):
        out["d" + name] = alloc.take((rows, *SHAPES[name]), F32, role="output", name="d" + name, offset_bytes=off)
    rc = lib.siren_helmholtz_loss_backward(*ptrs, rows, rows, g3.data_ptr(), out["dpred"].data_ptr(),
                                           out["djac"].data_ptr(), out["dhess"].data_ptr(), stream)
    assert rc == 0, _native.last_error()
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("rows", [1, 257, 70001])
def test_helmholtz_loss(rows, off):
    plain = Plain(DEV)
    a = run_helmholtz(plain, rows, off)
    plain.verify()
    arena = plain.arena()
    b = run_helmholtz(arena, rows, off)
    arena.verify()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"I5: {k} differs between the plain and the arena run"
    terms, dpred, djac, dhess = _h.formula64_grads(*_h.operands(1, rows, seed=70), G3)
    for got, ref in zip(b["out3"].cpu().tolist(), terms.tolist()):
        assert got == pytest.approx(ref, rel=1e-5, abs=0.0)
    assert orc.norm_rel(b["dpred"].cpu(), dpred.reshape(rows, 2)) <= 1e-6
    assert orc.norm_rel(b["djac"].cpu(), djac.reshape(rows, 2, 2)) <= 1e-6
    assert orc.norm_rel(b["dhess"].cpu(), dhess.reshape(rows, 2, 2, 2)) <= 1e-6


def test_helmholtz_loss_short_workspace_is_refused_before_any_launch():
    plain = Plain(DEV)
    run_helmholtz(plain, 257, 0)
    arena = plain.arena()
    assert run_helmholtz(arena, 257, 0, short=True) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()
