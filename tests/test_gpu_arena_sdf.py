"""GPU: siren_sdf_loss_forward / siren_sdf_loss_backward on a poisoned arena (tests/_arena.py), as
test_gpu_arena_losses.py runs the other loss entry points: R = 1, 257 (a ragged second workgroup) and 70001
(more rows than the forward's 256 workgroups x 256 threads) with D = 2 and 3, every operand on the
allocator's alignment and every float operand 4 bytes off it.

Each driver runs on ordinary zero-filled buffers and on the arena; after the arena run I1 (guards), I2
(inputs), I3 (out[4], dpred and dgrad written in full), I4 (the loss workspace is zero again) hold and I5
every output is bit-equal to the plain run. I7: a workspace one byte short is refused with SIREN_ENOSPACE
before any launch. The values are held to their float64 reference by test_gpu_sdf.py; a coarse float64
check of the arena run here keeps the two runs from being wrong together."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sdf  # noqa: E402
from _arena import Plain, same_bits  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENOSPACE = -3
F32, U8 = torch.float32, torch.uint8
G4 = (1.0, 2.0, 3.0, 4.0)


def run_sdf(alloc, rows, d, off, short=False):
    lib = _native.lib()
    pred, grad, sdf, nrm = _sdf.operands(1, rows, d, seed=50 + d)

    def inp(name, t):
        return alloc.take(t.shape, F32, role="input", fill=t, name=name, offset_bytes=off)

    p, g, s, n = inp("pred", pred.reshape(rows)), inp("grad", grad.reshape(rows, d)), inp("sdf", sdf.reshape(rows)), \
        inp("nrm", nrm.reshape(rows, d))
    g4 = inp("g4", torch.tensor(G4))
    out = {"out4": alloc.take((4,), F32, role="output", name="out4", offset_bytes=off)}
    wsn = int(lib.siren_sse_workspace_bytes())
    ws = alloc.take((wsn,), U8, role="zeroed", name="loss_ws")
    stream = _native.stream_handle(DEV)
    rc = lib.siren_sdf_loss_forward(p.data_ptr(), g.data_ptr(), s.data_ptr(), n.data_ptr(), rows, d,
                                    out["out4"].data_ptr(), ws.data_ptr(), wsn - short, stream)
    if short:
        return rc
    assert rc == 0, _native.last_error()
    out["dpred"] = alloc.take((rows,), F32, role="output", name="dpred", offset_bytes=off)
    out["dgrad"] = alloc.take((rows, d), F32, role="output", name="dgrad", offset_bytes=off)
    rc = lib.siren_sdf_loss_backward(p.data_ptr(), g.data_ptr(), s.data_ptr(), n.data_ptr(), rows, d, g4.data_ptr(),
                                     out["dpred"].data_ptr(), out["dgrad"].data_ptr(), stream)
    assert rc == 0, _native.last_error()
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("rows", [1, 257, 70001])
def test_sdf_loss(rows, d, off):
    plain = Plain(DEV)
    a = run_sdf(plain, rows, d, off)
    plain.verify()
    arena = plain.arena()
    b = run_sdf(arena, rows, d, off)
    arena.verify()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"I5: {k} differs between the plain and the arena run"
    terms, dpred, dgrad = _sdf.formula64_grads(*_sdf.operands(1, rows, d, seed=50 + d), G4)
    for got, ref in zip(b["out4"].cpu().tolist(), terms.tolist()):
        assert got == pytest.approx(ref, rel=1e-5, abs=0.0)
    assert orc.norm_rel(b["dpred"].cpu(), dpred.reshape(rows)) <= 1e-6
    assert orc.norm_rel(b["dgrad"].cpu(), dgrad.reshape(rows, d)) <= 1e-6


def test_sdf_loss_short_workspace_is_refused_before_any_launch():
    plain = Plain(DEV)
    run_sdf(plain, 257, 3, 0)
    arena = plain.arena()
    assert run_sdf(arena, 257, 3, 0, short=True) == ENOSPACE, _native.last_error()
    arena.assert_nothing_launched()
