"""GPU: wave-equation fitting on the native op siren_mri_amd::wave_loss / wave_loss_bwd (siren_wave.hip)
against float64 (golden/wave.npz and the same formula on the CPU, tests/_wave.py, pinned to the fixture by
test_wave_cpu.py), then end to end through the SIREN stack's Jacobian and Hessian passes.

Bounds. The op (tests 1, 2, 6): each term relative 1e-5, gradients oracle.norm_rel 1e-6 — what the k-space
and signed-distance loss ops are held to (test_gpu_kspace_losses.py, test_gpu_sdf.py) — or 8x the
reference's own float32-against-float64 error recorded in the fixture where that is larger (it is at most
3.9e-8 there, so this moves nothing today; the 8 covers the other summation order and the constants
folded differently). A term whose float64 value is 0 must be exactly 0, and so must every gradient entry
whose float64 value is exactly 0. End to end in fp32 mode (test 5): terms 4e-5 relative and parameter
gradients 1e-4 norm-relative, what test_gpu_hessian.py holds the FH prior's values and parameter
gradients to (the same stack ops under a kinked loss), against the reference's float32 run; 8x the
reference's float32-against-float64 error (terms at most 6.6e-8, gradients at most 4.1e-7) is smaller
than both, so that rule moves nothing either. The 3-step trajectory: 1e-4 relative, test_gpu_jvp.py's
trajectory bound. Every test prints the errors it measured; a run on an MI355X is recorded in
profiles/wave_loss_gpu_errors.txt.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wave  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native, diff_operators, loss_functions  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM_RTOL, GRAD_NORMREL = 1e-5, 1e-6
OPS = torch.ops.siren_mri_amd
NAMES = ("dpred", "djac", "dhess")


@pytest.fixture(scope="module")
def golden():
    return _wave.load_golden()


def on_dev(ops):
    return tuple(t.to(DEV) if t is not None else None for t in ops)


def run_native(pred, jac, hess, src, slow, mask, g=_wave.C):
    """(terms, dpred, djac, dhess or None) of the op and its autograd backward under the upstream weights g,
    on the CPU."""
    p, j = pred.to(DEV).requires_grad_(True), jac.to(DEV).requires_grad_(True)
    h = hess.to(DEV).requires_grad_(True) if hess is not None else None
    terms = OPS.wave_loss(p, j, h, src.to(DEV), slow.to(DEV), mask.to(DEV))
    assert "WaveLoss" in type(terms.grad_fn).__name__, type(terms.grad_fn).__name__
    (terms * torch.tensor(g, device=DEV)).sum().backward()
    return terms.detach().cpu(), p.grad.cpu(), j.grad.cpu(), (h.grad.cpu() if h is not None else None)


def term_errors(terms, ref):
    """Relative error per term; a term whose reference is 0 must be exactly 0."""
    errs = []
    for a, b in zip(terms.double().tolist(), ref.double().tolist()):
        if b == 0:
            assert a == 0
            errs.append(0.0)
        else:
            errs.append(abs(a - b) / abs(b))
    return errs


def check(tag, got, ref, term_rtol=(TERM_RTOL,) * 3, grad_tol=(GRAD_NORMREL,) * 3):
    te = term_errors(got[0], ref[0])
    ge = [orc.norm_rel(a, b) if b is not None else 0.0 for a, b in zip(got[1:], ref[1:])]
    print(f"\n[wave loss] {tag}: term rel err {', '.join(f'{e:.2e}' for e in te)} (bounds "
          f"{', '.join(f'{b:.1e}' for b in term_rtol)}); norm-rel "
          + ", ".join(f"{n} {e:.2e} ({b:.1e})" for n, e, b in zip(NAMES, ge, grad_tol)))
    assert torch.isfinite(got[0]).all()
    for e, b in zip(te, term_rtol):
        assert e <= b
    for n, a, b, e, tol in zip(NAMES, got[1:], ref[1:], ge, grad_tol):
        assert (a is None) == (b is None), n
        if a is None:
            continue
        assert torch.isfinite(a).all() and e < tol, n
        assert (a[b == 0] == 0).all(), n  # exact zeros wherever the float64 gradient is exactly 0


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the op against the fixture
def test_op_against_fixture(golden):
    ops = _wave.golden_operands(golden)
    pred, jac, hess, src, slow, mask = ops
    got = run_native(*ops)
    ref = tuple(torch.from_numpy(golden["op/" + k]) for k in ("terms64", "dpred64", "djac64", "dhess64"))
    check("fixture R=514", got, ref,
          tuple(max(TERM_RTOL, 8 * float(e)) for e in golden["op/terms_ref32_rel"]),
          tuple(max(GRAD_NORMREL, 8 * float(golden[f"op/{n}_ref32_normrel"])) for n in NAMES))
    _, dpred, djac, dhess = got
    flat = mask.reshape(-1)
    r0, r1, r2 = (int(golden["op/" + k]) for k in ("row_pred_eq_src", "row_ut0", "row_e0"))
    assert flat[r0] and flat[r1]
    # the planted rows: sign(0) = 0, and a difference that is exactly 0 is formed without contraction
    assert dpred.reshape(-1)[r0] == 0 and djac.reshape(-1, 3)[r1, 0] == 0 and (dhess.reshape(-1, 9)[r2] == 0).all()
    assert (dpred.reshape(-1)[~flat] == 0).all() and (djac.reshape(-1, 3)[~flat] == 0).all()
    assert (dpred.reshape(-1)[flat] != 0).sum() == flat.sum() - 1
    # the entries the loss does not read
    assert (djac[..., 1:] == 0).all()
    offdiag = ~torch.eye(3, dtype=torch.bool)
    assert (dhess[..., offdiag] == 0).all()
    others = torch.ones(flat.numel(), dtype=torch.bool)
    others[r2] = False
    assert (dhess.reshape(-1, 9)[others][:, [0, 4, 8]] != 0).all()
    # upstream (0, 0, 1): nothing reaches pred or jac; upstream (1, 1, 0): nothing reaches hess
    _, dp, dj, dh = run_native(*ops, g=(0.0, 0.0, 1.0))
    assert (dp == 0).all() and (dj == 0).all() and (dh != 0).any()
    _, dp, dj, dh = run_native(*ops, g=(1.0, 1.0, 0.0))
    assert (dh == 0).all() and (dp != 0).any() and (dj != 0).any()
    # NaN in src on the unmasked rows changes no bit of any output
    poisoned = src.clone()
    poisoned.reshape(-1)[~flat] = float("nan")
    again = run_native(pred, jac, hess, poisoned, slow, mask)
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ 2. shapes where the launch can go wrong
SHAPES = [(1, 1), (2, 1), (2, 63), (2, 257), (1, 2304), (1, 70001), (2, 70001)]


@pytest.mark.parametrize("mode", ["mixed", "none", "all_no_hess"])
@pytest.mark.parametrize("batch,n", SHAPES)
def test_op_shapes(batch, n, mode):
    """Rows R = batch x n: 1 and 2 (less than a wave), 126 (a ragged workgroup), 514 (three workgroups: the
    hand-off), 2304 (the fixture's batch), 70001 and 140002 (more rows than the 256 workgroups x 256 threads
    of the forward's cap: its grid stride). N = n, not R, scales the first two terms. Each with a mixed mask,
    an all-false mask, and hess=None under an all-true mask (the pretraining call)."""
    ops = list(_wave.operands(batch, n, seed=2000 + n, mask="all" if mode == "all_no_hess" else mode))
    if mode == "all_no_hess":
        ops[2] = None
    got = run_native(*ops)
    ref = _wave.formula64_grads(*ops, _wave.C)
    check(f"B={batch} N={n} {mode}", got, ref)
    if mode == "none":
        assert got[0][0] == 0 and got[0][1] == 0 and (got[1] == 0).all() and (got[2] == 0).all()
    if mode == "all_no_hess":
        assert got[0][2] == 0 and got[3] is None


def test_consecutive_launches_and_workspace():
    ops = on_dev(_wave.operands(1, 2304, seed=5))
    g = torch.tensor(_wave.C, device=DEV)
    first = (OPS.wave_loss(*ops), *OPS.wave_loss_bwd(*ops, g))
    second = (OPS.wave_loss(*ops), *OPS.wave_loss_bwd(*ops, g))
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    ws = _native.sse_workspace(DEV)
    assert int(ws.count_nonzero()) == 0  # the slots and the ticket are back to zero


def test_two_streams_have_their_own_workspaces():
    a = on_dev(_wave.operands(1, 2304, seed=6))
    b = on_dev(_wave.operands(1, 70001, seed=7))
    ref_a, ref_b = OPS.wave_loss(*a), OPS.wave_loss(*b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    outs, spaces = [], []
    for _ in range(4):
        for s, ops in ((s1, a), (s2, b)):
            with torch.cuda.stream(s):
                outs.append(OPS.wave_loss(*ops))
                spaces.append(_native.sse_workspace(DEV))
    torch.cuda.synchronize()
    assert spaces[0].data_ptr() != spaces[1].data_ptr()
    assert spaces[0].data_ptr() != _native.sse_workspace(DEV).data_ptr()
    for i, o in enumerate(outs):
        assert torch.equal(o, ref_a if i % 2 == 0 else ref_b)
    assert int(spaces[0].count_nonzero()) == 0 and int(spaces[1].count_nonzero()) == 0


# ------------------------------------------------------------------ 4. arguments, autograd registration
def test_argument_checks_and_empty_input():
    p, j, h = torch.zeros(1, 4, 1, device=DEV), torch.zeros(1, 4, 1, 3, device=DEV), torch.zeros(1, 4, 1, 3, 3, device=DEV)
    m = torch.zeros(1, 4, 1, device=DEV, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="one output"):
        OPS.wave_loss(torch.zeros(1, 4, 2, device=DEV), j, h, p, p, m)
    with pytest.raises(RuntimeError, match=r"jac .* must be \[1, 4, 1, 3\]"):
        OPS.wave_loss(p, torch.zeros(1, 4, 1, 2, device=DEV), h, p, p, m)
    with pytest.raises(RuntimeError, match=r"hess .* must be"):
        OPS.wave_loss(p, j, torch.zeros(1, 4, 3, 3, device=DEV), p, p, m)
    with pytest.raises(RuntimeError, match=r"slowness .* must be"):
        OPS.wave_loss(p, j, h, p, torch.zeros(1, 4, device=DEV), m)
    with pytest.raises(RuntimeError, match="float32"):
        OPS.wave_loss(p.double(), j, h, p, p, m)
    with pytest.raises(RuntimeError, match="mask must be bool"):
        OPS.wave_loss(p, j, h, p, p, m.float())
    with pytest.raises(RuntimeError, match="3 elements"):
        OPS.wave_loss_bwd(p, j, h, p, p, m, torch.zeros(1, device=DEV))
    e = (torch.zeros(1, 0, 1, device=DEV), torch.zeros(1, 0, 1, 3, device=DEV), torch.zeros(1, 0, 1, 3, 3, device=DEV))
    em = torch.zeros(1, 0, 1, device=DEV, dtype=torch.bool)
    terms = OPS.wave_loss(e[0], e[1], e[2], e[0], e[0], em)
    assert terms.shape == (3,) and (terms == 0).all()
    dp, dj, dh = OPS.wave_loss_bwd(e[0], e[1], e[2], e[0], e[0], em, torch.ones(3, device=DEV))
    assert dp.shape == e[0].shape and dj.shape == e[1].shape and dh.shape == e[2].shape
    dp, dj, dh = OPS.wave_loss_bwd(p, j, None, p, p, m, torch.ones(3, device=DEV))
    assert dh.numel() == 0 and (dp == 0).all() and (dj == 0).all()


def test_double_backward_raises():
    ops = on_dev(_wave.operands(1, 9, seed=8))
    p = ops[0].clone().requires_grad_(True)
    terms = OPS.wave_loss(p, *ops[1:])
    with pytest.raises(RuntimeError, match=r"double backward.*set_wave_loss_native\(False\)"):
        torch.autograd.grad(terms.sum(), p, create_graph=True)


def test_opcheck():
    pred, jac, hess, src, slow, mask = on_dev(_wave.operands(2, 9, seed=9))
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for h in (hess, None):
        leaves = (pred.clone().requires_grad_(True), jac.clone().requires_grad_(True),
                  h.clone().requires_grad_(True) if h is not None else None)
        torch.library.opcheck(OPS.wave_loss.default, (*leaves, src, slow, mask), test_utils=utils)
        torch.library.opcheck(OPS.wave_loss_bwd.default, (pred, jac, h, src, slow, mask, torch.ones(3, device=DEV)),
                              test_utils=utils)


# ------------------------------------------------------------------ 5. end to end, fp32 mode
def native_node(loss):
    """The autograd node of the op behind a dict value (terms[i]: an unbind of the op's output)."""
    fn = loss.grad_fn
    return type(fn.next_functions[0][0]).__name__ if fn is not None and fn.next_functions else ""


def stack(losses):
    return torch.stack([losses[k].detach().reshape(()) for k in _wave.KEYS])


def test_end_to_end_fp32(golden):
    m = _wave.golden_model(golden, "fp32", DEV)
    inp, gt = _wave.golden_batch(golden, DEV)
    losses = loss_functions.wave_pml(m(inp), gt)
    assert tuple(losses) == _wave.KEYS
    for k in _wave.KEYS:
        assert "WaveLoss" in native_node(losses[k]), native_node(losses[k])
    sum(losses.values()).backward()
    tb = [max(4e-5, 8 * float(e)) for e in golden["e2e/terms_ref32_rel"]]
    te = term_errors(stack(losses).cpu(), torch.from_numpy(golden["e2e/terms32"]))
    print(f"\n[wave loss] end to end fp32: term rel err {', '.join(f'{e:.2e}' for e in te)} (bounds "
          f"{', '.join(f'{b:.1e}' for b in tb)})")
    ge, gb = {}, {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k  # the output bias too: y itself is in the loss
        ge[k] = orc.norm_rel(p.grad.cpu(), torch.from_numpy(golden["e2e/grad32/" + k]))
        gb[k] = max(1e-4, 8 * float(golden["e2e/grad_ref32_normrel/" + k]))
    print("[wave loss] end to end fp32: parameter gradient norm-rel "
          + ", ".join(f"{k} {e:.2e} ({gb[k]:.1e})" for k, e in ge.items()))
    assert all(e <= b for e, b in zip(te, tb))
    assert all(ge[k] < gb[k] for k in ge)


def train3(m, inp, gt, tmp_path, name):
    from siren_mri_amd import training
    traj = []

    def loss_fn(model_output, gt_):
        losses = loss_functions.wave_pml(model_output, gt_)
        assert "WaveLoss" in native_node(losses["dirichlet"])
        traj.append(stack(losses))
        return losses

    training.train(m, [(inp, gt)], epochs=3, lr=2e-5, steps_til_summary=1000, epochs_til_checkpoint=1000,
                   model_dir=str(tmp_path / name), loss_fn=loss_fn, summary_fn=lambda *a, **k: None, clip_grad=False)
    return torch.stack(traj).cpu().double().numpy()


def test_training_trajectory_fp32(golden, tmp_path):
    m = _wave.golden_model(golden, "fp32", DEV)
    inp, gt = _wave.golden_batch(golden)
    got = train3(m, inp, gt, tmp_path, "run")
    ref = golden["e2e/traj"]
    print(f"\n[wave loss] 3-step trajectory: max rel err per step {np.abs(got / ref - 1).max(axis=1)} (bound 1e-4)")
    np.testing.assert_allclose(got, ref, rtol=1e-4)


def test_pretrain_batch_trains_without_the_hessian(golden, tmp_path):
    m = _wave.golden_model(golden, "fp32", DEV)
    inp, gt = _wave.golden_batch(golden, mode="pre")
    assert bool(gt["dirichlet_mask"].all())
    got = train3(m, inp, gt, tmp_path, "pre")
    print(f"\n[wave loss] pretrain batch, 3 steps: {got.tolist()}")
    assert np.isfinite(got).all() and (got[:, 2] == 0).all()
    assert got[2].sum() < got[0].sum()


# ------------------------------------------------------------------ 6. bf16 mode
def test_bf16_stack_native_equals_expression(golden):
    """The op on the bf16 stack's (y, jac, hess) against the expression path on those same tensors, in
    float64 and in float32 on the device: independent of the stack's precision."""
    m = _wave.golden_model(golden, "bf16", DEV)
    inp, gt = _wave.golden_batch(golden, DEV)
    o = m(inp)
    y, x = o["model_out"], o["model_in"]
    jac, _ = diff_operators.jacobian(y, x)
    hess, _ = diff_operators.hessian(y, x)
    src, slow, mask = gt["source_boundary_values"], gt["squared_slowness"], gt["dirichlet_mask"]
    ops = tuple(t.detach().float().cpu() for t in (y, jac, hess)) + (src.cpu(), slow.cpu(), mask.cpu())
    got = run_native(*ops)
    check("bf16 stack's (y, jac, hess) vs float64", got, _wave.formula64_grads(*ops, _wave.C))
    p, j, h = (t.to(DEV).requires_grad_(True) for t in ops[:3])
    expr = loss_functions._wave_expression(p, j, h, src, slow, mask, y.shape[1])
    terms = torch.stack([expr[k] for k in _wave.KEYS])
    (terms * torch.tensor(_wave.C, device=DEV)).sum().backward()
    check("bf16 stack's (y, jac, hess) vs expression path", got,
          (terms.detach().cpu(), p.grad.cpu(), j.grad.cpu(), h.grad.cpu()))
    # and through loss_functions.wave_pml the native op is what runs in bf16 mode
    losses = loss_functions.wave_pml(o, gt)
    assert "WaveLoss" in native_node(losses["diff_constraint_hom"])
    sum(losses.values()).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())


# ------------------------------------------------------------------ 7. switch and fallbacks
def test_switch_and_fallbacks(golden):
    from siren_mri_amd import modules
    m = _wave.golden_model(golden, "fp32", DEV)
    inp, gt = _wave.golden_batch(golden, DEV)
    native = loss_functions.wave_pml(m(inp), gt)
    assert "WaveLoss" in native_node(native["dirichlet"])
    loss_functions.set_wave_loss_native(False)
    try:
        expr = loss_functions.wave_pml(m(inp), gt)
    finally:
        loss_functions.set_wave_loss_native(True)
    assert "WaveLoss" not in native_node(expr["dirichlet"])
    te = term_errors(stack(native).cpu(), stack(expr).cpu())
    print(f"\n[wave loss] native vs expression path, same model: term rel err {', '.join(f'{e:.2e}' for e in te)}")
    assert all(e <= TERM_RTOL for e in te)
    sum(expr.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    # a 2-input model and a 2-output model: the expression path, finite
    torch.manual_seed(0)
    m2 = modules.SingleBVPNet(type="sine", in_features=2, hidden_features=64, num_hidden_layers=1, precision="fp32").to(DEV)
    l2 = loss_functions.wave_pml(m2({"coords": inp["coords"][..., :2].contiguous()}), gt)
    mo = modules.SingleBVPNet(type="sine", in_features=3, out_features=2, hidden_features=64, num_hidden_layers=1,
                              precision="fp32").to(DEV)
    lo = loss_functions.wave_pml(mo(inp), gt)
    for model, losses in ((m2, l2), (mo, lo)):
        assert tuple(losses) == _wave.KEYS and "WaveLoss" not in native_node(losses["dirichlet"])
        assert all(torch.isfinite(v).all() for v in losses.values())
        sum(v.sum() for v in losses.values()).backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    # float64 operands and CPU operands too
    ops = _wave.operands(1, 5, seed=3)
    assert loss_functions._wave_native_applies(*on_dev(ops))
    f64 = tuple(t.double() if t.is_floating_point() else t for t in on_dev(ops))
    for other in (f64, ops):
        assert not loss_functions._wave_native_applies(*other)
        vals = loss_functions._wave_expression(*other, 5)
        assert all(torch.isfinite(v).all() and v.device == other[0].device for v in vals.values())
        assert torch.allclose(torch.stack([vals[k].double().cpu() for k in _wave.KEYS]), _wave.formula64(*ops), rtol=1e-5)


# ------------------------------------------------------------------ 8. capture
def test_graph_capture_of_the_two_ops():
    """wave_loss then wave_loss_bwd captured on a side stream, R = 2304: two replays each equal the eager
    result bit for bit."""
    ops = on_dev(_wave.operands(1, 2304, seed=10))
    g = torch.tensor(_wave.C, device=DEV)
    eager = (OPS.wave_loss(*ops), *OPS.wave_loss_bwd(*ops, g))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):  # warm-up on the capture stream: its workspace exists before the capture
        OPS.wave_loss(*ops)
        OPS.wave_loss_bwd(*ops, g)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cap = (OPS.wave_loss(*ops), *OPS.wave_loss_bwd(*ops, g))
    for _ in range(2):
        for c in cap:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for c, e in zip(cap, eager):
            assert torch.equal(bits(c), bits(e))


# ------------------------------------------------------------------ 9. script smoke
def test_train_wave_equation_script_and_dense_evaluation(tmp_path):
    """20 pretraining steps of experiment_scripts/train_wave_equation.py in a child process (2304 rows, a
    3-64-64-64-64-1 net), then wave_eval.wave_field of the fitted model."""
    from siren_mri_amd import dataio, modules, wave_eval
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "train_wave_equation.py"), "--logging_root",
           str(tmp_path), "--experiment_name", "run", "--pretrain", "--sidelength", "48", "--hidden_features", "64",
           "--num_epochs", "20", "--steps_til_summary", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    steps = {}
    for line in r.stdout.splitlines():
        mt = re.match(r"step (\d+): (.*)", line)
        if mt:
            steps[int(mt.group(1))] = {k: float(v) for k, v in (kv.rsplit(" ", 1) for kv in mt.group(2).split(", "))}
    assert sorted(steps) == list(range(20)), sorted(steps)
    assert all(tuple(s) == _wave.KEYS and all(np.isfinite(v) for v in s.values()) for s in steps.values())
    print(f"\n[wave loss] train_wave_equation.py step 1: {steps[0]}\n[wave loss] train_wave_equation.py step 20: {steps[19]}")
    assert steps[19]["dirichlet"] < steps[0]["dirichlet"]
    assert all(s["diff_constraint_hom"] == 0 for s in steps.values())  # pretraining: no PDE term yet

    m = modules.SingleBVPNet(type="sine", in_features=3, hidden_features=64, num_hidden_layers=3, precision="fp32")
    m.load_state_dict(torch.load(tmp_path / "run" / "checkpoints" / "model_final.pth", weights_only=True))
    m = m.to(DEV)
    field = wave_eval.wave_field(m, 0.0, N=17)
    assert field.shape == (17, 17) and field.device.type == "cpu" and torch.isfinite(field).all()
    rows = torch.cat((torch.zeros(289, 1), dataio.get_mgrid(17)), dim=1)[None].to(DEV)
    with torch.no_grad():
        direct = m({"coords": rows})["model_out"].reshape(17, 17).cpu()
    # the same fp32 forward on the same rows: the stack's forward bound (smoke(): 1e-5)
    assert torch.allclose(field, direct, rtol=1e-5, atol=1e-5)
