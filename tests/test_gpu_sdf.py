"""GPU: signed-distance fitting on the native op siren_mri_amd::sdf_loss / sdf_loss_bwd (siren_sdf.hip)
against the reference's float64 values (golden/sdf.npz) and the same formula in float64 on the CPU
(tests/_sdf.py, pinned to the reference by test_sdf_cpu.py), then end to end through the SIREN stack.

Bounds. The op (tests 1, 2, 4): each term relative 1e-5, gradients oracle.norm_rel 1e-6 — what the
k-space loss ops are held to (test_gpu_kspace_losses.py) — or 8x the reference's own
float32-against-float64 error recorded in the fixture where that is larger (it is at most 1.0e-7 there,
so this moves nothing today; the 8 covers device math functions specified to a few ulp and the other
summation order). dgrad holds two on-surface rows with grad == 0 whose reference gradient is n / 1e-8,
1e8 times the rest: next to the whole-tensor bound the same bound is held on the other rows alone.
End to end in fp32 mode (test 3): terms 4e-5 relative and parameter gradients 1e-4 norm-relative, what
test_gpu_hessian.py holds the FH prior's values and parameter gradients to (the same stack ops under a
kinked loss), against the reference's float32 run; 8x the reference's float32-against-float64 error is
smaller than both for every term and parameter (inter: 4.6e-8), so the rule for inter's exp(-100 |y|)
moves nothing. The 3-step trajectory: 1e-4 relative, test_gpu_jvp.py's bound for the C3 trajectory.
Every test prints the errors it measured; a run on an MI355X is recorded in
profiles/sdf_loss_gpu_errors.txt.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sdf  # noqa: E402
from oracle import siren_oracle as orc  # noqa: E402
from siren_mri_amd import _native, diff_operators, loss_functions  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM_RTOL, GRAD_NORMREL = 1e-5, 1e-6
OPS = torch.ops.siren_mri_amd


@pytest.fixture(scope="module")
def golden():
    return _sdf.load_golden()


def run_native(pred, grad, sdf, normals, g=_sdf.C):
    """(terms, dpred, dgrad) of the op and its autograd backward under the upstream weights g, on the CPU."""
    p, gr = pred.to(DEV).requires_grad_(True), grad.to(DEV).requires_grad_(True)
    terms = OPS.sdf_loss(p, gr, sdf.to(DEV), normals.to(DEV))
    assert "SdfLoss" in type(terms.grad_fn).__name__, type(terms.grad_fn).__name__
    (terms * torch.tensor(g, device=DEV)).sum().backward()
    return terms.detach().cpu(), p.grad.cpu(), gr.grad.cpu()


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


def huge_rows(grad, sdf):
    """Flat mask of the on-surface rows with grad == 0 (their dgrad is n / 1e-8)."""
    d = grad.shape[-1]
    return ((grad.reshape(-1, d) == 0).all(-1)) & (sdf.reshape(-1) != -1)


def check(tag, got, ref, operands, term_rtol=(TERM_RTOL,) * 4, dpred_tol=GRAD_NORMREL, dgrad_tol=GRAD_NORMREL):
    terms, dpred, dgrad = got
    ref_t, ref_dp, ref_dg = ref
    te = term_errors(terms, ref_t)
    pe, ge = orc.norm_rel(dpred, ref_dp), orc.norm_rel(dgrad, ref_dg)
    keep = ~huge_rows(operands[1], operands[2])
    d = dgrad.shape[-1]
    ge_rest = orc.norm_rel(dgrad.reshape(-1, d)[keep], ref_dg.reshape(-1, d)[keep]) if keep.any() else 0.0
    print(f"\n[sdf loss] {tag}: term rel err {', '.join(f'{e:.2e}' for e in te)} (bounds "
          f"{', '.join(f'{b:.1e}' for b in term_rtol)}); dpred norm-rel {pe:.2e} ({dpred_tol:.1e}); dgrad norm-rel "
          f"{ge:.2e}, without the grad == 0 on-surface rows {ge_rest:.2e} ({dgrad_tol:.1e})")
    assert torch.isfinite(terms).all() and torch.isfinite(dpred).all() and torch.isfinite(dgrad).all()
    for e, b in zip(te, term_rtol):
        assert e <= b
    assert pe < dpred_tol and ge < dgrad_tol and ge_rest < dgrad_tol
    # exact zeros wherever the float64 gradient is exactly 0
    assert (dpred[ref_dp == 0] == 0).all() and (dgrad[ref_dg == 0] == 0).all()


# ------------------------------------------------------------------ 1. the op against the fixture
@pytest.mark.parametrize("tag", ["d3", "d2"])
def test_op_against_fixture(golden, tag):
    ops = tuple(torch.from_numpy(golden[f"{tag}/{k}"]) for k in ("pred", "grad", "sdf", "normals"))
    pred, grad, sdf, normals = ops
    d = grad.shape[-1]
    got = run_native(*ops)
    ref = tuple(torch.from_numpy(golden[f"{tag}/{k}"]) for k in ("terms64", "dpred64", "dgrad64"))
    check(f"fixture {tag}", got, ref, ops,
          tuple(max(TERM_RTOL, 8 * float(e)) for e in golden[f"{tag}/terms_ref32_rel"]),
          max(GRAD_NORMREL, 8 * float(golden[f"{tag}/dpred_ref32_normrel"])),
          max(GRAD_NORMREL, 8 * float(golden[f"{tag}/dgrad_ref32_normrel"])))
    _, dpred, dgrad = got
    idx = {k: torch.from_numpy(golden[f"{tag}/{k}"]) for k in ("pred0_on", "pred0_off", "grad0", "grad_unit")}
    off = sdf.reshape(-1) == -1
    # pred == 0: sign(0) = 0 on both branches
    assert (dpred.reshape(-1)[idx["pred0_on"]] == 0).all() and (dpred.reshape(-1)[idx["pred0_off"]] == 0).all()
    # grad == 0 and |grad| == 1 exactly: the grad_constraint part is 0 (all of dgrad on an off-surface row)
    for k in ("grad0", "grad_unit"):
        rows = idx[k][off[idx[k]]]
        assert rows.numel() and (dgrad.reshape(-1, d)[rows] == 0).all(), k
    _, dp3, dg3 = run_native(*ops, g=(0.0, 0.0, 0.0, 1.0))
    assert (dp3 == 0).all()
    for k in ("grad0", "grad_unit"):
        assert (dg3.reshape(-1, d)[idx[k]] == 0).all(), k
    # upstream (0, 0, 1, 0): nothing reaches pred, and nothing an off-surface row
    _, dp2, dg2 = run_native(*ops, g=(0.0, 0.0, 1.0, 0.0))
    assert (dp2 == 0).all()
    assert (dg2.reshape(-1, d)[off] == 0).all() and (dg2.reshape(-1, d)[~off] != 0).any()
    # NaN normals on the off-surface rows change nothing
    poisoned = normals.clone()
    poisoned.reshape(-1, d)[off] = float("nan")
    again = run_native(pred, grad, sdf, poisoned)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 2. shapes where the launch can go wrong
SHAPES = [(1, 1), (2, 1), (2, 63), (2, 257), (2, 1400), (1, 2800), (1, 70001), (2, 70001)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("batch,n", SHAPES)
def test_op_shapes(batch, n, d):
    """Rows R = batch x n: 1 and 2 (less than a wave), 126 and 514 (a ragged workgroup; three of them, the
    hand-off), 2800 (the script's batch, as 2 x 1400 and 1 x 2800), 70001 and 140002 (more rows than the 256
    workgroups x 256 threads of the forward's cap: its grid stride)."""
    ops = _sdf.operands(batch, n, d, seed=1000 + n + d)
    got = run_native(*ops)
    ref = _sdf.formula64_grads(*ops, _sdf.C)
    check(f"B={batch} N={n} D={d}", got, ref, ops)


@pytest.mark.parametrize("d", [2, 3])
def test_consecutive_launches_and_workspace(d):
    ops = tuple(t.to(DEV) for t in _sdf.operands(2, 1400, d, seed=5))
    g = torch.tensor(_sdf.C, device=DEV)
    first = (OPS.sdf_loss(*ops), *OPS.sdf_loss_bwd(*ops, g))
    second = (OPS.sdf_loss(*ops), *OPS.sdf_loss_bwd(*ops, g))
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    ws = _native.sse_workspace(DEV)
    assert int(ws.count_nonzero()) == 0  # the slots and the ticket are back to zero


def test_two_streams_have_their_own_workspaces():
    a = tuple(t.to(DEV) for t in _sdf.operands(2, 1400, 3, seed=6))
    b = tuple(t.to(DEV) for t in _sdf.operands(1, 70001, 3, seed=7))
    ref_a, ref_b = OPS.sdf_loss(*a), OPS.sdf_loss(*b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    outs, spaces = [], []
    for _ in range(4):
        for s, ops in ((s1, a), (s2, b)):
            with torch.cuda.stream(s):
                outs.append(OPS.sdf_loss(*ops))
                spaces.append(_native.sse_workspace(DEV))
    torch.cuda.synchronize()
    assert spaces[0].data_ptr() != spaces[1].data_ptr()
    assert spaces[0].data_ptr() != _native.sse_workspace(DEV).data_ptr()
    for i, o in enumerate(outs):
        assert torch.equal(o, ref_a if i % 2 == 0 else ref_b)
    assert int(spaces[0].count_nonzero()) == 0 and int(spaces[1].count_nonzero()) == 0


def test_argument_checks_and_empty_input():
    p, g = torch.zeros(1, 4, 1, device=DEV), torch.zeros(1, 4, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r"must be \[B, N, D\]"):
        OPS.sdf_loss(p, torch.zeros(1, 4, 4, device=DEV), p, torch.zeros(1, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="one output"):
        OPS.sdf_loss(torch.zeros(1, 4, 2, device=DEV), g, p, g)
    with pytest.raises(RuntimeError, match="float32"):
        OPS.sdf_loss(p.double(), g, p, g)
    with pytest.raises(RuntimeError, match="4 elements"):
        OPS.sdf_loss_bwd(p, g, p, g, torch.zeros(1, device=DEV))
    e = torch.zeros(1, 0, 1, device=DEV), torch.zeros(1, 0, 3, device=DEV)
    terms = OPS.sdf_loss(e[0], e[1], e[0], e[1])
    assert terms.shape == (4,) and (terms == 0).all()
    dp, dg = OPS.sdf_loss_bwd(e[0], e[1], e[0], e[1], torch.ones(4, device=DEV))
    assert dp.shape == e[0].shape and dg.shape == e[1].shape


def test_double_backward_raises():
    ops = tuple(t.to(DEV) for t in _sdf.operands(1, 9, 3, seed=8))
    p = ops[0].clone().requires_grad_(True)
    terms = OPS.sdf_loss(p, *ops[1:])
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(terms.sum(), p, create_graph=True)


def test_opcheck():
    ops = tuple(t.to(DEV) for t in _sdf.operands(2, 9, 3, seed=9))
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(OPS.sdf_loss.default, (ops[0].clone().requires_grad_(True), ops[1].clone().requires_grad_(True),
                                                 ops[2], ops[3]), test_utils=utils)
    torch.library.opcheck(OPS.sdf_loss_bwd.default, (*ops, torch.ones(4, device=DEV)), test_utils=utils)


# ------------------------------------------------------------------ 3. end to end, fp32 mode
def native_node(loss):
    """The autograd node of the op behind a dict value (terms[i]: a select of the op's output)."""
    return type(loss.grad_fn.next_functions[0][0]).__name__


def test_end_to_end_fp32(golden):
    m = _sdf.golden_model(golden, "fp32", DEV)
    inp, gt = _sdf.golden_batch(golden, DEV)
    losses = loss_functions.sdf(m(inp), gt)
    assert tuple(losses) == _sdf.KEYS
    for k in _sdf.KEYS:
        assert "SdfLoss" in native_node(losses[k]), native_node(losses[k])
    sum(losses.values()).backward()
    te = term_errors(torch.stack([losses[k].detach() for k in _sdf.KEYS]).cpu(), torch.from_numpy(golden["e2e/terms32"]))
    print(f"\n[sdf loss] end to end fp32: term rel err {', '.join(f'{e:.2e}' for e in te)} (bound 4.0e-05)")
    ge = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k  # the output bias too: y itself is in the loss
        ge[k] = orc.norm_rel(p.grad.cpu(), torch.from_numpy(golden["e2e/grad32/" + k]))
    print("[sdf loss] end to end fp32: parameter gradient norm-rel " + ", ".join(f"{k} {e:.2e}" for k, e in ge.items())
          + " (bound 1.0e-04)")
    assert all(e <= 4e-5 for e in te)
    assert all(e < 1e-4 for e in ge.values())


def test_training_trajectory_fp32(golden, tmp_path):
    from siren_mri_amd import training
    m = _sdf.golden_model(golden, "fp32", DEV)
    inp, gt = _sdf.golden_batch(golden)
    traj = []

    def loss_fn(model_output, gt_):
        losses = loss_functions.sdf(model_output, gt_)
        traj.append(torch.stack([losses[k].detach() for k in _sdf.KEYS]))
        return losses

    training.train(m, [(inp, gt)], epochs=3, lr=1e-4, steps_til_summary=1000, epochs_til_checkpoint=1000,
                   model_dir=str(tmp_path / "run"), loss_fn=loss_fn, summary_fn=lambda *a, **k: None, clip_grad=True)
    got = torch.stack(traj).cpu().double().numpy()
    ref = golden["e2e/traj"]
    print(f"\n[sdf loss] 3-step trajectory: max rel err per step {np.abs(got / ref - 1).max(axis=1)} (bound 1e-4)")
    np.testing.assert_allclose(got, ref, rtol=1e-4)


# ------------------------------------------------------------------ 4. bf16 mode
def test_bf16_stack_native_equals_expression(golden):
    """The op on the bf16 stack's (y, grad y) against the expression path on those same tensors, in float64
    and in float32 on the device: independent of the stack's precision."""
    m = _sdf.golden_model(golden, "bf16", DEV)
    inp, gt = _sdf.golden_batch(golden, DEV)
    o = m(inp)
    y = o["model_out"]
    g = diff_operators.gradient(y, o["model_in"])
    ops = (y.detach().cpu(), g.detach().cpu(), gt["sdf"].cpu(), gt["normals"].cpu())
    got = run_native(*ops)
    check("bf16 stack's (y, grad) vs float64", got, _sdf.formula64_grads(*ops, _sdf.C), ops)
    p, gr = ops[0].to(DEV).requires_grad_(True), ops[1].to(DEV).requires_grad_(True)
    expr = loss_functions._sdf_expression(p, gr, gt["sdf"], gt["normals"])
    terms = torch.stack([expr[k] for k in _sdf.KEYS])
    (terms * torch.tensor(_sdf.C, device=DEV)).sum().backward()
    check("bf16 stack's (y, grad) vs expression path", got, (terms.detach().cpu(), p.grad.cpu(), gr.grad.cpu()), ops)
    # and through loss_functions.sdf the native op is what runs in bf16 mode
    assert "SdfLoss" in native_node(loss_functions.sdf(o, gt)["inter"])


# ------------------------------------------------------------------ 5. switch and fallbacks
def _uses_native(losses):
    fn = losses["sdf"].grad_fn
    return fn is not None and fn.next_functions and "SdfLoss" in type(fn.next_functions[0][0]).__name__


def test_switch_and_fallbacks(golden):
    from siren_mri_amd import modules
    m = _sdf.golden_model(golden, "fp32", DEV)
    inp, gt = _sdf.golden_batch(golden, DEV)
    native = loss_functions.sdf(m(inp), gt)
    assert _uses_native(native)
    loss_functions.set_sdf_loss_native(False)
    try:
        expr = loss_functions.sdf(m(inp), gt)
    finally:
        loss_functions.set_sdf_loss_native(True)
    assert not _uses_native(expr)
    te = term_errors(torch.stack([native[k].detach() for k in _sdf.KEYS]).cpu(),
                     torch.stack([expr[k].detach() for k in _sdf.KEYS]).cpu())
    print(f"\n[sdf loss] native vs expression path, same model: term rel err {', '.join(f'{e:.2e}' for e in te)}")
    assert all(e <= TERM_RTOL for e in te)
    sum(expr.values()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    # a 2-channel output and 4 input dimensions: the expression path, finite
    torch.manual_seed(0)
    m2 = modules.SingleBVPNet(type="sine", in_features=3, out_features=2, hidden_features=64, num_hidden_layers=1,
                              precision="fp32").to(DEV)
    l2 = loss_functions.sdf(m2(inp), gt)
    m4 = modules.SingleBVPNet(type="sine", in_features=4, hidden_features=64, num_hidden_layers=1, precision="fp32").to(DEV)
    c4 = torch.cat([inp["coords"], inp["coords"][..., :1]], dim=-1)
    n4 = torch.cat([gt["normals"], gt["normals"][..., :1]], dim=-1)
    l4 = loss_functions.sdf(m4({"coords": c4}), {"sdf": gt["sdf"], "normals": n4})
    for losses in (l2, l4):
        assert tuple(losses) == _sdf.KEYS and not _uses_native(losses)
        assert all(torch.isfinite(v) for v in losses.values())
        sum(losses.values()).backward()
    # float64 operands and CPU operands too
    z1, z3 = torch.zeros(1, 5, 1, device=DEV), torch.zeros(1, 5, 3, device=DEV)
    assert loss_functions._sdf_native_applies(z1, z3, z1, z3)
    assert not loss_functions._sdf_native_applies(z1.double(), z3.double(), z1.double(), z3.double())
    assert not loss_functions._sdf_native_applies(z1.cpu(), z3.cpu(), z1.cpu(), z3.cpu())


# ------------------------------------------------------------------ 6. capture
def test_graph_capture_of_the_two_ops():
    """sdf_loss then sdf_loss_bwd captured on a side stream, R = 2800: two replays each equal the eager
    result bit for bit."""
    ops = tuple(t.to(DEV) for t in _sdf.operands(2, 1400, 3, seed=10))
    g = torch.tensor(_sdf.C, device=DEV)
    eager = (OPS.sdf_loss(*ops), *OPS.sdf_loss_bwd(*ops, g))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):  # warm-up on the capture stream: its workspace exists before the capture
        OPS.sdf_loss(*ops)
        OPS.sdf_loss_bwd(*ops, g)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cap = (OPS.sdf_loss(*ops), *OPS.sdf_loss_bwd(*ops, g))
    for _ in range(2):
        for c in cap:
            c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for c, e in zip(cap, eager):
            assert torch.equal(c, e)


# ------------------------------------------------------------------ 7. script smoke
def test_train_sdf_script_and_dense_evaluation(tmp_path):
    """20 steps of experiment_scripts/train_sdf.py on the synthetic torus in a child process (one epoch of
    28000 points in batches of 1400), then sdf_meshing.sdf_volume of the fitted model."""
    from siren_mri_amd import modules, sdf_meshing
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "train_sdf.py"), "--logging_root", str(tmp_path),
           "--experiment_name", "run", "--num_epochs", "1", "--synthetic_points", "28000", "--steps_til_summary", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    steps = {}
    for line in r.stdout.splitlines():
        mt = re.match(r"step (\d+): (.*)", line)
        if mt:
            steps[int(mt.group(1))] = {k: float(v) for k, v in (kv.rsplit(" ", 1) for kv in mt.group(2).split(", "))}
    assert sorted(steps) == list(range(20)), sorted(steps)
    assert all(tuple(s) == _sdf.KEYS and all(np.isfinite(v) for v in s.values()) for s in steps.values())
    print(f"\n[sdf loss] train_sdf.py step 1: {steps[0]}\n[sdf loss] train_sdf.py step 20: {steps[19]}")
    assert steps[19]["sdf"] < steps[0]["sdf"] and steps[19]["normal_constraint"] < steps[0]["normal_constraint"]
    totals = np.loadtxt(tmp_path / "run" / "checkpoints" / "train_losses_final.txt")
    assert totals.shape == (20,) and np.all(np.isfinite(totals))

    m = modules.SingleBVPNet(type="sine", in_features=3, precision="fp32")
    m.load_state_dict(torch.load(tmp_path / "run" / "checkpoints" / "model_final.pth", weights_only=True))
    m = m.to(DEV)
    vol = sdf_meshing.sdf_volume(m, N=17)
    assert vol.shape == (17, 17, 17) and vol.device.type == "cpu" and torch.isfinite(vol).all()
    idx = torch.randint(0, 17, (50, 3), generator=torch.Generator().manual_seed(0))
    pts = (-1 + 2 * idx.float() / 16)[None].to(DEV)
    with torch.no_grad():
        direct = m({"coords": pts})["model_out"].reshape(-1).cpu()
    # two launches of one fp32 forward on different row sets: the stack's forward bound (smoke(): 1e-5)
    assert torch.allclose(vol[idx[:, 0], idx[:, 1], idx[:, 2]], direct, rtol=1e-5, atol=1e-5)
