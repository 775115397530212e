"""GPU: a training step replayed from a hipGraph computes what the same step computes eagerly.

bench.py reports, for the small grids, the time of ONE replay of a hipGraph holding K captured steps.
These tests check what such a replay trains, through bench.py's own enable_graph_mode() and capture()
(a fresh side stream with no warm-up on it, K steps in one graph, single-stream captures only).

1. The bench sequence (run_timed's order): 2 eager warm-up steps, enable_graph_mode, 1 eager step; a
   1-step graph replayed twice; a 3-step graph replayed twice; the graphs deleted; 2 eager steps on the
   default stream: 13 executed steps. The twin is the same workload built again from the same seed
   (initial parameters torch.equal) running the same 13 steps eagerly. After every segment the
   parameters, exp_avg, exp_avg_sq, the step count after sync_graph_steps(), the loss and model_out
   are compared.
   Bound: the eager twin runs twice. Where the two eager runs are torch.equal (after every segment)
   the replayed run must be torch.equal to them too, after every segment: no arithmetic differs
   between a replayed and an eager launch, and the
   SIREN stack, the losses and Adam are fixed-order sums (test_backward_deterministic,
   test_deterministic_and_expression_path_agrees), so c1, c2 and c3 must reproduce and are asserted
   to. Where they are not (c4: MIOpen's convolution gradients are not reproducible run to run,
   test_gpu_c4_precision.py), with D = p_final - p_init per parameter tensor:
       |D_replay - D_eagerA| <= 4 |D_eagerA - D_eagerB|   (4: one pair is a small sample of the spread)
       |D_replay - D_eagerA| <  1e-2 |D_eagerA|           (a stuck counter, a stale gradient or a baked
                                                           scalar moves D by tens of percent)
       |D_eagerA - D_eagerB| <  1e-2 |D_eagerA| / 4       (else the measurement says nothing)
   and the step counts are exact.
2. The reference loop's recorded trajectory (golden/train_c1.npz, fp32): 1 eager step, then a 3-step
   graph replayed 3 times. Bounds of test_training_train_matches_reference_loop: the 10 losses at rtol
   1e-5, the final parameters at norm_rel < 1e-4.
3. Replays read the buffers' current contents: the coordinates and targets are rewritten in place
   before every replay (a seeded sequence, the same for the twin), at the smallest shapes that take
   the pair ring with its tail reduce, the copy of a misaligned x (a hipMemcpyAsync node), the fp32
   path, per-set weights that are themselves parameters, and a k-space loss step whose reduction
   workspace is created inside the capture. Bound: the rule of part 1 against the all-eager twin; the
   bf16 cases also against the fp64 oracle on the LAST replayed step's inputs, at the bf16 tolerances
   of test_gpu_siren_stack.py (forward 3e-2, gradients 5e-2 norm-relative).
Every test prints what it measured; one MI355X run is recorded in profiles/graph_replay_parity.txt.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import siren_oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 3
# (steps of the unit, replayed from a graph in the replay run, snapshot after it, name)
UNITS = [(1, False, False, "warm-up 1"), (1, False, False, "warm-up 2"),
         (1, False, True, "eager step in graph mode"),
         (1, True, True, "1-step graph, replay 1"), (1, True, True, "1-step graph, replay 2"),
         (K, True, True, f"{K}-step graph, replay 1"), (K, True, True, f"{K}-step graph, replay 2"),
         (1, False, True, "eager step 1 after the graphs"), (1, False, True, "eager step 2 after the graphs")]
SEGMENTS = [(name, sum(u[0] for u in UNITS[:i + 1])) for i, (_, _, snap, name) in enumerate(UNITS) if snap]
LAST_REPLAY = [name for name, _ in SEGMENTS].index(f"{K}-step graph, replay 2")
assert SEGMENTS[-1][1] == 13


def _state(wl):
    """Everything a step leaves behind, cloned: parameters, Adam's moments and step counts (after
    sync_graph_steps), the step's loss and model_out, and what the workload asks to be watched."""
    torch.cuda.synchronize()
    opt = wl.extra["optimizer"]
    opt.sync_graph_steps()
    params = [p for g in opt.param_groups for p in g["params"]]
    states = [opt.state[p] if p in opt.state else {} for p in params]
    snap = {"param": [p.detach().clone() for p in params],
            "exp_avg": [s["exp_avg"].clone() if "exp_avg" in s else None for s in states],
            "exp_avg_sq": [s["exp_avg_sq"].clone() if "exp_avg_sq" in s else None for s in states],
            "step": [float(s["step"]) if "step" in s else None for s in states],
            "loss": [wl.extra["last"]["loss"].clone()], "model_out": [wl.extra["last"]["model_out"].clone()]}
    for name, ts in wl.extra.get("watch", {}).items():
        snap[name] = [t.clone() for t in ts]
    return snap


def _bench_sequence(wl, replay, feed=None):
    """bench.run_timed's order on a workload (UNITS); feed(i), if given, rewrites the workload's static
    inputs before unit i. replay=False: every unit runs eagerly on the default stream (the twin)."""
    import bench
    snaps, graphs = [], {}
    for i, (n, from_graph, snap, name) in enumerate(UNITS):
        if name == "eager step in graph mode":
            torch.cuda.synchronize()
            bench.enable_graph_mode(wl)
        if replay and not from_graph:
            graphs.clear()  # run_timed deletes its graphs before the eager region
        if replay and from_graph and n not in graphs:
            graphs[n] = bench.capture(wl.step, n)
        if feed is not None:
            feed(i)
        if replay and from_graph:
            graphs[n].replay()
        else:
            for _ in range(n):
                wl.step()
        if snap:
            snaps.append(_state(wl))
    return snaps


def _differing(a, b):
    """Names of the entries of two snapshots that are not torch.equal, with the largest difference."""
    bad = []
    for key in a:
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            if key == "step" or x is None or y is None:
                same, d = x == y, ""
            else:
                same = torch.equal(x, y)
                d = "" if same else f" (max |diff| {float((x.double() - y.double()).abs().max()):.3e})"
            if not same:
                bad.append(f"{key}[{i}]{d}")
    return bad


def _assert_replay_equals_eager(tag, runs, must_reproduce=True):
    """The rule of part 1 for runs = {"eager A", "eager B", "replay"} of (initial parameters, snapshots).
    Returns False when the two eager runs differ somewhere (and must_reproduce is False)."""
    for name in ("eager B", "replay"):
        assert all(torch.equal(x, y) for x, y in zip(runs["eager A"][0], runs[name][0])), \
            f"{tag}: {name} does not start from eager A's parameters"
    found = []
    for k, (seg, steps) in enumerate(SEGMENTS):
        a, b, r = (runs[name][1][k] for name in ("eager A", "eager B", "replay"))
        for name, s in (("eager A", a), ("replay", r)):
            counts = {c for c in s["step"] if c is not None}
            assert counts == {float(steps)}, f"{tag}, after '{seg}': {name} step counts {counts}, expected {steps}"
        ab, ar = _differing(a, b), _differing(a, r)
        found.append((seg, ab, ar))
        print(f"[graph replay] {tag}, after '{seg}' (step {steps}): eager A vs eager B "
              f"{'equal' if not ab else 'DIFFER ' + ', '.join(ab[:4])}; replay vs eager A "
              f"{'equal' if not ar else 'DIFFER ' + ', '.join(ar[:4])}")
    # two eager runs that agree after some segments and not after others are not reproducible (an
    # intermittent difference): bit-equality of the replayed run is asked only of workloads whose two
    # eager runs agree after every segment
    reproducible = not any(ab for _, ab, _ in found)
    if must_reproduce:
        for seg, ab, _ in found:
            assert not ab, f"{tag}, after '{seg}': two eager runs differ in {ab[:8]}"
    if reproducible:
        for seg, _, ar in found:
            assert not ar, f"{tag}, after '{seg}': the replayed run differs from the eager twin in {ar[:8]}"
    return reproducible


# ------------------------------------------------------------------ 1. the bench sequence
@pytest.fixture
def bench_args(monkeypatch):
    import bench
    old = torch.backends.cudnn.benchmark  # build_c4 switches MIOpen's find mode on for the process

    def args(cfg):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--config", cfg])
        return bench.parse()
    yield args
    torch.backends.cudnn.benchmark = old


def _build(cfg, precision, args):
    import bench
    if cfg in ("c1", "c2"):
        return bench.build_fit(cfg, args, DEV, 0, 1, precision)
    if cfg == "c3":
        return bench.build_c3(args, DEV, 0, 1, precision)
    return bench.build_c4(args, DEV, 0, 1, precision)


def _three_runs(build, feed_of=None):
    runs = {}
    for name, replay in (("eager A", False), ("eager B", False), ("replay", True)):
        wl = build()
        init = [p.detach().clone() for g in wl.extra["optimizer"].param_groups for p in g["params"]]
        runs[name] = (init, _bench_sequence(wl, replay, feed_of(wl) if feed_of else None), wl)
    return runs


@pytest.mark.parametrize("cfg,precision", [("c1", "bf16"), ("c1", "fp32"), ("c2", "bf16"), ("c2", "fp32"),
                                           ("c3", "fp32")])
def test_bench_sequence_replay_equals_eager(cfg, precision, bench_args):
    """c1 (64^2, 2-256-256-1), c2 (256^2, 5x256: the pair ring with several slabs per launch, the tail
    reduce handed to the next launch, more than one persistent round of the register forward) and c3
    (gradients_mse: the tangent-stream kernels and their double backward): bit for bit."""
    args = bench_args(cfg)
    runs = _three_runs(lambda: _build(cfg, precision, args))
    print()
    _assert_replay_equals_eager(f"{cfg} {precision}", runs)


def test_bench_sequence_c4_replay_within_the_eager_spread(bench_args):
    """c4 (bf16): conv encoder, hypernetwork heads, DC + loss, clip_grad_norm_, graph-mode Adam. Bit for
    bit where two eager runs are; else the measured bound of the module docstring. Measured on an
    MI355X: two eager runs differ in one tensor, the encoder's 1x1 convolution weight (MIOpen's weight
    gradient), by 3.3e-5 of its 13-step movement; the replayed run is 1.1 x that away from eager A there
    and torch.equal to it in every other parameter, the loss and model_out. That difference is
    intermittent (two runs can agree after 3 steps and differ later), so bit-equality is asked only
    when the eager runs agree after every segment. (The first c4 steps of a process run MIOpen's find,
    9 to 12 s once per process; after that this test takes 1.8 s.)"""
    args = bench_args("c4")
    runs = _three_runs(lambda: _build("c4", "bf16", args))
    print()
    if _assert_replay_equals_eager("c4 bf16", runs, must_reproduce=False):
        return
    init = runs["eager A"][0]
    fin = {name: runs[name][1][-1] for name in runs}
    assert {c for c in fin["replay"]["step"] if c is not None} == {13.0}
    for key in ("loss", "model_out"):
        a, b, r = (fin[name][key][0].double() for name in ("eager A", "eager B", "replay"))
        print(f"[graph replay] c4 bf16 final {key}: |A - B| / |A| {float((a - b).norm() / a.norm()):.3e}, "
              f"|replay - A| / |A| {float((r - a).norm() / a.norm()):.3e}")
    failures = []
    for i, p0 in enumerate(init):
        dA, dB, dR = ((fin[name]["param"][i].double() - p0.double()) for name in ("eager A", "eager B", "replay"))
        move, spread, err = float(dA.norm()), float((dA - dB).norm()), float((dR - dA).norm())
        cap = 1e-2 * move
        print(f"[graph replay] c4 bf16 param[{i}] {tuple(p0.shape)}: |D_A| {move:.3e}, |D_A - D_B| {spread:.3e} "
              f"({spread / move if move else 0.0:.2e} of |D_A|), |D_replay - D_A| {err:.3e} "
              f"({err / spread if spread else 0.0:.2f} x the spread)")
        if move == 0.0:
            if err != 0.0:
                failures.append(f"param[{i}]: unmoved by the eager run, moved by the replayed one")
            continue
        if not spread < cap / 4:
            failures.append(f"param[{i}]: eager spread {spread:.3e} not under a quarter of the cap {cap:.3e}")
        if not (err <= 4 * spread and err < cap):
            failures.append(f"param[{i}]: |D_replay - D_A| {err:.3e} > 4 x {spread:.3e} or >= {cap:.3e}")
    assert not failures, failures


# ------------------------------------------------------------------ 2. the reference's trajectory
def test_replayed_fit_follows_the_reference_trajectory():
    from siren_mri_amd import dataio, fusion, loss_functions, modules, training
    import bench
    d = np.load(os.path.join(G, "train_c1.npz"), allow_pickle=False)
    m = modules.SingleBVPNet(type="sine", hidden_features=256, num_hidden_layers=1, precision="fp32")
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init/")})
    m = m.to(DEV)
    model_input = {"coords": dataio.get_mgrid(64)[None].to(DEV)}
    gt = {"img": torch.from_numpy(d["img"]).to(DEV)}
    opt = training.make_adam(m.parameters(), 1e-4)
    opt.enable_graph_mode()
    kept = []

    def step():
        st = fusion.stage_image_loss(gt["img"])
        loss = loss_functions.image_mse(None, m(model_input), gt, high_freq=False)["img_loss"]
        fusion.clear(st)
        kept.append(loss.detach())
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    step()
    torch.cuda.synchronize()
    losses = [float(kept.pop())]
    graph = bench.capture(step, K)
    assert len(kept) == K
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        losses += [float(v) for v in kept]
    opt.sync_graph_steps()
    assert {float(opt.state[p]["step"]) for p in m.parameters()} == {10.0}
    rel = np.abs(np.array(losses) - d["losses"]) / np.abs(d["losses"])
    print(f"\n[graph replay] reference trajectory: worst loss rel err {rel.max():.2e} (bound 1e-5)")
    np.testing.assert_allclose(losses, d["losses"], rtol=1e-5)
    sd = m.state_dict()
    for k in sd:
        e = orc.norm_rel(sd[k].cpu(), torch.from_numpy(d["final/" + k]))
        print(f"[graph replay] reference trajectory: final {k} norm-rel {e:.2e} (bound 1e-4)")
        assert e < 1e-4, k


# ------------------------------------------------------------------ 3. replays read current contents
def _params(dims, sets, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for l in range(len(dims) - 1):
        W, b = orc.siren_init(dims, seed=seed + l)[l]
        if sets:
            W = (W.unsqueeze(0).repeat(sets, 1, 1) * (1 + 0.1 * torch.randn(sets, 1, 1, generator=g))).contiguous()
            b = (b.unsqueeze(0).repeat(sets, 1) + 0.01 * torch.randn(sets, dims[l + 1], generator=g)).contiguous()
        out.append((W, b))
    return out


def _plan_text(dims, precision, sets, rows, flags):
    from siren_mri_amd import _native
    desc = _native.describe_only(dims, prec=_native.PRECISIONS[precision], weights_batched=bool(sets),
                                 batch=sets or 1, rows_per_batch=rows)
    lib = _native.load_library()
    n = lib.siren_mlp_backward_plan(ctypes.byref(desc), flags, None, 0)
    assert n > 0, _native.last_error()
    buf = ctypes.create_string_buffer(n)
    assert lib.siren_mlp_backward_plan(ctypes.byref(desc), flags, buf, n) == n
    return buf.value.decode()


class _Stack:
    """A SIREN stack fitted by the bench's step (stage -> forward -> loss -> backward -> graph-mode Adam
    -> zero_grad(set_to_none=True)) on static coordinate / target buffers that feed() rewrites in place.
    kspace: the step is SIREN -> DataConsistencyInKspace -> image_asinh instead. Every step also leaves
    the parameters its forward read, its gradients and dx in static buffers (extra["watch"])."""

    def __init__(self, dims, precision, rows, sets=None, lead=1, misaligned=False, kspace=False, seed=0):
        from siren_mri_amd import training
        from siren_mri_amd.data_consistency import DataConsistencyInKspace
        self.dims, self.precision, self.sets, self.rows, self.kspace = dims, precision, sets, rows, kspace
        ps = _params(dims, sets, seed)
        self.ws = [W.to(DEV).requires_grad_(True) for W, _ in ps]
        self.bs = [b.to(DEV).requires_grad_(True) for _, b in ps]
        self.params = self.ws + self.bs
        B = sets or lead
        self.xbuf = torch.zeros(B, rows + (1 if misaligned else 0), dims[0], device=DEV)
        self.x = self.xbuf[:, 1:, :] if misaligned else self.xbuf  # an 8-byte-offset view
        assert self.x.is_contiguous() and (self.x.data_ptr() % 16 != 0) == misaligned
        self.tgt = torch.zeros(B, rows, dims[-1], device=DEV)
        g = torch.Generator().manual_seed(seed + 100)
        self.data = [[(torch.rand(self.x.shape, generator=g) * 2 - 1).to(DEV),
                      (0.5 * torch.randn(self.tgt.shape, generator=g)).to(DEV)] for _ in UNITS]
        if kspace:
            side = int(round(rows ** 0.5))
            self.dc = DataConsistencyInKspace()
            self.k0 = torch.zeros(B, dims[-1], side, side, device=DEV)
            self.mask = (torch.rand(self.k0.shape, generator=g) < 0.33).float().to(DEV)
            for unit in self.data:
                unit.append((0.5 * torch.randn(self.k0.shape, generator=g)).to(DEV))
        self.one = torch.ones((), device=DEV)
        opt = training.make_adam(self.params, 1e-4)
        self.p_in = [torch.zeros_like(p) for p in self.params]
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.dx = torch.zeros_like(self.x)
        self.last = {}
        self.extra = {"optimizer": opt, "last": self.last, "watch": {"p_in": self.p_in, "grad": self.grads,
                                                                     "dx": [self.dx]}}

    def feed(self, i):
        self.x.copy_(self.data[i][0])
        self.tgt.copy_(self.data[i][1])
        if self.kspace:
            self.k0.copy_(self.data[i][2])

    def step(self):
        from siren_mri_amd import fusion, loss_functions
        from siren_mri_amd.ops import siren_mlp
        opt = self.extra["optimizer"]
        x = self.x.detach().requires_grad_(True)  # as SingleBVPNet: the coordinates are a grad leaf
        with torch.no_grad():
            for s, p in zip(self.p_in, self.params):
                s.copy_(p)
        if self.kspace:
            y = siren_mlp(x, self.ws, self.bs, precision=self.precision)
            out = self.dc(y, self.k0, self.mask)
            loss = loss_functions.image_asinh(None, {"model_out": out}, {"img": self.tgt})["img_loss"]
            assert "KspaceLoss" in type(loss.grad_fn).__name__
        else:
            st = fusion.stage_image_loss(self.tgt, weight=loss_functions.KSPACE_WEIGHT)
            y = siren_mlp(x, self.ws, self.bs, precision=self.precision)
            loss = loss_functions.weighted_sse(y, self.tgt)
            fusion.clear(st)
        self.last["model_out"], self.last["loss"] = y.detach(), loss.detach()
        loss.backward(self.one)
        with torch.no_grad():
            for s, p in zip(self.grads, self.params):
                s.copy_(p.grad)
            self.dx.copy_(x.grad)
        opt.step()
        opt.zero_grad(set_to_none=True)

    def oracle(self, snap, unit):
        """fp64 forward and gradients of one step: parameters snap["p_in"], inputs self.data[unit]."""
        n = len(self.ws)
        ps = [(W.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True))
              for W, b in zip(snap["p_in"][:n], snap["p_in"][n:])]
        x = self.data[unit][0].double().cpu().requires_grad_(True)
        t = self.data[unit][1].double().cpu()
        y = orc.siren_forward(x, ps, 30.0, True)
        w = 1.0 / (128 * 128)
        if self.kspace:
            B, C = y.shape[0], y.shape[-1]
            k = self.data[unit][2].double().cpu().permute(0, 2, 3, 1).reshape(B, -1, C)
            m = self.mask.double().cpu().permute(0, 2, 3, 1).reshape(B, -1, C)
            out = (1 - m) * y + m * k
            loss = w * ((torch.asinh(400 * out) / 6.7 - torch.asinh(400 * t) / 6.7) ** 2).sum()
        else:
            loss = w * ((y - t) ** 2).sum()
        loss.backward()
        return y.detach(), loss.detach(), [W.grad for W, _ in ps] + [b.grad for _, b in ps], x.grad


STACKS = {
    # the pair ring, its tail reduce handed to the next launch, a ragged last tile (1000 = 7 x 128 + 104)
    "pair_ring": dict(dims=[2, 256, 256, 256, 256, 1], precision="bf16", rows=1000),
    # x 8 bytes past a 16-byte boundary: the plan starts with the hipMemcpyAsync of x into the workspace
    "misaligned_x": dict(dims=[2, 256, 256, 256, 1], precision="bf16", rows=1000, misaligned=True),
    "fp32_3_inputs": dict(dims=[3, 128, 128, 2], precision="fp32", rows=517),
    # weights [3, out, in] that are themselves the parameters Adam updates
    "per_set_weights": dict(dims=[2, 256, 256, 256, 2], precision="bf16", rows=500, sets=3),
    # SIREN -> DataConsistencyInKspace -> image_asinh on two 12x12 planes: the loss's reduction
    # workspace does not exist on the capture stream before the capture
    "kspace_loss": dict(dims=[2, 256, 256, 2], precision="bf16", rows=144, lead=2, kspace=True),
}


@pytest.mark.parametrize("case", list(STACKS))
def test_replays_read_the_current_buffer_contents(case):
    kw = STACKS[case]
    runs = _three_runs(lambda: _Stack(seed=len(case), **kw), feed_of=lambda wl: wl.feed)
    wl = runs["replay"][2]
    plan = _plan_text(kw["dims"], kw["precision"], kw.get("sets"), kw["rows"] * (1 if kw.get("sets") else kw.get("lead", 1)),
                      1 | (0 if kw.get("misaligned") else 2) | 4)
    if case == "pair_ring":
        assert all(s in plan for s in ("class=12", "class=13", "class=14", "reduce=next_pair")), plan
    if case == "misaligned_x":
        assert "xcopy=1" in plan and "hipMemcpyAsync" in plan, plan
    print()
    _assert_replay_equals_eager(case, runs)
    if kw["precision"] != "bf16":
        return
    # the last replayed step (the K-step graph's last, on the data fed before that replay)
    snap = runs["replay"][1][LAST_REPLAY]
    unit = [name for _, _, _, name in UNITS].index(SEGMENTS[LAST_REPLAY][0])
    y64, loss64, g64, dx64 = wl.oracle(snap, unit)
    ey = orc.norm_rel(snap["model_out"][0].cpu(), y64)
    el = abs(float(snap["loss"][0]) - float(loss64)) / abs(float(loss64))
    eg = [orc.norm_rel(g.cpu(), r) for g, r in zip(snap["grad"], g64)]
    edx = orc.norm_rel(snap["dx"][0].cpu(), dx64)
    print(f"[graph replay] {case}, last replayed step against the fp64 oracle: forward {ey:.2e} (bound 3e-2), "
          f"loss rel {el:.2e}, worst gradient {max(eg):.2e}, dx {edx:.2e} (bound 5e-2)")
    assert ey <= 3e-2
    for i, e in enumerate(eg):
        assert e <= 5e-2, f"gradient {i}: {e:.3e}"
    assert edx <= 5e-2
