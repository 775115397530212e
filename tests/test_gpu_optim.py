"""GPU: siren_mri_amd.optim.Adam (one native launch) against torch.optim.Adam's default foreach
path (the reference's optimizer, training.py:29) — same operation order; the two compilers'
multiply-add contraction differs, so values agree to an ulp (rtol 1e-6), not bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("kw", [dict(), dict(weight_decay=0.01), dict(maximize=True, betas=(0.8, 0.99))])
def test_adam_matches_torch_foreach(kw):
    from siren_mri_amd.optim import Adam
    g = torch.Generator().manual_seed(0)
    shapes = [(256, 2), (256,), (256, 256), (256,), (1, 256), (1,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    ours = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    ref = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    o1 = Adam(ours, lr=1e-3, **kw)
    o2 = torch.optim.Adam(ref, lr=1e-3, foreach=True, **kw)
    for step in range(7):
        grads = [torch.randn(s, generator=g).to(DEV) for s in shapes]
        for p, q, gr in zip(ours, ref, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        o1.step()
        o2.step()
    torch.cuda.synchronize()
    for p, q in zip(ours, ref):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(o1.state[p]["exp_avg"], o2.state[q]["exp_avg"], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(o1.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"], rtol=1e-6, atol=1e-10)
        assert float(o1.state[p]["step"]) == float(o2.state[q]["step"])


def test_adam_state_dict_round_trip_with_torch():
    from siren_mri_amd.optim import Adam
    p = torch.nn.Parameter(torch.randn(10, device=DEV))
    o1 = Adam([p], lr=1e-2)
    p.grad = torch.randn(10, device=DEV)
    o1.step()
    o2 = torch.optim.Adam([p], lr=1e-2)
    o2.load_state_dict(o1.state_dict())
    assert torch.equal(o2.state[p]["exp_avg"], o1.state[p]["exp_avg"])


@pytest.mark.parametrize("form", ["table", "computed"])
@pytest.mark.parametrize("sizes", [(300,), (300000, 77, 256 * 256), tuple(range(1, 60))])
def test_adam_graph_mode_replay_matches_eager(sizes, form, monkeypatch):
    """enable_graph_mode(): bias corrections from device step counters, so a hipGraph of the
    step replays with the right t each time (same values as eager steps). Table form: one launch
    per chunk of tensors, its workgroups advancing their own counters (59 tensors: two
    chunks); computed form (a table too long for the betas): a single-thread launch per step
    advances the group counter and computes the scalars."""
    from siren_mri_amd.optim import Adam
    if form == "computed":
        monkeypatch.setattr(Adam, "_TABLE_MAX", 4)
    g = torch.Generator().manual_seed(1)
    inits = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g).to(DEV) for n in sizes] for _ in range(6)]
    p_e = [torch.nn.Parameter(t.clone().to(DEV)) for t in inits]
    o_e = Adam(p_e, lr=1e-2)
    for gs in grads:
        for p, gr in zip(p_e, gs):
            p.grad = gr.clone()
        o_e.step()
    p_g = [torch.nn.Parameter(t.clone().to(DEV)) for t in inits]
    o_g = Adam(p_g, lr=1e-2)
    o_g.enable_graph_mode()
    gbuf = [torch.empty(n, device=DEV) for n in sizes]
    for p, b, gr in zip(p_g, gbuf, grads[0]):
        p.grad = b
        b.copy_(gr)
    o_g.step()  # eager first step creates the device counter (t = 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g.step()
    for gs in grads[1:]:
        for b, gr in zip(gbuf, gs):
            b.copy_(gr)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(p_g, p_e):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)
    o_g.sync_graph_steps()
    # the capture itself does not step: 1 eager + 5 replays = 6 steps, like the eager optimizer
    assert float(o_g.state[p_g[0]]["step"]) == 6.0


def _graph_mode_against_torch(groups, n_steps, loaded_steps=None, seed=3):
    """Graph-mode Adam (1 eager step, then ONE captured step() over all groups replayed n_steps - 1
    times on gradient buffers rewritten in place) against torch.optim.Adam(foreach=True) on the same
    gradients, and against the same update on float64 copies. groups: [(sizes, optimizer options)];
    loaded_steps: per group, the step count of a state dict (seeded moments) loaded into all three
    optimizers first. Returns the graph-mode optimizer and its parameters per group."""
    from oracle import siren_oracle as orc
    from siren_mri_amd.optim import Adam
    g = torch.Generator().manual_seed(seed)
    inits = [[torch.randn(n, generator=g) for n in sizes] for sizes, _ in groups]
    grads = [[[torch.randn(n, generator=g).to(DEV) for n in sizes] for sizes, _ in groups] for _ in range(n_steps)]
    moments = [[(0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)) for n in sizes]
               for sizes, _ in groups]

    def make(cls, dtype, **extra):
        ps = [[torch.nn.Parameter(t.clone().to(DEV, dtype)) for t in ts] for ts in inits]
        opt = cls([dict(params=p, **kw) for p, (_, kw) in zip(ps, groups)], lr=1e-2, **extra)
        if loaded_steps is not None:
            sd = opt.state_dict()
            flat = [(gi, k) for gi, ts in enumerate(inits) for k in range(len(ts))]
            assert [i for grp in sd["param_groups"] for i in grp["params"]] == list(range(len(flat)))
            sd["state"] = {i: {"step": torch.tensor(float(loaded_steps[gi])), "exp_avg": moments[gi][k][0].clone(),
                               "exp_avg_sq": moments[gi][k][1].clone()} for i, (gi, k) in enumerate(flat)}
            opt.load_state_dict(sd)
        return ps, opt

    p32, o32 = make(torch.optim.Adam, torch.float32, foreach=True)
    p64, o64 = make(torch.optim.Adam, torch.float64, foreach=True)
    for gs in grads:
        for ps, dtype in ((p32, torch.float32), (p64, torch.float64)):
            for pg, gg in zip(ps, gs):
                for p, gr in zip(pg, gg):
                    p.grad = gr.to(dtype)
        o32.step()
        o64.step()
    pg_, og = make(Adam, torch.float32)
    og.enable_graph_mode()
    bufs = [[torch.empty_like(p) for p in pg] for pg in pg_]
    for pg, bg in zip(pg_, bufs):
        for p, b in zip(pg, bg):
            p.grad = b

    def feed(gs):
        for bg, gg in zip(bufs, gs):
            for b, gr in zip(bg, gg):
                b.copy_(gr)
    feed(grads[0])
    og.step()  # the eager step in graph mode creates the device counters from the (loaded) step count
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    for gs in grads[1:]:
        feed(gs)
        graph.replay()
    torch.cuda.synchronize()
    og.sync_graph_steps()
    for gi in range(len(groups)):
        for a, b, r in zip(pg_[gi], p32[gi], p64[gi]):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(og.state[a]["exp_avg"], o32.state[b]["exp_avg"], rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(og.state[a]["exp_avg_sq"], o32.state[b]["exp_avg_sq"], rtol=1e-6, atol=1e-10)
            # no further from the float64 update than torch's own fp32 result
            ea, eb = orc.norm_rel(a.detach().cpu(), r.detach().cpu()), orc.norm_rel(b.detach().cpu(), r.detach().cpu())
            assert ea <= 2 * eb + 1e-7, (gi, ea, eb)
            assert float(og.state[a]["step"]) == float(o32.state[b]["step"])
    return og, pg_


SIZES = (300, 70000, 77)


@pytest.mark.parametrize("form", ["table", "computed"])
def test_adam_graph_mode_replays_past_the_table_end(form, monkeypatch):
    """Betas (0.5, 0.6): both bias corrections reach 1 in double within 100 steps, so the table is that
    short. From a loaded step count three short of its length: 1 eager step and 6 replays run across
    its last row and beyond it (the kernel repeats the last row). The computed form takes the same steps."""
    from siren_mri_amd.optim import Adam
    n = Adam._bias_corrections(0.5, 0.6)[0].shape[0]
    assert 8 < n < 100
    if form == "computed":
        monkeypatch.setattr(Adam, "_TABLE_MAX", 4)
    og, ps = _graph_mode_against_torch([(SIZES, dict(betas=(0.5, 0.6)))], 7, loaded_steps=[n - 3])
    tab = og._tables[id(og.param_groups[0])][2]
    assert (tab is None) == (form == "computed") and (tab is None or tab.shape[0] == n)
    assert float(og.state[ps[0][0]]["step"]) == n + 4


@pytest.mark.parametrize("form", ["table", "computed"])
def test_adam_graph_mode_resumes_from_a_loaded_step(form, monkeypatch):
    """Graph mode entered from a checkpoint at step 1000 (default betas): the device counters start
    there, and sync_graph_steps() brings 1000 + 1 eager + 5 replays back."""
    from siren_mri_amd.optim import Adam
    if form == "computed":
        monkeypatch.setattr(Adam, "_TABLE_MAX", 4)
    og, ps = _graph_mode_against_torch([(SIZES, dict())], 6, loaded_steps=[1000])
    assert all(float(og.state[p]["step"]) == 1006.0 for p in ps[0])


@pytest.mark.parametrize("kw", [dict(weight_decay=0.01), dict(maximize=True, betas=(0.8, 0.99))])
def test_adam_graph_mode_options_under_replay(kw):
    og, ps = _graph_mode_against_torch([(SIZES, kw)], 6)
    assert float(og.state[ps[0][0]]["step"]) == 6.0


def test_adam_graph_mode_two_groups_in_one_graph():
    """Two param groups (their own lr, betas and loaded step counts) in one optimizer and ONE graph:
    each group advances its own counters and reads its own table. 49 tensors in the second group:
    two launches of it."""
    groups = [((300, 4097), dict(lr=1e-2)), (tuple(range(1, 50)), dict(lr=1e-3, betas=(0.8, 0.99)))]
    og, ps = _graph_mode_against_torch(groups, 6, loaded_steps=[3, 10])
    assert float(og.state[ps[0][0]]["step"]) == 9.0 and float(og.state[ps[1][-1]]["step"]) == 16.0
    tabs = [og._tables[id(g)][2] for g in og.param_groups]
    assert tabs[0] is not tabs[1] and tabs[0].shape != tabs[1].shape


def test_adam_graph_mode_lr_schedule_rewrites_table_in_place():
    """an lr change in graph mode rewrites the step-scalar table in place (its length
    depends on the betas only): nothing is retired or allocated per lr value, and a hipGraph
    captured before the change replays the NEW lr, as the eager optimizer does."""
    from siren_mri_amd.optim import Adam
    g = torch.Generator().manual_seed(2)
    init = torch.randn(4096, generator=g)
    grads = [torch.randn(4096, generator=g).to(DEV) for _ in range(6)]
    lrs = [1e-2, 1e-2, 5e-3, 2.5e-3, 1e-3, 1e-3]
    p_e = torch.nn.Parameter(init.clone().to(DEV))
    o_e = Adam([p_e], lr=lrs[0])
    for lr, gr in zip(lrs, grads):
        o_e.param_groups[0]["lr"] = lr
        p_e.grad = gr.clone()
        o_e.step()
    p_g = torch.nn.Parameter(init.clone().to(DEV))
    o_g = Adam([p_g], lr=lrs[0])
    o_g.enable_graph_mode()
    buf = torch.empty(4096, device=DEV)
    p_g.grad = buf
    buf.copy_(grads[0])
    o_g.step()
    table = o_g._tables[id(o_g.param_groups[0])][2]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g.step()
    for lr, gr in zip(lrs[1:], grads[1:]):
        o_g.param_groups[0]["lr"] = lr  # a scheduler's per-step lr
        o_g.update_graph_scalars()
        buf.copy_(gr)
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(p_g.detach(), p_e.detach(), rtol=1e-6, atol=1e-7)
    assert o_g._tables[id(o_g.param_groups[0])][2] is table
    assert not o_g.__dict__.get("_retired")
