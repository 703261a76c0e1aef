"""GPU: omnifusion_amd.optim.AdamW (csrc/omni_optim.hip) against float64 — the gate of tests/_adamw_ref.py, taken from
torch's own CPU AdamW in float32 and float64 — on segment sizes around every boundary of the layout (1 element, off multiples of 4 and
64, a chunk minus / plus one, several chunks), two parameter groups, gradients whose scale runs from 1e-6 to 1e+1, in both gradient
modes.  Every buffer the optimiser allocates is NaN-filled first (ops._empty), so an element no kernel writes shows."""
import copy
import functools

import pytest
import torch

import _adamw_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = (False, True)                                                             # flat_grads


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def make(flat, **kw):
    from omnifusion_amd import optim
    params = [torch.nn.Parameter(p.to(DEV)) for p in ar.params0()]
    return optim.AdamW(ar.group_dicts(params), flat_grads=flat, **kw), params


def set_grads(opt, params, gs):
    for p, g in zip(params, gs):
        if opt.flat_grads:
            p.grad.copy_(g) if g is not None else p.grad.zero_()
        else:
            p.grad = None if g is None else g.to(DEV)


def moments(opt, params):
    """the views of the two moment arenas in the order of `params` (the arena's own order is group by group)"""
    at = {id(p): i for i, p in enumerate(opt._params)}
    return [opt._m_views[at[id(p)]] for p in params], [opt._v_views[at[id(p)]] for p in params]


def result(opt, params):
    torch.cuda.synchronize()
    m, v = moments(opt, params)
    return {"p0": ar.params0(), "p": [p.detach().cpu() for p in params], "m": [t.cpu() for t in m], "v": [t.cpu() for t in v]}


def same_bits(a, b, skip=()):
    return all(torch.equal(x, y) for k in ("p", "m", "v") for i, (x, y) in enumerate(zip(a[k], b[k])) if i not in skip)


def run_case(name, flat, **kw):
    """CASES[name] on the device -> (result, the optimiser, the parameters)"""
    c = ar.CASES[name]
    opt, params = make(flat, max_grad_norm=c["max_norm"], **kw)
    if c["loaded"]:
        opt.load_state_dict(ar.loaded_state(opt))
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2) if c["sched"] else None
    for k in range(c["steps"]):
        set_grads(opt, params, ar.grads(k, c["gfactor"]))
        opt.step()
        if sched is not None:
            sched.step()
    return result(opt, params), opt, params


@functools.lru_cache(maxsize=None)
def loaded_run(flat):
    return run_case("loaded", flat)[0]


def test_one_step_from_loaded_state():
    runs = {flat: loaded_run(flat) for flat in MODES}
    for flat, got in runs.items():
        ar.check_gate("loaded", got, "flat" if flat else "pointers")
    assert same_bits(runs[False], runs[True])                                   # the two modes
    again, opt, _ = run_case("loaded", True)
    assert same_bits(runs[True], again)                                         # two runs
    assert int(opt.step_count) == ar.LOADED_STEP + 1 and int(opt.skipped_steps) == 0


@pytest.mark.parametrize("flat", MODES)
def test_ten_steps_with_a_scheduler(flat):
    got, opt, _ = run_case("ten", flat)
    ar.check_gate("ten", got, "flat" if flat else "pointers", direction=False)
    want = ar.run_torch("ten", torch.float64)["lrs"]
    assert int(opt.step_count) == 10 and want[0] != ar.GROUPS[0]["lr"]


@pytest.mark.parametrize("name", ["clip_above", "clip_below"])
def test_clipping(name):
    r64 = ar.reference(name)[0]
    norm64 = r64["norms"][0]
    assert (norm64 > 0.5) == (name == "clip_above")
    runs = []
    for flat in MODES:
        c = ar.CASES[name]
        opt, params = make(flat, max_grad_norm=c["max_norm"])
        opt.load_state_dict(ar.loaded_state(opt))
        gs = ar.grads(0, c["gfactor"])
        set_grads(opt, params, gs)
        opt.step()
        got = result(opt, params)
        norm = float(opt.grad_norm)
        print(f"adamw {name} [{'flat' if flat else 'pointers'}] grad_norm {norm!r}  float64 {norm64!r}  relative error {abs(norm - norm64) / norm64:.3e}")
        assert opt.grad_norm.dtype == torch.float32 and abs(norm - norm64) <= 2.0 ** -22 * norm64
        assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(params, gs))    # p.grad keeps its unclipped bits
        ar.check_gate(name, got, "flat" if flat else "pointers")
        runs.append(got)
    assert same_bits(*runs)


def test_pointer_mode():
    from omnifusion_amd import optim
    none = 5
    opt, params = make(False)
    opt.load_state_dict(ar.loaded_state(opt))
    m_before, v_before = (t[none].cpu() for t in moments(opt, params))
    gs = ar.grads(0)
    set_grads(opt, params, [None if i == none else g for i, g in enumerate(gs)])
    opt.step()
    got = result(opt, params)
    assert torch.equal(got["p"][none], ar.params0()[none]) and torch.equal(got["m"][none], m_before) and torch.equal(got["v"][none], v_before)
    assert same_bits(got, loaded_run(False), skip=(none,))                      # without clipping the others do not see the missing one
    fresh, fparams = make(False)
    set_grads(fresh, fparams, [None if i == none else g for i, g in enumerate(gs)])
    fresh.step()
    assert fparams[none] not in fresh.state and len(fresh.state) == len(fparams) - 1          # no gradient, no state: as torch
    assert set(fresh.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # gradients that are views ONE element into a larger buffer: 4-byte aligned only, the bits of the aligned copies
    opt, params = make(False)
    opt.load_state_dict(ar.loaded_state(opt))
    for p, g in zip(params, gs):
        big = torch.zeros(g.numel() + 9, device=DEV)
        big[1:1 + g.numel()].copy_(g)
        p.grad = big[1:1 + g.numel()]
        assert p.grad.data_ptr() % 16 == 4
    opt.step()
    assert same_bits(result(opt, params), loaded_run(False))
    # other strides than the parameter's
    w = torch.nn.Parameter(torch.randn(3, 5, device=DEV))
    o = optim.AdamW([w])
    w.grad = torch.randn(5, 3, device=DEV).t()
    with pytest.raises(ValueError, match="strides"):
        o.step()
    assert int(o.step_count) == 0


@pytest.mark.parametrize("flat", MODES)
def test_nonfinite_gradient(flat):
    bad_tensor, bad_element = 10, 1234
    g0, g1, g2 = ar.grads(0), ar.grads(1), ar.grads(2)
    g1[bad_tensor][bad_element] = float("inf")
    # skip_nonfinite=True: the bad step changes nothing but skipped_steps, the next step is the step of a run without it
    opt, params = make(flat, skip_nonfinite=True, max_grad_norm=0.5)
    clean, cparams = make(flat, skip_nonfinite=True, max_grad_norm=0.5)
    for o, ps in ((opt, params), (clean, cparams)):
        set_grads(o, ps, g0)
        o.step()
    before = result(opt, params)
    set_grads(opt, params, g1)
    opt.step()
    assert same_bits(result(opt, params), before) and int(opt.step_count) == 1 and int(opt.skipped_steps) == 1
    assert float(opt.grad_norm) == float("inf")
    for o, ps in ((opt, params), (clean, cparams)):
        set_grads(o, ps, g2)
        o.step()
    assert same_bits(result(opt, params), result(clean, cparams)) and int(opt.step_count) == 2 == int(clean.step_count)
    assert int(opt.skipped_steps) == 1 and int(clean.skipped_steps) == 0
    # the default: exactly the elements torch's float32 AdamW makes non-finite (no clipping)
    cpu = [torch.nn.Parameter(p.clone()) for p in ar.params0()]
    topt = torch.optim.AdamW(ar.group_dicts(cpu), foreach=False)
    opt, params = make(flat)
    for gs in (g0, g1):
        for p, g in zip(cpu, gs):
            p.grad = g.clone()
        topt.step()
        set_grads(opt, params, gs)
        opt.step()
    got = result(opt, params)
    assert int(opt.skipped_steps) == 0 and int(opt.step_count) == 2
    count = 0
    for i, p in enumerate(cpu):
        for mine, theirs in ((got["p"][i], p.detach()), (got["m"][i], topt.state[p]["exp_avg"]), (got["v"][i], topt.state[p]["exp_avg_sq"])):
            assert torch.equal(torch.isfinite(mine), torch.isfinite(theirs)), i
            count += int((~torch.isfinite(theirs)).sum())
    assert count == 3                                                           # p, exp_avg and exp_avg_sq of the one element


def device_torch_adamw(steps, first=0):
    params = [torch.nn.Parameter(p.to(DEV)) for p in ar.params0()]
    opt = torch.optim.AdamW(ar.group_dicts(params))
    for k in range(first, first + steps):
        for p, g in zip(params, ar.grads(k)):
            p.grad = g.to(DEV)
        opt.step()
    return opt, params


@pytest.mark.parametrize("flat", MODES)
def test_checkpoint_from_torch(flat):
    from omnifusion_amd import optim
    topt, params = device_torch_adamw(3)
    sd = copy.deepcopy(topt.state_dict())
    for p in params:
        p.grad = None
    opt = optim.AdamW(ar.group_dicts(params), flat_grads=flat)
    opt.load_state_dict(sd)
    assert int(opt.step_count) == 3
    for k in range(3, 6):
        set_grads(opt, params, ar.grads(k))
        opt.step()
    ar.check_gate("six", result(opt, params), "torch -> ours, " + ("flat" if flat else "pointers"))


def test_checkpoint_to_torch():
    opt, params = make(False)
    for k in range(3):
        set_grads(opt, params, ar.grads(k))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.AdamW(ar.group_dicts(tparams))
    theirs = topt.state_dict()
    topt.load_state_dict(sd)
    assert set(sd) == set(theirs) and set(sd["state"]) == set(range(len(params)))
    assert all(set(e) == {"step", "exp_avg", "exp_avg_sq"} for e in sd["state"].values())
    for mine, other in zip(sd["param_groups"], theirs["param_groups"]):
        assert set(mine) - set(other) == {"max_grad_norm", "skip_nonfinite", "flat_grads"} and set(other) <= set(mine)
        assert mine["params"] == other["params"]
    for p, g in zip(tparams, ar.grads(3)):
        p.grad = g.to(DEV)
    topt.step()
    torch.cuda.synchronize()
    got = {"p0": ar.params0(), "p": [p.detach().cpu() for p in tparams], "m": [topt.state[p]["exp_avg"].cpu() for p in tparams],
           "v": [topt.state[p]["exp_avg_sq"].cpu() for p in tparams]}
    ar.check_gate("four", got, "ours -> torch")
    # and back into a fresh optimiser of this class
    opt2, params2 = make(True)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(torch.equal(a, b) for a, b in zip(opt2._m_views, opt._m_views)) and int(opt2.step_count) == 3


def test_graph_replay_follows_gradients_and_lr():
    lrs = [(2e-3, 1e-3), (5e-4, 4e-3), (1e-3, 3e-3)]

    def sequence(graphed):
        opt, params = make(True, max_grad_norm=0.5)
        set_grads(opt, params, ar.grads(0))
        opt.step()                                                              # eager warm-up: kernels loaded before the capture
        graph = None
        if graphed:
            torch.cuda.synchronize()
            before = result(opt, params)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
            assert same_bits(result(opt, params), before) and int(opt.step_count) == 1      # capturing runs nothing
        for k, pair in enumerate(lrs):
            set_grads(opt, params, ar.grads(1 + k, 1e-4 if k == 1 else 1.0))
            for group, lr in zip(opt.param_groups, pair):
                group["lr"] = lr
            if graphed:
                opt.sync_hyperparameters()
                graph.replay()
            else:
                opt.step()
        out = result(opt, params)
        return out, int(opt.step_count), float(opt.grad_norm)

    eager, graphed = sequence(False), sequence(True)
    assert eager[1] == graphed[1] == 4 and eager[2] == graphed[2]
    assert same_bits(eager[0], graphed[0]) and not any(torch.isnan(p).any() for p in graphed[0]["p"])
    opt, params = make(False)
    set_grads(opt, params, ar.grads(0))
    opt.step()
    torch.cuda.synchronize()
    before = result(opt, params)
    graph, marker = torch.cuda.CUDAGraph(), torch.zeros(1, device=DEV)
    with torch.cuda.graph(graph):
        marker.add_(1.0)                                                        # (the capture is not empty)
        with pytest.raises(RuntimeError, match="captur"):
            opt.step()
    assert same_bits(result(opt, params), before)


def test_arena_over_a_converted_block():
    """Construction over an ops.convert-ed residual block whose conv1 weight is channels-last; then one forward / backward / step against
    float64 autograd + the float64 restatement.  eps = 1e-2: Adam's step lr . g / (|g| + eps) has slope <= lr / eps = 0.1 in g, so the
    convolution gate on the gradients (3e-5 of their rms) bounds the parameters' error; with eps = 1e-8 an element whose gradient is within
    the gradients' own error of zero would move by +-lr in either run, which says nothing about the optimiser."""
    import test_batchnorm_gpu as bn
    from omnifusion_amd import ops, optim
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-2, weight_decay=0.01)
    gen = torch.Generator().manual_seed(bn.BLOCK_SEED)
    sd = bn.block_state(gen)
    x, target = torch.randn(4, 64, 8, 8, generator=gen), torch.randn(4, 1, 8, 8, generator=gen)
    ref = bn.TorchBlock().double()
    ref.load_state_dict(sd)
    names = [k for k, _ in ref.named_parameters()]
    p64 = [p.detach().clone() for p in ref.parameters()]
    diff = ref(x.double()).mean(1, keepdim=True) - target.double()
    diff.abs().sum().backward()
    assert min(ref.z1.abs().min().item(), ref.z2.abs().min().item(), diff.abs().min().item()) >= bn.ZMARGIN
    r = ar.Restatement(p64, [0] * len(p64), [hyper], max_norm=0.5)
    r.step([p.grad for p in ref.parameters()])

    block, swapped = ops.convert(bn.TorchBlock())
    block.load_state_dict(sd)
    block.to(DEV)
    block.conv1.weight.data = block.conv1.weight.data.contiguous(memory_format=torch.channels_last)
    before = {k: (p, p.detach().clone(), p.stride()) for k, p in block.named_parameters()}
    keys = list(block.state_dict())
    assert before["conv1.weight"][2] != before["conv2.weight"][2]
    opt = optim.AdamW(block.parameters(), max_grad_norm=0.5, **hyper)
    assert list(block.state_dict()) == keys and [k for k, _ in block.named_parameters()] == names
    for k, p in block.named_parameters():
        assert p is before[k][0] and torch.equal(p.detach(), before[k][1]) and p.stride() == before[k][2], k
        lo, hi = opt.params_arena.data_ptr(), opt.params_arena.data_ptr() + 4 * opt.params_arena.numel()
        assert lo <= p.data_ptr() < hi and (p.data_ptr() - lo) % 256 == 0                     # it lives in the arena, at a multiple of 64 floats
    assert torch.isnan(opt.params_arena).sum() == 0
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    (block(cl(x)).mean(1, keepdim=True) - cl(target)).abs().sum().backward()
    opt.step()
    for k, want in zip(names, r.p):
        e = ar.nerr(before[k][0].detach().cpu(), want)
        print(f"adamw block {k} after the step: normalised error {e:.3e}  gate {bn.CONV_GATE:.1e}")
        assert e <= bn.CONV_GATE, (k, e)
    # a step between a forward and its backward: autograd refuses the backward, as with torch's optimiser
    out = block(cl(x))
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


@pytest.mark.parametrize("flat", MODES)
def test_the_real_model(flat):
    """model.trainable.spherical_fusion at test_train_model_gpu.py's configuration: all 222 tensors, the 1-element and 5-D ones included"""
    import test_train_model_gpu as tm
    from omnifusion_amd import optim
    from omnifusion_amd.supervision.direct import calculate_berhu_loss
    gen = torch.Generator().manual_seed(0)
    rgb = torch.rand(tm.BS, 3, tm.H, tm.W, generator=gen).to(DEV)
    gt = (1.0 + 3.0 * torch.rand(tm.BS, 1, tm.H, tm.W, generator=gen)).to(DEV)
    mask = (torch.rand(tm.BS, 1, tm.H, tm.W, generator=gen) < 0.9).float().to(DEV)
    net = tm.device_model()
    named = list(net.named_parameters())
    hyper = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt = optim.AdamW(net.parameters(), flat_grads=flat, max_grad_norm=0.5, **hyper)
    assert len(named) == 222 and min(p.numel() for _, p in named) == 1 and max(p.dim() for _, p in named) == 5
    p0 = [p.detach().cpu() for _, p in named]
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = calculate_berhu_loss(net(rgb, confidence=True), gt, mask, torch.ones_like(gt))
        loss.backward()
        if step == 0:
            grads = [p.grad.detach().cpu().clone() for _, p in named]
        opt.step()
        losses.append(loss.item())
        if step == 0:
            # the float64 formula on the fp32 gradients the device produced, against torch's CPU AdamW in float32 on the same gradients
            r = ar.Restatement(p0, [0] * len(p0), [hyper], max_norm=0.5)
            norm64 = r.step(grads)
            cpu = [torch.nn.Parameter(p.clone()) for p in p0]
            for p, g in zip(cpu, grads):
                p.grad = g.clone()
            torch.nn.utils.clip_grad_norm_(cpu, 0.5, foreach=False)
            torch.optim.AdamW(cpu, foreach=False, **hyper).step()
            assert abs(float(opt.grad_norm) - norm64) <= 2.0 ** -22 * norm64
            # one vector over all 222 tensors, as in the other tests: (p - p0) / lr
            direction = lambda after: torch.cat([((b.detach().cpu().double() - a.double()) / hyper["lr"]).reshape(-1) for b, a in zip(after, p0)])
            d64 = direction(r.p)
            gate = ar.FACTOR * max(ar.nerr(direction(cpu), d64), ar.FLOOR)
            got = direction([p for _, p in named])
            e = ar.nerr(got, d64)
            print(f"adamw real model [{'flat' if flat else 'pointers'}]: 222 tensors, (p - p0) / lr: normalised error {e:.3e}  gate {gate:.3e}  "
                  f"ratio {e / gate:.3f}")
            assert not torch.isnan(got).any() and e <= gate, f"{e:.3e} > {gate:.3e}"
    print("adamw real model, BerHu loss:", " ".join(f"{v:.6f}" for v in losses))
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert torch.isfinite(opt.params_arena).all() and torch.isfinite(opt.exp_avg).all() and torch.isfinite(opt.exp_avg_sq).all()
    assert int(opt.step_count) == 3
