"""CPU: the optimiser's host side (omnifusion_amd/optim.py) — the arena's layout function, the float64 restatement the GPU
tests are read against (tests/_adamw_ref.py) held to torch.optim.AdamW itself, and the constructor's rejections, all of which come before
anything touches a GPU."""
import pytest
import torch

import _adamw_ref as ar
from omnifusion_amd import optim


def test_layout_covers_every_element_once():
    offsets, total, chunks = optim.layout(ar.SIZES)
    assert len(offsets) == len(ar.SIZES) and all(o % 64 == 0 for o in offsets) and total % 64 == 0
    assert offsets[0] == 0 and all(b >= a + n for a, b, n in zip(offsets, offsets[1:] + [total], ar.SIZES))       # segments do not overlap
    assert total == sum(-(-n // 64) * 64 for n in ar.SIZES)
    seen = torch.zeros(total, dtype=torch.int32)
    per_segment = [0] * len(ar.SIZES)
    for s, o in chunks:
        assert 0 <= s < len(ar.SIZES) and o % optim.CHUNK == 0 and 0 <= o < ar.SIZES[s]          # starts at the segment's start, a whole number of chunks in
        count = min(optim.CHUNK, ar.SIZES[s] - o)                                              # what the kernels take: never past the segment
        assert 1 <= count <= optim.CHUNK
        seen[offsets[s] + o: offsets[s] + o + count] += 1
        per_segment[s] += count
    assert per_segment == ar.SIZES
    inside = torch.zeros(total, dtype=torch.bool)
    for off, n in zip(offsets, ar.SIZES):
        inside[off:off + n] = True
    assert torch.equal(seen == 1, inside) and int(seen[~inside].sum()) == 0                    # every element once, the padding never
    assert chunks == sorted(chunks) and len(set(chunks)) == len(chunks)
    assert len(chunks) == sum(-(-n // optim.CHUNK) for n in ar.SIZES)
    # a pure function of the sizes; the real model's shape of the problem: many tiny tensors
    assert optim.layout(ar.SIZES) == (offsets, total, chunks)
    assert optim.layout([1] * 5) == ([0, 64, 128, 192, 256], 320, [(i, 0) for i in range(5)])
    assert optim.layout([0, 3]) == ([0, 0], 64, [(1, 0)])
    with pytest.raises(ValueError):
        optim.layout([2 ** 31])


def test_restatement_equals_torch_adamw_in_float64():
    """five steps of clip_grad_norm_(..., 0.5) + torch.optim.AdamW with a CosineAnnealingWarmRestarts step in between, in float64"""
    params = [torch.nn.Parameter(p.double()) for p in ar.params0()]
    opt = torch.optim.AdamW(ar.group_dicts(params), foreach=False)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2)
    mine = ar.Restatement(ar.params0(), ar.GROUP_OF, ar.GROUPS, max_norm=0.5)
    for k in range(5):
        gfactor = 1.0 if k % 2 == 0 else 1e-4                                                  # the norm above and below 0.5
        gs = [g.double() for g in ar.grads(k, gfactor)]
        for p, g in zip(params, gs):
            p.grad = g.clone()
        norm = float(torch.nn.utils.clip_grad_norm_(params, 0.5, foreach=False))
        assert (norm > 0.5) == (k % 2 == 0)
        for g, group in zip(mine.groups, opt.param_groups):
            g["lr"] = group["lr"]
        opt.step()
        sched.step()
        assert abs(mine.step(gs) - norm) <= 1e-13 * norm
        for i, p in enumerate(params):
            for got, want in ((mine.p[i], p.detach()), (mine.m[i], opt.state[p]["exp_avg"]), (mine.v[i], opt.state[p]["exp_avg_sq"])):
                assert (got - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1e-300), (k, i)
    assert len({round(g["lr"], 12) for g in opt.param_groups}) == 2 and opt.param_groups[0]["lr"] != ar.GROUPS[0]["lr"]    # the schedule moved


def test_constructor_errors_come_before_any_gpu_call(monkeypatch):
    from omnifusion_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    P = torch.nn.Parameter
    with pytest.raises(ValueError, match="no CPU path"):
        optim.AdamW([P(torch.zeros(3))])
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([P(torch.zeros(3))], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([dict(params=[P(torch.zeros(3))], amsgrad=True)])
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([P(torch.zeros(3))], maximize=True)
    with pytest.raises(ValueError, match="fp32 parameters only"):
        optim.AdamW([P(torch.zeros(3, dtype=torch.float16))])
    shared = P(torch.zeros(3))
    with pytest.raises(ValueError, match="more than one parameter group"):
        optim.AdamW([dict(params=[shared]), dict(params=[shared], lr=1.0)])
    with pytest.raises(ValueError):
        optim.AdamW([P(torch.zeros(3))], lr=-1.0)
    with pytest.raises(ValueError):
        optim.AdamW([P(torch.zeros(3))], max_grad_norm=-0.5)
