"""A rank of the optimiser's two-rank test, started through dist.launch_command():

    _optim_rank_probe.py OUT     two ranks over gloo that share one GPU (test_optim_ranks_gpu.py): a residual block with SyncBatchNorm2d,
                                 optim.AdamW(flat_grads=True), two training steps on each rank's half of the batch

Every rank writes what it measured to OUT.<rank> (JSON) — the test asserts on it — and exits non-zero at its first failure, which ends the
other rank through the launcher; nothing is retried."""
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omnifusion_amd import dist          # noqa: E402

OUT = sys.argv[1]
info = {}


def same_on_all_ranks(tensors, world):
    """every tensor of the dict has the same bits on all ranks"""
    mine = {k: v.detach().cpu() for k, v in tensors.items()}
    every = [None] * world
    torch.distributed.all_gather_object(every, mine)
    return all(list(o) == list(mine) and all(torch.equal(o[k], mine[k]) for k in mine) for o in every)


def main():
    torch.distributed.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    rank, _, world, DEV = dist.init("gloo")
    assert DEV.type == "cuda" and world == 2, "the probe needs an MI355X and two ranks"
    info.update(rank=rank, world=world)
    import test_batchnorm_gpu as bn
    from omnifusion_amd import ops, optim
    from omnifusion_amd.sync_batchnorm import convert_model
    ops._empty = lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), float("nan"), **kw)    # an unwritten element shows
    gen = torch.Generator().manual_seed(bn.BLOCK_SEED)
    sd = bn.block_state(gen)
    block, _ = ops.convert(bn.TorchBlock())
    block = convert_model(block)
    block.load_state_dict(sd)
    block.to(DEV)
    assert type(block.bn1) is ops.SyncBatchNorm2d
    opt = optim.AdamW(block.parameters(), lr=1e-3, max_grad_norm=0.5, flat_grads=True)
    params = list(block.parameters())
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    lo, hi = dist.shard(4, rank, world)
    for step in range(2):
        x, target = torch.randn(4, 64, 8, 8, generator=gen), torch.randn(4, 1, 8, 8, generator=gen)
        opt.zero_grad()
        (block(cl(x[lo:hi])).mean(1, keepdim=True) - cl(target[lo:hi])).abs().sum().backward()          # the LOCAL summed L1 loss
        assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, opt._g_views))            # autograd accumulated in place
        local = {i: p.grad.detach().clone() for i, p in enumerate(params)}
        info[f"{step}.local_differs"] = not same_on_all_ranks(local, world)
        # dist.sync_gradients on clones of the same gradients: the bits opt.sync_gradients must leave
        clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for c, p in zip(clones, params):
            c.grad = p.grad.detach().clone()
        assert dist.sync_gradients(clones) == len(params)
        assert opt.sync_gradients() == len(params)
        info[f"{step}.sync_bits"] = all(torch.equal(c.grad, p.grad) for c, p in zip(clones, params))
        info[f"{step}.sync_changed"] = not all(torch.equal(local[i], p.grad) for i, p in enumerate(params))
        assert info[f"{step}.sync_bits"] and info[f"{step}.sync_changed"], step
        opt.step()
        state = {"params": opt.params_arena, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "grad_norm": opt.grad_norm,
                 "step_count": opt.step_count}
        info[f"{step}.finite"] = all(bool(torch.isfinite(v.float()).all()) for v in state.values())
        info[f"{step}.state_equal"] = same_on_all_ranks(state, world)
        info[f"{step}.grad_norm"] = float(opt.grad_norm)
        print(f"optim ranks [{rank}] step {step}: grad_norm {info[f'{step}.grad_norm']!r}  equal across ranks {info[f'{step}.state_equal']}", flush=True)
        assert info[f"{step}.finite"] and info[f"{step}.state_equal"], step
    info["steps"] = int(opt.step_count)
    with open(f"{OUT}.{rank}", "w") as fh:
        json.dump(info, fh)
    dist.finalize()


if __name__ == "__main__":
    main()
