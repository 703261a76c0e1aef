"""A rank of the synchronised batch normalisation's tests, started through dist.launch_command():

    _syncbn_rank_probe.py cpu  OUT     two ranks over gloo, CPU tensors: dist.all_gather_records, dist.sync_gradients (test_syncbn_cpu.py)
    _syncbn_rank_probe.py gpu  OUT     two ranks over gloo that share one GPU (test_syncbn_ranks_gpu.py): (a) ops.sync_batch_norm against
                                       float64, (b) a residual block's training step, (c) the whole model's forward, (d) the world-1 paths
    _syncbn_rank_probe.py gpu1 OUT     ONE process, no launcher, no process group: (d) alone

Every rank writes what it measured to OUT.<rank> (JSON) — the test asserts on it — and exits non-zero at its first failure, which ends the
other rank through the launcher; nothing is retried.  Rank 0 of `gpu` also saves the model's patches and buffers to OUT.model.pt for (c)."""
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omnifusion_amd import dist          # noqa: E402

MODE, OUT = sys.argv[1], sys.argv[2]
MODEL = (3, 10, (128, 128), (80, 80))                                           # nrows, patches, patch size, fov: the smallest the network admits
info = {}


def finish(rank):
    with open(f"{OUT}.{rank}", "w") as fh:
        json.dump(info, fh)
    dist.finalize()


def cpu_exchange():
    rank, _, world, _ = dist.init("gloo")
    info.update(rank=rank, world=world)
    vec = torch.tensor([0.5 + rank, 1.0 + rank, 2.0 ** -60], dtype=torch.float64)
    table = dist.all_gather_records(vec)
    assert table.shape == (world, 3) and table.dtype == torch.float64
    info["table"] = table.tolist()
    lin = torch.nn.Linear(3, 2)
    frozen = torch.nn.Parameter(torch.ones(4))                                  # no gradient: it does not travel
    lin.weight.grad, lin.bias.grad = torch.full((2, 3), 1.0 + rank), torch.full((2,), 10.0 * (1 + rank))
    w_grad = lin.weight.grad
    info["count"] = dist.sync_gradients(list(lin.parameters()) + [frozen])
    assert lin.weight.grad is w_grad                                            # in place
    info["grad_w"], info["grad_b"], info["frozen_untouched"] = lin.weight.grad.tolist(), lin.bias.grad.tolist(), frozen.grad is None
    lin.weight.grad = torch.full((2, 3), 1.0 + rank)
    lin.bias.grad = None
    dist.sync_gradients(lin, average=True)
    info["grad_avg"] = lin.weight.grad[0].tolist()
    finish(rank)


def same_on_all_ranks(tensors, world):
    """every tensor of the dict has the same bits on all ranks"""
    mine = {k: v.detach().cpu() for k, v in tensors.items()}
    if world == 1:
        return True
    every = [None] * world
    torch.distributed.all_gather_object(every, mine)
    return all(list(o) == list(mine) and all(torch.equal(o[k], mine[k]) for k in mine) for o in every)


def operator_vs_float64(rank, world, DEV):
    """(a) ops.sync_batch_norm on this rank's shard against the float64 reference on the concatenated batch"""
    import _syncbn_ref as sr
    from omnifusion_amd import ops
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    for name in ("odd105", "offset"):
        d, want, gate = sr.reference(name)
        act = sr.CASES[name][4]
        lo, hi = sr.bounds(name)[rank]
        leaf = {k: (None if d[k] is None else (d[k].to(DEV) if k in "wb" else cl(d[k][lo:hi])).requires_grad_(True)) for k in ("x", "w", "b", "res")}
        rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
        y = ops.sync_batch_norm(leaf["x"], leaf["w"], leaf["b"], rm, rv, res=leaf["res"], training=True, momentum=0.1, eps=1e-5, act=act)
        y.backward(cl(d["g"][lo:hi]))
        got = {"y": y.detach().cpu(), "x": leaf["x"].grad.cpu(), "res": None if leaf["res"] is None else leaf["res"].grad.cpu(),
               "rm": rm.cpu(), "rv": rv.cpu()}
        params = torch.stack([leaf["w"].grad, leaf["b"].grad]).cpu()            # the ranks' LOCAL sums: their total is the batch's gradient
        every = [None] * world
        torch.distributed.all_gather_object(every, params)
        got["w"], got["b"] = sum(e[0].double() for e in every), sum(e[1].double() for e in every)
        for k in sr.OUTS:
            if want[k] is None:
                continue
            w = want[k][lo:hi] if k in ("y", "x", "res") else want[k]
            # the normaliser is the whole tensor's rms (the gate's), the error this rank's slice
            e = ((got[k].double() - w.double()).abs().max() / max(1.0, want[k].double().pow(2).mean().sqrt().item())).item()
            info[f"a.{name}.{k}"] = [e, gate[k]]
            print(f"syncbn ranks [{rank}] (a) {name} {k}: normalised error {e:.3e}  gate {gate[k]:.3e}", flush=True)
            assert not torch.isnan(got[k]).any() and e <= gate[k], (name, k, e, gate[k])
        info[f"a.{name}.buffers_equal"] = same_on_all_ranks({"rm": rm, "rv": rv}, world)
        assert info[f"a.{name}.buffers_equal"], name


def residual_block_step(rank, world, DEV):
    """(b) conv -> BN + ReLU -> conv -> BN + identity + ReLU: global [4,64,8,8], two items per rank, one SGD step"""
    import test_batchnorm_gpu as bn
    from omnifusion_amd import ops
    from omnifusion_amd.sync_batchnorm import convert_model
    gen = torch.Generator().manual_seed(bn.BLOCK_SEED)
    sd = bn.block_state(gen)
    x, target = torch.randn(4, 64, 8, 8, generator=gen), torch.randn(4, 1, 8, 8, generator=gen)
    ref = bn.TorchBlock().double()
    ref.load_state_dict(sd)
    dx64, g64, diff64 = bn.block_step(ref, x.double(), target.double())
    assert min(ref.z1.abs().min().item(), ref.z2.abs().min().item(), diff64.abs().min().item()) >= bn.ZMARGIN
    block, names = ops.convert(bn.TorchBlock())
    block = convert_model(block)
    assert names == ["conv1", "bn1", "conv2", "bn2"] and type(block.bn1) is ops.SyncBatchNorm2d and type(block.bn2) is ops.SyncBatchNorm2d
    block.load_state_dict(sd)
    block.to(DEV)
    lo, hi = dist.shard(4, rank, world)
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    xl = cl(x[lo:hi]).requires_grad_(True)
    opt = torch.optim.SGD(block.parameters(), lr=0.1)
    (block(xl).mean(1, keepdim=True) - cl(target[lo:hi])).abs().sum().backward()          # the LOCAL summed L1 loss
    dist.sync_gradients(block, average=False)
    got = {k: p.grad.detach().cpu() for k, p in block.named_parameters()}
    opt.step()
    for k, want in g64.items():
        e = bn.nerr(got[k], want)
        info[f"b.grad.{k}"] = [e, bn.CONV_GATE]
        print(f"syncbn ranks [{rank}] (b) d{k}: normalised error {e:.3e}  gate {bn.CONV_GATE:.1e}", flush=True)
        assert not torch.isnan(got[k]).any() and e <= bn.CONV_GATE, (k, e)
    e = ((xl.grad.cpu().double() - dx64[lo:hi]).abs().max() / max(1.0, dx64.pow(2).mean().sqrt().item())).item()
    info["b.grad.x"] = [e, bn.CONV_GATE]
    print(f"syncbn ranks [{rank}] (b) dx (local): normalised error {e:.3e}  gate {bn.CONV_GATE:.1e}", flush=True)
    assert e <= bn.CONV_GATE, e
    after, after64 = block.state_dict(), ref.state_dict()
    for k, want in after64.items():
        if k.endswith("num_batches_tracked"):
            info[f"b.after.{k}"] = int(after[k])
            assert int(after[k]) == int(want) == 1, k
        else:
            e = bn.nerr(after[k].cpu(), want)
            info[f"b.after.{k}"] = [e, bn.CONV_GATE]
            assert e <= bn.CONV_GATE, (k, e)
    info["b.state_equal"] = same_on_all_ranks(after, world)
    assert info["b.state_equal"]


def whole_model_forward(rank, world, DEV):
    """(c) one training-mode forward of the converted model, one panorama per rank; rank 0 leaves the patches of the global batch and its
    buffers for the test's float64 restatement"""
    from omnifusion_amd import _lib, ops
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
    from omnifusion_amd.model import trainable
    from omnifusion_amd.sync_batchnorm import convert_model
    from omnifusion_amd.weights import make_state_dict
    net = trainable.spherical_fusion(*MODEL)
    net.load_state_dict(make_state_dict(42, MODEL[1]))
    net = convert_model(net).to(DEV)
    assert net.training and type(net.bn1) is ops.SyncBatchNorm2d and type(net.mlp_points[1]) is ops.BatchNorm2d
    rgb = torch.rand(world, 3, 128, 256, generator=torch.Generator().manual_seed(0))
    out = net(rgb[rank:rank + 1].to(DEV))
    assert out.shape == (1, 1, 128, 256) and torch.isfinite(out).all()
    buffers = {k: v for k, v in net.named_buffers()}
    info["c.tracked"] = sorted({int(v) for k, v in buffers.items() if k.endswith("num_batches_tracked")})
    info["c.buffers"] = len(buffers)
    info["c.buffers_equal"] = same_on_all_ranks(buffers, world)
    assert info["c.buffers_equal"] and info["c.tracked"] == [1]
    if rank == 0:
        patches = equi2pers_patches(rgb.to(DEV), MODEL[3], MODEL[0], MODEL[2], layout=_lib.LAYOUT_BNCHW)
        torch.save({"patches": patches.cpu(), "stats": {k: v.cpu() for k, v in buffers.items() if not k.endswith("num_batches_tracked")}},
                   OUT + ".model.pt")


def world_one_paths(DEV, groups):
    """(d) a SyncBatchNorm2d whose statistics are nobody else's IS ops.BatchNorm2d: in eval mode, and in training mode at world 1 (`groups`:
    the process groups to construct it with — None without a launcher, a one-rank group under it)"""
    import _syncbn_ref as sr
    from omnifusion_amd import ops
    d, _, _ = sr.reference("odd105")
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)

    def run(layer, train):
        layer.load_state_dict({"weight": d["w"], "bias": d["b"], "running_mean": d["rm"], "running_var": d["rv"],
                               "num_batches_tracked": torch.tensor(0)})
        layer.to(DEV).train(train)
        x, res = cl(d["x"]).requires_grad_(True), cl(d["res"]).requires_grad_(True)
        layer(x, res=res).backward(cl(d["g"]))
        return [x.grad, res.grad, layer.weight.grad, layer.bias.grad, layer.running_mean, layer.running_var, layer.num_batches_tracked]

    checks = [("eval", None, False)] + [(f"train{i}", g, True) for i, g in enumerate(groups)]
    for what, group, train in checks:
        got = run(ops.SyncBatchNorm2d(32, act="relu", process_group=group), train)
        want = run(ops.BatchNorm2d(32, act="relu"), train)
        info[f"d.{what}"] = all(torch.equal(a, b) for a, b in zip(got, want)) and not any(torch.isnan(a).any() for a in got)
        assert info[f"d.{what}"], what


def gpu_ranks():
    torch.distributed.init_process_group("gloo", timeout=datetime.timedelta(seconds=60)) if "WORLD_SIZE" in os.environ else None
    rank, _, world, DEV = dist.init("gloo")
    assert DEV.type == "cuda", "the probe's gpu modes need an MI355X"
    info.update(rank=rank, world=world)
    from omnifusion_amd import ops
    ops._empty = lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), float("nan"), **kw)    # an unwritten element shows
    if MODE == "gpu1":
        assert world == 1 and not torch.distributed.is_initialized()
        world_one_paths(DEV, [None])
        return finish(rank)
    assert world == 2
    operator_vs_float64(rank, world, DEV)
    residual_block_step(rank, world, DEV)
    whole_model_forward(rank, world, DEV)
    ones = [torch.distributed.new_group([r], backend="gloo") for r in range(world)]           # every rank creates every group
    world_one_paths(DEV, [ones[rank]])
    finish(rank)


if __name__ == "__main__":
    cpu_exchange() if MODE == "cpu" else gpu_ranks()
