"""CPU: the synchronised batch normalisation's boundary — the float64 restatement of its four phases against torch autograd
on the concatenated batch, every rejection of the C calls and of ops.sync_batch_norm / SyncBatchNorm2d / convert_sync_batchnorm before a
launch, sync_batchnorm.convert_model on both trainable models, and dist.all_gather_records / dist.sync_gradients at world 2 over gloo."""
import ctypes
import json
import os
import subprocess

import pytest
import torch

import _syncbn_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "_syncbn_rank_probe.py")


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_the_four_phases_in_float64_are_batch_norm_on_the_concatenation(name):
    """records -> rank-ordered totals -> the two formulas, against F.batch_norm + autograd on the concatenated batch, both in float64.  The
    tolerance is the restatement's own rounding (sr.restatement_bound).  Measured: at most 1.6e-14 (rows10240, dx) on every case but `offset`, 3.7e-9
    there (dx; bounds 1.1e-13 .. 1.2e-12 and 1.1e-6)."""
    d, want, _ = sr.reference(name)
    act = sr.CASES[name][4]
    cut = lambda t: [None if t is None else t[lo:hi] for lo, hi in sr.bounds(name)]
    got = sr.phases(cut(d["x"]), cut(d["res"]), cut(d["g"]), d["w"], d["b"], d["rm"], d["rv"], 0.1, 1e-5, act)
    bound = sr.restatement_bound(d["x"])
    whole = {k: sr.like(torch.cat(got[k]), d["x"]) for k in ("y", "x", "res")}
    whole.update(w=sum(got["w"]), b=sum(got["b"]), rm=got["rm"], rv=got["rv"])
    for k in sr.OUTS:
        if want[k] is None:
            continue
        e = sr.nerr(whole[k], want[k])
        print(f"syncbn restatement {name} {k}: normalised error {e:.3e}  bound {bound:.3e}")
        assert e <= bound, (name, k, e, bound)
    if len(sr.CASES[name][6]) > 1 and name != "rows18":                        # one shard's OWN statistics are not the batch's
        local = sr.phases(cut(d["x"])[:1], cut(d["res"])[:1], cut(d["g"])[:1], d["w"], d["b"], d["rm"], d["rv"], 0.1, 1e-5, act)
        assert not sr.nerr(local["rv"], want["rv"]) <= 1e-6


def test_package_names_and_layer():
    from omnifusion_amd import ops, sync_batchnorm as sb
    assert sb.SynchronizedBatchNorm2d is ops.SyncBatchNorm2d and issubclass(ops.SyncBatchNorm2d, ops.BatchNorm2d)
    assert callable(sb.convert_model) and callable(ops.sync_batch_norm) and callable(ops.convert_sync_batchnorm)
    with pytest.raises(NotImplementedError, match="one process per GPU"):
        sb.DataParallelWithCallback(torch.nn.Identity())
    layer = ops.SyncBatchNorm2d(64, act="relu")
    assert layer.act == "relu" and layer.process_group is None
    assert list(layer.state_dict()) == list(torch.nn.BatchNorm2d(64).state_dict())
    assert [n for n, _ in layer.named_buffers()] == ["running_mean", "running_var", "num_batches_tracked"]
    assert ops.SyncBatchNorm2d(16, process_group="g").process_group == "g"
    with pytest.raises(ValueError, match="momentum=None"):
        ops.SyncBatchNorm2d(32, momentum=None)
    with pytest.raises(ValueError, match="act must be"):
        ops.SyncBatchNorm2d(32, act="gelu")
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.SyncBatchNorm2d(6)


def test_symbols_and_c_boundary_reject_before_touching_a_device():
    """Every rejection of the four calls.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "omnifusion.h")).read()
    for name in ("omni_syncbn_stats_f32", "omni_syncbn_fwd_apply_f32", "omni_syncbn_bwd_reduce_f32", "omni_syncbn_bwd_apply_f32"):
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(L, name), name
    p, odd, z = ctypes.c_void_p(4096), ctypes.c_void_p(4100), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    big = 1 << 30
    err = L.omni_last_error

    def stats(x=p, sums=p, rows=64, C=32, ws=p, nb=big):
        return L.omni_syncbn_stats_f32(x, sums, rows, C, ws, nb, z)

    assert stats(x=z) == INV and b"null" in err()
    assert stats(sums=z) == INV and stats(sums=odd) == INV and b"aligned" in err()
    for C in (0, -4, 6, 30):
        assert stats(C=C) == INV and b"multiple of 4" in err(), C
    assert stats(rows=0) == INV and stats(rows=-1) == INV
    assert stats(nb=16) == INV and b"workspace" in err()
    assert stats(ws=z) == INV and stats(rows=1 << 31) == UNS

    def fwd(x=p, res=p, gamma=p, beta=p, table=p, world=2, rm=p, rv=p, y=p, saved=p, rows=64, C=32, momentum=0.1, eps=1e-5, act=0):
        return L.omni_syncbn_fwd_apply_f32(x, res, gamma, beta, table, world, rm, rv, y, saved, rows, C, momentum, eps, act, z)

    assert fwd(x=z) == INV and fwd(y=z) == INV and fwd(saved=z) == INV and fwd(table=z) == INV and b"null" in err()
    for world in (0, -1, 65, 1 << 20):
        assert fwd(world=world) == INV and b"world" in err(), world
    assert fwd(table=odd) == INV and b"aligned" in err()
    for C in (0, 6):
        assert fwd(C=C) == INV and b"multiple of 4" in err()
    assert fwd(rows=0) == INV
    assert fwd(rows=1, world=1) == INV and b"more than 1 value per channel" in err()
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert fwd(eps=eps) == INV and b"eps" in err(), eps
    for m in (-0.01, 1.01, float("nan")):
        assert fwd(momentum=m) == INV and b"momentum" in err(), m
    assert fwd(rm=z) == INV and fwd(rv=z) == INV and b"come together" in err()
    assert fwd(act=2) == UNS and b"GELU" in err()
    assert fwd(act=7) == INV

    def red(g=p, x=p, y=p, saved=p, dz=z, sums=p, dgamma=p, dbeta=p, rows=64, C=32, act=0, ws=p, nb=big):
        return L.omni_syncbn_bwd_reduce_f32(g, x, y, saved, dz, sums, dgamma, dbeta, rows, C, act, ws, nb, z)

    assert red(g=z) == INV and red(x=z) == INV and red(saved=z) == INV and red(sums=z) == INV and b"null" in err()
    assert red(sums=odd) == INV and b"aligned" in err()
    assert red(act=1, y=z) == INV and b"ReLU" in err()
    assert red(act=0, dz=p) == INV and b"g itself" in err()
    assert red(C=30) == INV and red(rows=0) == INV and red(act=2) == UNS and red(act=5) == INV
    assert red(nb=16) == INV and b"workspace" in err()
    assert red(ws=z) == INV and red(rows=1 << 31) == UNS

    def app(g=p, y=p, x=p, gamma=p, saved=p, table=p, world=2, dx=p, dres=z, rows=64, C=32, act=0):
        return L.omni_syncbn_bwd_apply_f32(g, y, x, gamma, saved, table, world, dx, dres, rows, C, act, z)

    assert app(g=z) == INV and b"null" in err()
    assert app(dx=z) == INV and b"no gradient requested" in err()
    assert app(x=z) == INV and app(saved=z) == INV and app(table=z) == INV and b"null" in err()
    for world in (0, 65):
        assert app(world=world) == INV and b"world" in err(), world
    assert app(table=odd) == INV and b"aligned" in err()
    assert app(act=0, dres=p) == INV and app(act=1, y=z, dres=p) == INV and b"dres" in err()
    assert app(rows=1, world=1) == INV and b"more than 1 value per channel" in err()
    assert app(C=6) == INV and app(rows=0) == INV and app(act=2) == UNS and app(act=9) == INV and app(rows=1 << 31) == UNS


def test_python_errors(monkeypatch):
    """Every ValueError of sync_batch_norm on the path that would exchange (world 2), raised before a launch and before a collective."""
    from omnifusion_amd import ops
    launched = []
    monkeypatch.setattr(ops._SyncBatchNorm, "apply", staticmethod(lambda *a: launched.append(a)))
    x = torch.rand(2, 32, 4, 4)
    v = lambda n=32: dev(torch.rand(n))
    X = dev(x)
    monkeypatch.setattr(ops, "_syncbn_world", lambda group: 1)                 # world 1: ops.batch_norm itself, with its own messages
    with pytest.raises(ValueError, match="x must be a tensor on an MI355X device; there is no CPU path"):
        ops.sync_batch_norm(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        ops.sync_batch_norm(dev(torch.rand(1, 32, 1, 1)))
    monkeypatch.setattr(ops, "_syncbn_world", lambda group: 65)
    with pytest.raises(ValueError, match="at most 64 ranks"):
        ops.sync_batch_norm(X)
    monkeypatch.setattr(ops, "_syncbn_world", lambda group: 2)
    with pytest.raises(ValueError, match="x must be a tensor on an MI355X device; there is no CPU path"):
        ops.sync_batch_norm(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.SyncBatchNorm2d(32)(x)
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.sync_batch_norm(x.numpy())
    with pytest.raises(ValueError, match="weight must be a tensor on an MI355X device"):
        ops.sync_batch_norm(X, torch.rand(32))
    with pytest.raises(ValueError, match="float32"):
        ops.sync_batch_norm(dev(x.double()))
    with pytest.raises(ValueError, match=r"non-empty \[M,C,H,W\]"):
        ops.sync_batch_norm(dev(torch.rand(2, 32, 4)))
    with pytest.raises(ValueError, match="non-empty"):
        ops.sync_batch_norm(dev(torch.rand(0, 32, 4, 4)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.sync_batch_norm(dev(torch.rand(2, 6, 4, 4)))
    for kw in ({"weight": v(16)}, {"bias": v(16)}, {"running_mean": v(16), "running_var": v()}, {"running_mean": v(), "running_var": v(64)}):
        with pytest.raises(ValueError, match=next(iter(kw)) if len(kw) == 1 else r"running_\w+ must be \[C\]"):
            ops.sync_batch_norm(X, **kw)
    with pytest.raises(ValueError, match="come together"):
        ops.sync_batch_norm(X, running_mean=v())
    with pytest.raises(ValueError, match="cannot require a gradient"):
        ops.sync_batch_norm(X, running_mean=dev(torch.rand(32).requires_grad_(True)), running_var=v())
    with pytest.raises(ValueError, match="res must have x's shape"):
        ops.sync_batch_norm(X, res=dev(torch.rand(2, 32, 4, 2)))
    with pytest.raises(ValueError, match="gelu.*'none' and 'relu' only"):
        ops.sync_batch_norm(X, act="gelu")
    with pytest.raises(ValueError, match="'none' or 'relu'"):
        ops.sync_batch_norm(X, act="tanh")
    with pytest.raises(ValueError, match="momentum=None"):
        ops.sync_batch_norm(X, momentum=None)
    for m in (-0.1, 1.5, float("nan"), "0.1"):
        with pytest.raises(ValueError, match=r"momentum must be a number in \[0, 1\]"):
            ops.sync_batch_norm(X, momentum=m)
    for eps in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="eps must be a positive finite number"):
            ops.sync_batch_norm(X, eps=eps)
    with pytest.raises(ValueError, match="training=False needs running_mean"):      # eval mode is ops.batch_norm at any world
        ops.sync_batch_norm(X, training=False)
    assert launched == []
    ops.sync_batch_norm(dev(torch.rand(1, 32, 1, 1)))                          # ONE value per channel on this rank: accepted when world > 1
    ops.sync_batch_norm(X, v(), v(), v(), v(), res=X, act="relu", group="g")
    assert len(launched) == 2 and launched[1][-2:] == ("g", 2)
    with pytest.raises(ValueError, match=r"float64 \[2, 65\]"):
        ops._check_syncbn_records("t", torch.zeros(1, 65, dtype=torch.float64), 2, 32, torch.device("cpu"))
    with pytest.raises(ValueError, match="float64"):
        ops._check_syncbn_records("t", torch.zeros(2, 65), 2, 32, torch.device("cpu"))


def test_convert_sync_batchnorm_on_a_small_model():
    from omnifusion_amd import ops
    nn = torch.nn
    model = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), ops.BatchNorm2d(64, act="relu"),
                          nn.BatchNorm2d(64, momentum=None), nn.BatchNorm2d(6),
                          nn.Sequential(ops.BatchNorm2d(32), ops.BatchNorm2d(32)))
    model[2].eval()
    hook = model[2].register_forward_hook(lambda *a: None)
    tensors = {k: id(t) for k, t in list(model.named_parameters()) + list(model.named_buffers())}
    keys = list(model.state_dict())
    old = list(model)
    out, names = ops.convert_sync_batchnorm(model, process_group="pg", skip=("5.1",))
    assert out is model and names == ["1", "2", "5.0"]
    assert type(model[0]) is nn.Conv2d and model[0] is old[0]                                  # convolutions are ops.convert's business
    assert type(model[1]) is ops.SyncBatchNorm2d and model[1].act == "none" and model[1].training
    assert type(model[2]) is ops.SyncBatchNorm2d and model[2].act == "relu" and not model[2].training
    assert hook.id in model[2]._forward_hooks
    assert model[3] is old[3] and model[4] is old[4]                                          # out of scope: left alone
    assert type(model[5][0]) is ops.SyncBatchNorm2d and type(model[5][1]) is ops.BatchNorm2d   # the skipped name
    assert all(m.process_group == "pg" for m in model.modules() if isinstance(m, ops.SyncBatchNorm2d))
    assert {k: id(t) for k, t in list(model.named_parameters()) + list(model.named_buffers())} == tensors
    assert list(model.state_dict()) == keys
    assert ops.convert_sync_batchnorm(model, skip=("5.1",))[1] == []                           # twice: a no-op
    assert ops.convert_sync_batchnorm(model)[1] == ["5.1"]
    root, names = ops.convert_sync_batchnorm(nn.BatchNorm2d(16))
    assert type(root) is ops.SyncBatchNorm2d and names == [""]
    pre = nn.Sequential()
    pre.add_module("mlp_points", ops.BatchNorm2d(16))
    pre.add_module("mlp_points1", ops.BatchNorm2d(16))
    assert ops.convert_sync_batchnorm(pre, skip=("mlp_points",))[1] == ["mlp_points1"]         # a prefix ends at a dot
    with pytest.raises(ValueError, match="not a string"):
        ops.convert_sync_batchnorm(model, skip="5.1")
    with pytest.raises(ValueError, match="non-empty name prefixes"):
        ops.convert_sync_batchnorm(model, skip=("",))
    with pytest.raises(ValueError, match="non-empty name prefixes"):
        ops.convert_sync_batchnorm(model, skip=(3,))
    with pytest.raises(ValueError, match="nn.Module"):
        ops.convert_sync_batchnorm([model])


@pytest.mark.parametrize("which", ["single_pass", "iterative"])
def test_convert_model_on_the_trainable_models(which):
    from omnifusion_amd import ops
    from omnifusion_amd.model import trainable, trainable_iterative
    from omnifusion_amd.sync_batchnorm import convert_model
    net, local = ((trainable.spherical_fusion(3, 10, (128, 128), (80, 80)), "mlp_points") if which == "single_pass" else
                  (trainable_iterative.spherical_fusion(3, 10, (128, 128), (80, 80)), "mlp_points1"))
    assert type(net).SYNCBN_REPLICATED == (local,)
    before = [(k, id(v)) for k, v in net.state_dict(keep_vars=True).items()]
    bns = [n for n, m in net.named_modules() if isinstance(m, ops.BatchNorm2d)]
    acts = {n: m.act for n, m in net.named_modules() if isinstance(m, ops.BatchNorm2d)}
    assert convert_model(net) is net
    assert [(k, id(v)) for k, v in net.state_dict(keep_vars=True).items()] == before           # keys, order and tensor objects
    kept = [n for n in bns if n.startswith(local + ".")]
    assert kept == [local + ".1", local + ".4"]
    for n, m in net.named_modules():
        if n in bns:
            assert type(m) is (ops.BatchNorm2d if n in kept else ops.SyncBatchNorm2d), n
            assert m.act == acts[n] and m.training and (n in kept or m.process_group is None), n
    assert len(bns) - len(kept) >= 40
    classes = [type(m) for m in net.modules()]
    assert convert_model(net) is net and [type(m) for m in net.modules()] == classes           # twice: a no-op
    assert ops.convert_sync_batchnorm(net, skip=type(net).SYNCBN_REPLICATED)[1] == []
    assert ops.convert_sync_batchnorm(net)[1] == kept                                          # skip=(): the reference's "everything"


def test_world_one_creates_no_group():
    from omnifusion_amd import dist
    vec = torch.arange(5, dtype=torch.float64)
    table = dist.all_gather_records(vec)
    assert table.shape == (1, 5) and table.data_ptr() == vec.data_ptr()
    lin = torch.nn.Linear(3, 2)
    lin.weight.grad = torch.ones(2, 3)
    assert dist.sync_gradients(lin, average=True) == 1 and torch.equal(lin.weight.grad, torch.ones(2, 3)) and lin.bias.grad is None
    assert dist.sync_gradients([lin.bias]) == 0
    with pytest.raises(ValueError, match="a record is a vector"):
        dist.all_gather_records(torch.zeros(2, 3, dtype=torch.float64))
    assert not torch.distributed.is_initialized()


def test_exchange_at_world_two_over_gloo(tmp_path):
    """dist.all_gather_records and dist.sync_gradients with CPU tensors, two ranks under the launcher (the probe's `cpu` mode)"""
    from omnifusion_amd import dist
    out = str(tmp_path / "probe.json")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(dist.launch_command(PROBE, ["cpu", out], 2), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = [json.load(open(f"{out}.{rank}")) for rank in range(2)]
    for rank, i in enumerate(info):
        assert i["world"] == 2 and i["rank"] == rank
        assert i["table"] == [[0.5, 1.0, 2.0 ** -60], [1.5, 2.0, 2.0 ** -60]]                  # rank order, float64 bits intact
        assert i["grad_w"] == [[3.0] * 3] * 2 and i["grad_b"] == [30.0, 30.0]                  # (1 + 2), (10 + 20): added, in place
        assert i["grad_avg"] == [1.5] * 3 and i["frozen_untouched"] and i["count"] == 2
