"""CPU: the boundary of the batch normalisation (omnifusion_amd.ops.batch_norm / BatchNorm2d / convert, csrc/omni_batchnorm.hip) — the module
imports without a GPU, the new symbols are declared, exported and bound, the workspace query, the C-level rejections that return before a
device is touched, the argument checks of the Python operators, and ops.convert on a CPU model."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omnifusion.h")
UNIT = os.path.join(ROOT, "omnifusion_amd", "csrc", "omni_batchnorm.hip")
NEW_SYMBOLS = ("omni_batchnorm_workspace_bytes", "omni_batchnorm_fwd_f32", "omni_batchnorm_bwd_f32")


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


def test_ops_imports_without_a_gpu():
    from omnifusion_amd import ops
    assert callable(ops.batch_norm) and callable(ops.convert) and issubclass(ops.BatchNorm2d, torch.nn.BatchNorm2d)
    layer = ops.BatchNorm2d(64, act="relu")
    assert layer.act == "relu"
    assert list(layer.state_dict()) == list(torch.nn.BatchNorm2d(64).state_dict())               # a drop-in for the torch layer
    assert [n for n, _ in layer.named_parameters()] == ["weight", "bias"]
    assert [n for n, _ in layer.named_buffers()] == ["running_mean", "running_var", "num_batches_tracked"]
    plain = ops.BatchNorm2d(16, affine=False, track_running_stats=False)
    assert plain.weight is None and plain.running_mean is None and list(plain.state_dict()) == []


def test_symbols_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(HEADER).read()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_batchnorm_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.omni_batchnorm_fwd_f32.argtypes) == 17 and len(L.omni_batchnorm_bwd_f32.argtypes) == 16


def test_no_getenv_no_atomic_and_no_guarded_kernel_name_in_the_unit():
    from omnifusion_amd import isa
    src = open(UNIT).read() + open(os.path.join(os.path.dirname(UNIT), "omni_partials.h")).read()       # (the finish order the unit includes)
    assert "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
    kernels = re.findall(r"void\s+(\w+_kernel)\s*\(", src)
    assert {"bn_stats_kernel", "bn_stats_finish_kernel", "bn_eval_saved_kernel", "bn_apply_kernel", "bn_bwd_reduce_kernel",
            "bn_bwd_finish_kernel", "bn_bwd_apply_kernel"} <= set(kernels)
    for k in kernels:
        assert not any(g in k for g in isa.COUNTED + isa.HOT), k


def test_workspace_query():
    from omnifusion_amd import _lib
    q = _lib.load().omni_batchnorm_workspace_bytes
    for bad in ((0, 32), (-5, 32), (64, 0), (64, -4), (64, 6), (64, 30), (64, 33), (1 << 31, 32), (1 << 40, 4)):
        assert q(*bad) == 0, bad
    for rows, C in ((1, 4), (2, 32), (18, 512), (105, 32), (10240, 32), (144 * 128 * 128, 32), (144 * 4 * 4, 512), (7, 96)):
        n = q(rows, C)
        assert n > 0 and n % 16 == 0, (rows, C)
        assert n >= 2 * C * 8 + 2 * C * 4                                       # one slab of partials in double, the rounded pair of sums
        assert n <= 1024 * 2 * C * 8 + 2 * C * 4 + 16                          # never more than 1024 slabs
    assert q(10240, 32) > q(512, 32)                                            # more than one slab at 10 240 rows of 32 channels


def test_c_boundary_rejects_before_touching_a_device():
    """Every rejection of the header, in both calls.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    big = 1 << 30
    fwd, bwd = L.omni_batchnorm_fwd_f32, L.omni_batchnorm_bwd_f32
    err = L.omni_last_error

    #   x res gamma beta rm rv y saved | rows C training momentum eps act | ws ws_bytes stream
    def f(x=p, res=p, gamma=p, beta=p, rm=p, rv=p, y=p, saved=p, rows=64, C=32, training=1, momentum=0.1, eps=1e-5, act=0, ws=p, nb=big):
        return fwd(x, res, gamma, beta, rm, rv, y, saved, rows, C, training, momentum, eps, act, ws, nb, z)

    assert f(x=z) == INV and b"null" in err()
    assert f(y=z) == INV and f(saved=z) == INV
    for C in (0, -4, 6, 30):
        assert f(C=C) == INV and b"multiple of 4" in err(), C
    assert f(rows=0) == INV and f(rows=-1) == INV
    assert f(rows=1) == INV and b"more than 1 value per channel" in err()
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert f(eps=eps) == INV and b"eps" in err(), eps
    for m in (-0.01, 1.01, float("nan")):
        assert f(momentum=m) == INV and b"momentum" in err(), m
    assert f(act=2) == UNS and b"GELU" in err()
    assert f(act=7) == INV and f(act=-1) == INV
    assert f(training=0, rm=z, rv=z) == INV and b"running" in err()
    assert f(rm=z) == INV and f(rv=z) == INV                                    # one running buffer without the other
    assert f(nb=16) == INV and b"workspace" in err()
    assert f(ws=z) == INV and b"workspace" in err()
    assert f(rows=1 << 31) == UNS and b"32-bit" in err()

    #   g x y gamma saved dx dres dgamma dbeta | rows C training act | ws ws_bytes stream
    def b(g=p, x=p, y=p, gamma=p, saved=p, dx=p, dres=z, dgamma=p, dbeta=p, rows=64, C=32, training=1, act=0, ws=p, nb=big):
        return bwd(g, x, y, gamma, saved, dx, dres, dgamma, dbeta, rows, C, training, act, ws, nb, z)

    assert b(g=z) == INV and b"null" in err()
    assert b(x=z) == INV and b(saved=z) == INV
    assert b(dx=z, dgamma=z, dbeta=z) == INV and b"no gradient requested" in err()
    for C in (0, -4, 6, 30):
        assert b(C=C) == INV and b"multiple of 4" in err(), C
    assert b(rows=0) == INV
    assert b(rows=1) == INV and b"more than 1 value per channel" in err()
    assert b(act=2) == UNS and b"GELU" in err()
    assert b(act=5) == INV
    assert b(act=1, y=z, dres=p) == INV and b"ReLU" in err()
    assert b(act=0, dres=p) == INV and b"g itself" in err()
    assert b(nb=16) == INV and b"workspace" in err()
    assert b(ws=z) == INV and b"workspace" in err()
    assert b(rows=1 << 31) == UNS and b"32-bit" in err()


def test_python_errors():
    from omnifusion_amd import ops
    x = torch.rand(2, 32, 4, 4)
    v = lambda n=32: dev(torch.rand(n))
    with pytest.raises(ValueError, match="x must be a tensor on an MI355X device; there is no CPU path"):
        ops.batch_norm(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.BatchNorm2d(32)(x)
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.batch_norm(x.numpy())
    X = dev(x)
    with pytest.raises(ValueError, match="weight must be a tensor on an MI355X device; there is no CPU path"):
        ops.batch_norm(X, torch.rand(32))
    with pytest.raises(ValueError, match="float32"):
        ops.batch_norm(dev(x.double()))
    with pytest.raises(ValueError, match="running_var must be float32"):
        ops.batch_norm(X, None, None, v(), dev(torch.rand(32).double()))
    with pytest.raises(ValueError, match=r"non-empty \[M,C,H,W\]"):
        ops.batch_norm(dev(torch.rand(2, 32, 4)))
    with pytest.raises(ValueError, match="non-empty"):
        ops.batch_norm(dev(torch.rand(0, 32, 4, 4)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.batch_norm(dev(torch.rand(2, 6, 4, 4)))
    for kw in ({"weight": v(16)}, {"bias": v(16)}, {"running_mean": v(16), "running_var": v()}, {"running_mean": v(), "running_var": v(64)}):
        with pytest.raises(ValueError, match=next(iter(kw)) if len(kw) == 1 else r"running_\w+ must be \[C\]"):
            ops.batch_norm(X, **kw)
    with pytest.raises(ValueError, match="come together"):
        ops.batch_norm(X, running_mean=v())
    with pytest.raises(ValueError, match="cannot require a gradient"):
        ops.batch_norm(X, running_mean=dev(torch.rand(32).requires_grad_(True)), running_var=v())
    with pytest.raises(ValueError, match="res must have x's shape"):
        ops.batch_norm(X, res=dev(torch.rand(2, 32, 4, 2)))
    with pytest.raises(ValueError, match="gelu.*'none' and 'relu' only"):
        ops.batch_norm(X, act="gelu")
    with pytest.raises(ValueError, match="'none' or 'relu'"):
        ops.batch_norm(X, act="tanh")
    with pytest.raises(ValueError, match="momentum=None"):
        ops.batch_norm(X, momentum=None)
    for m in (-0.1, 1.5, float("nan"), "0.1"):
        with pytest.raises(ValueError, match=r"momentum must be a number in \[0, 1\]"):
            ops.batch_norm(X, momentum=m)
    for eps in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="eps must be a positive finite number"):
            ops.batch_norm(X, eps=eps)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        ops.batch_norm(dev(torch.rand(1, 32, 1, 1)))
    with pytest.raises(ValueError, match="training=False needs running_mean"):
        ops.batch_norm(X, training=False)
    with pytest.raises(ValueError, match="momentum=None"):
        ops.BatchNorm2d(32, momentum=None)
    with pytest.raises(ValueError, match="act must be"):
        ops.BatchNorm2d(32, act="gelu")
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.BatchNorm2d(6)


def test_convert_swaps_what_is_in_scope_and_keeps_every_tensor():
    from omnifusion_amd import ops
    nn = torch.nn
    model = nn.Sequential(nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False),          # the stem: 3 channels
                          nn.Conv2d(64, 64, 3, padding=1, bias=False),
                          nn.BatchNorm2d(64),
                          nn.ReLU(),
                          nn.Conv2d(64, 64, 3, padding=1, groups=2),
                          nn.BatchNorm2d(64, momentum=None))
    model[2].eval()                                                                        # the mode travels with the layer
    tensors = {k: id(t) for k, t in list(model.named_parameters()) + list(model.named_buffers())}
    keys = list(model.state_dict())
    old = list(model)
    out, names = ops.convert(model)
    assert out is model and names == ["1", "2"]
    assert type(model[1]) is ops.Conv2d and type(model[2]) is ops.BatchNorm2d
    assert model[1].act == "none" and model[2].act == "none" and not model[2].training and model[1].training
    for i in (0, 3, 4, 5):
        assert model[i] is old[i]
    assert type(model[0]) is nn.Conv2d and type(model[4]) is nn.Conv2d and type(model[5]) is nn.BatchNorm2d
    assert {k: id(t) for k, t in list(model.named_parameters()) + list(model.named_buffers())} == tensors
    assert list(model.state_dict()) == keys
    assert model[1].weight is old[1].weight and model[2].running_var is old[2].running_var
    assert model[2].num_batches_tracked is old[2].num_batches_tracked
    assert ops.convert(model)[1] == []                                                     # nothing left to replace

    nested = nn.Sequential(nn.Sequential(nn.Conv2d(32, 32, 1), nn.BatchNorm2d(32)), nn.BatchNorm2d(6), nn.Conv2d(32, 32, 3, dilation=2),
                           nn.Conv2d(32, 48, 3), nn.Conv2d(32, 32, 5), nn.Conv2d(32, 32, 3, stride=3), nn.Conv2d(32, 32, (3, 1)))
    assert ops.convert(nested)[1] == ["0.0", "0.1"]
    root, names = ops.convert(nn.BatchNorm2d(16))                                          # a bare layer: the replacement is what is returned
    assert type(root) is ops.BatchNorm2d and names == [""]
