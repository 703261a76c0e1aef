"""CPU: the boundary of the differentiable convolution (omnifusion_amd.ops, csrc/omni_conv_bwd.hip) — the module imports without a GPU, the
new symbols are declared, exported and bound, the workspace query, the C-level rejections that return before a device is touched, and the
argument checks of ops.conv2d / ops.Conv2d."""
import ctypes
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnifusion.h")
NEW_SYMBOLS = ("omni_conv2d_bwd_workspace_bytes", "omni_conv2d_bwd_epilogue_f32", "omni_conv2d_bwd_data_f16x3",
               "omni_conv2d_bwd_weight_f16x3", "omni_conv2d_split_weights_f16x3")


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


def test_ops_imports_without_a_gpu():
    from omnifusion_amd import ops
    assert callable(ops.conv2d) and issubclass(ops.Conv2d, torch.nn.Conv2d)
    layer = ops.Conv2d(32, 64, 3, padding=1, act="relu")
    assert tuple(layer.weight.shape) == (64, 32, 3, 3) and layer.act == "relu"
    assert set(layer.state_dict()) == set(torch.nn.Conv2d(32, 64, 3, padding=1).state_dict())      # a drop-in for the torch layer


def test_symbols_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(HEADER).read()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_conv2d_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.omni_conv2d_bwd_data_f16x3.argtypes) == 18 and len(L.omni_conv2d_bwd_weight_f16x3.argtypes) == 18
    assert _lib.get_option("conv_wgrad_rows") == 0                              # 0: the library's plan


def test_no_getenv_and_no_guarded_kernel_name_in_the_unit():
    from omnifusion_amd import isa
    csrc = os.path.join(os.path.dirname(HEADER), "..", "omnifusion_amd", "csrc")
    src = open(os.path.join(csrc, "omni_conv_bwd.hip")).read() + open(os.path.join(csrc, "omni_partials.h")).read()    # (the finish order it includes)
    assert "getenv" not in src and "atomic" not in src.replace("no floating-point atomics", "").replace("no atomics", "")
    kernels = re.findall(r"void\s+(\w+_kernel)\s*\(", src)
    assert {"conv_dgrad_kernel", "conv_wgrad_kernel"} <= set(kernels)
    for k in kernels:
        assert not any(g in k for g in isa.COUNTED + isa.HOT), k


def test_workspace_query():
    from omnifusion_amd import _lib
    L = _lib.load()
    q = L.omni_conv2d_bwd_workspace_bytes
    #        M  H  W  C1  C2  Cout KH KW s  p
    for bad in ((2, 8, 8, 48, 0, 32, 3, 3, 1, 1), (2, 8, 8, 32, 16, 32, 3, 3, 1, 1), (2, 8, 8, 32, 0, 40, 3, 3, 1, 1), (2, 8, 8, 32, 0, 32, 2, 2, 1, 0),
                (2, 8, 8, 32, 0, 32, 3, 1, 1, 1), (2, 8, 8, 32, 0, 32, 3, 3, 3, 1), (0, 8, 8, 32, 0, 32, 3, 3, 1, 1), (2, 8, 8, 32, 0, 32, 3, 3, 1, -1),
                (2, 1, 1, 32, 0, 32, 3, 3, 1, 0)):
        assert q(*bad) == 0, bad
    shape = (40, 16, 16, 32, 0, 32, 3, 3, 1, 1)
    rows, Cout, K = 40 * 16 * 16, 32, 288
    n = q(*shape)
    assert n % 16 == 0 and n >= Cout * K * 4 and n >= ((rows + 63) // 64) * (Cout + 1) * 4       # the split weights of dgrad; the epilogue's partials
    try:
        _lib.set_option("conv_wgrad_rows", 32)                                  # the smallest chunk: one slab of partial sums per 32 rows
        assert q(*shape) == (rows // 32) * Cout * K * 4
        _lib.set_option("conv_wgrad_rows", 33)                                  # rounded up to a multiple of 32
        assert q(*shape) == (rows // 64) * Cout * K * 4
    finally:
        _lib.set_option("conv_wgrad_rows", 0)
    assert q(*shape) == n


def test_c_boundary_rejects_before_touching_a_device():
    """Null pointers, shapes outside the scope, GELU, short workspaces.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    big = 1 << 30
    assert L.omni_conv2d_bwd_epilogue_f32(p, p, p, p, p, 64, 32, 2, p, big, z) == UNS and b"GELU" in L.omni_last_error()
    assert L.omni_conv2d_bwd_epilogue_f32(p, p, p, p, p, 64, 32, 7, p, big, z) == INV
    assert L.omni_conv2d_bwd_epilogue_f32(z, p, p, p, p, 64, 32, 0, p, big, z) == INV
    assert L.omni_conv2d_bwd_epilogue_f32(p, z, p, p, p, 64, 32, 1, p, big, z) == INV and b"ReLU" in L.omni_last_error()
    assert L.omni_conv2d_bwd_epilogue_f32(p, p, p, p, p, 64, 48, 0, p, big, z) == INV
    assert L.omni_conv2d_bwd_epilogue_f32(p, p, p, p, p, 64, 32, 0, p, 16, z) == INV and b"workspace" in L.omni_last_error()
    good = (2, 8, 8, 32, 0, 32, 3, 3, 1, 1)
    for fn in (L.omni_conv2d_bwd_data_f16x3, L.omni_conv2d_bwd_weight_f16x3):
        assert fn(z, p, p, p, p, *good, p, big, z) == INV
        assert fn(p, p, p, p, p, *good, p, 16, z) == INV and b"workspace" in L.omni_last_error()
        assert fn(p, p, p, p, p, 2, 8, 8, 48, 0, 32, 3, 3, 1, 1, p, big, z) == INV and b"multiples of 32" in L.omni_last_error()
        assert fn(p, p, p, p, p, 2, 8, 8, 32, 0, 32, 2, 2, 1, 0, p, big, z) == UNS and b"1x1 or 3x3" in L.omni_last_error()
        assert fn(p, p, p, p, p, 2, 8, 8, 32, 0, 32, 3, 3, 4, 1, p, big, z) == UNS and b"stride" in L.omni_last_error()
    assert L.omni_conv2d_bwd_data_f16x3(p, p, p, z, z, *good, p, big, z) == INV and b"requested" in L.omni_last_error()
    assert L.omni_conv2d_bwd_data_f16x3(p, p, p, z, p, *good, p, big, z) == INV                   # dx2 without a second source
    assert L.omni_conv2d_bwd_weight_f16x3(p, p, z, p, p, 2, 8, 8, 32, 32, 32, 3, 3, 1, 1, p, big, z) == INV   # C2 > 0 without src2
    assert L.omni_conv2d_split_weights_f16x3(p, p, 32, 40, z) == INV and L.omni_conv2d_split_weights_f16x3(z, p, 32, 32, z) == INV


def test_python_errors():
    from omnifusion_amd import ops
    x, w = torch.rand(2, 32, 8, 8), torch.rand(32, 32, 3, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.conv2d(x, w, padding=1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.Conv2d(32, 32, 3, padding=1)(x)
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.conv2d(x.numpy(), w)
    with pytest.raises(ValueError, match="bias must be a tensor on an MI355X device; there is no CPU path"):
        ops.conv2d(dev(x), dev(w), torch.rand(32), padding=1)
    X, Wt = dev(x), dev(w)
    with pytest.raises(ValueError, match="float32"):
        ops.conv2d(dev(x.double()), Wt)
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv2d(dev(torch.rand(2, 48, 8, 8)), dev(torch.rand(32, 48, 3, 3)))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv2d(X, dev(torch.rand(40, 32, 3, 3)))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv2d(X, dev(torch.rand(32, 48, 3, 3)), x2=dev(torch.rand(2, 16, 8, 8)))
    for k in (2, 5):
        with pytest.raises(ValueError, match="1x1 or 3x3"):
            ops.conv2d(X, dev(torch.rand(32, 32, k, k)))
    with pytest.raises(ValueError, match="1x1 or 3x3"):
        ops.conv2d(X, dev(torch.rand(32, 32, 3, 1)))
    with pytest.raises(ValueError, match="gelu.*'none' and 'relu' only"):
        ops.conv2d(X, Wt, act="gelu")
    with pytest.raises(ValueError, match="'none' or 'relu'"):
        ops.conv2d(X, Wt, act="tanh")
    with pytest.raises(ValueError, match="stride must be 1 or 2"):
        ops.conv2d(X, Wt, stride=3)
    with pytest.raises(ValueError, match="input channels"):
        ops.conv2d(X, dev(torch.rand(32, 64, 3, 3)))
    with pytest.raises(ValueError, match="x2 must be"):
        ops.conv2d(X, dev(torch.rand(32, 64, 3, 3)), x2=dev(torch.rand(2, 32, 4, 4)))
    with pytest.raises(ValueError, match="res must have the result's shape"):
        ops.conv2d(X, Wt, padding=1, res=dev(torch.rand(2, 32, 6, 6)))
    with pytest.raises(ValueError, match="bias must be"):
        ops.conv2d(X, Wt, dev(torch.rand(16)), padding=1)
    with pytest.raises(ValueError, match="padding"):
        ops.conv2d(X, Wt, padding=-1)
    with pytest.raises(ValueError, match="no groups"):
        ops.Conv2d(32, 32, 3, groups=2)
    with pytest.raises(ValueError, match="act must be"):
        ops.Conv2d(32, 32, 3, act="gelu")
