"""CPU: the boundary of the stem convolution, the max-pool and the 2x bilinear up-sampling in training mode (omnifusion_amd.ops,
csrc/omni_stem_conv.hip, omni_maxpool_bwd.hip, omni_upsample_bwd.hip) — the module imports without a GPU, the new symbols
are declared, exported and bound, the workspace query follows the documented chunking, the C-level rejections return before a device is
touched, the argument checks of the Python operators fire, and ops.convert swaps what it says it swaps."""
import ctypes
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnifusion.h")
NEW_SYMBOLS = ("omni_stem_conv_fwd_f32", "omni_stem_conv_bwd_workspace_bytes", "omni_stem_conv_bwd_weight_f32",
               "omni_maxpool3x3s2_bwd_f32", "omni_upsample_bilinear2x_bwd_f32")
UNITS = ("omni_stem_conv.hip", "omni_maxpool_bwd.hip", "omni_upsample_bwd.hip")


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


def small_model():
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
                         nn.Conv2d(64, 64, 3, padding=1))


def test_ops_imports_without_a_gpu():
    from omnifusion_amd import ops
    assert callable(ops.stem_conv2d) and callable(ops.max_pool2d) and callable(ops.upsample_bilinear2x)
    assert issubclass(ops.StemConv2d, torch.nn.Conv2d) and issubclass(ops.MaxPool2d, torch.nn.MaxPool2d)
    stem = ops.StemConv2d(3, 64, 7, stride=2, padding=3, bias=False)
    assert tuple(stem.weight.shape) == (64, 3, 7, 7) and stem.bias is None
    assert set(stem.state_dict()) == set(torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).state_dict())
    assert set(ops.StemConv2d(3, 64, 7, stride=2, padding=3, bias=True).state_dict()) == {"weight", "bias"}
    ops.MaxPool2d(3, 2, 1), ops.UpsampleBilinear2x()


def test_symbols_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(HEADER).read()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_stem_conv_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.omni_stem_conv_fwd_f32.argtypes) == 8 and len(L.omni_stem_conv_bwd_weight_f32.argtypes) == 10
    assert len(L.omni_maxpool3x3s2_bwd_f32.argtypes) == 8 and len(L.omni_upsample_bilinear2x_bwd_f32.argtypes) == 7


def test_units_have_no_atomics_no_getenv_and_no_guarded_kernel_name():
    from omnifusion_amd import isa
    csrc = os.path.join(os.path.dirname(HEADER), "..", "omnifusion_amd", "csrc")
    for unit in UNITS + ("omni_partials.h",):                                      # (the finish order the stem's unit includes)
        src = open(os.path.join(csrc, unit)).read()
        code = re.sub(r"//[^\n]*", "", src)                                    # (the comments say "no atomics")
        assert "getenv" not in code and "atomic" not in code.lower(), unit
        kernels = re.findall(r"void\s+(\w+_kernel)\s*\(", code)
        assert kernels or unit.endswith(".h"), unit
        for k in kernels:
            assert not any(g in k for g in isa.COUNTED + isa.HOT), k


def test_workspace_query():
    """nchunk . 148 . 64 . 4 bytes with ntiles = M . ceil(Ho/8) . ceil(Wo/8), tpc = max(4, ceil(ntiles / 1024)), nchunk = ceil(ntiles / tpc)."""
    from omnifusion_amd import _lib
    q = _lib.load().omni_stem_conv_bwd_workspace_bytes
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, -3, 8)):
        assert q(*bad) == 0, bad

    def want(M, H, W):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        ntiles = M * ((Ho + 7) // 8) * ((Wo + 7) // 8)
        tpc = max(4, (ntiles + 1023) // 1024)
        return ((ntiles + tpc - 1) // tpc) * 148 * 64 * 4

    for shape in ((2, 1, 1), (2, 16, 16), (3, 7, 9), (1, 6, 70), (40, 32, 32), (144, 64, 64), (144, 128, 128), (1000, 64, 64), (4096, 64, 64)):
        n = q(*shape)
        assert n > 0 and n % 16 == 0 and n == want(*shape), shape
    assert q(2, 1, 1) == 148 * 64 * 4                                           # one chunk
    assert q(40, 32, 32) == 40 * 148 * 64 * 4                                   # 160 tiles in chunks of 4
    assert q(144, 64, 64) == 576 * 148 * 64 * 4                                 # the benched shape: 2304 tiles in chunks of 4
    assert q(4096, 64, 64) <= 1024 * 148 * 64 * 4 < q(4096, 64, 64) * 2         # past 4096 tiles the chunks grow, not their number


def test_c_boundary_rejects_before_touching_a_device():
    """Null pointers, M, H, W <= 0, C % 4, short workspaces.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV = _lib.OMNI_ERR_INVALID
    big = 1 << 30
    fwd, wq, bww = L.omni_stem_conv_fwd_f32, L.omni_stem_conv_bwd_workspace_bytes, L.omni_stem_conv_bwd_weight_f32
    for args in ((z, p, p, p), (p, z, p, p), (p, p, p, z)):
        assert fwd(*args, 2, 8, 8, z) == INV and b"null" in L.omni_last_error(), args
    for shape in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
        assert fwd(p, p, p, p, *shape, z) == INV and b">= 1" in L.omni_last_error(), shape
        assert bww(p, p, p, p, *shape, p, big, z) == INV and b">= 1" in L.omni_last_error(), shape
    assert bww(z, p, p, p, 2, 8, 8, p, big, z) == INV and bww(p, z, p, p, 2, 8, 8, p, big, z) == INV
    assert bww(p, p, z, z, 2, 8, 8, p, big, z) == INV and b"requested" in L.omni_last_error()
    assert bww(p, p, p, p, 2, 8, 8, z, big, z) == INV and b"workspace" in L.omni_last_error()
    assert bww(p, p, p, p, 2, 8, 8, p, wq(2, 8, 8) - 1, z) == INV and b"workspace" in L.omni_last_error()
    assert bww(p, p, p, p, 40, 32, 32, p, wq(2, 8, 8), z) == INV and b"workspace" in L.omni_last_error()
    pool, up = L.omni_maxpool3x3s2_bwd_f32, L.omni_upsample_bilinear2x_bwd_f32
    for args in ((z, p, p), (p, z, p), (p, p, z)):
        assert pool(*args, 2, 8, 8, 8, z) == INV and b"null" in L.omni_last_error(), args
    for args in ((z, p), (p, z)):
        assert up(*args, 2, 8, 8, 8, z) == INV and b"null" in L.omni_last_error(), args
    for fn, ptrs in ((pool, (p, p, p)), (up, (p, p))):
        for shape in ((0, 8, 8, 8), (2, 0, 8, 8), (2, 8, -2, 8)):
            assert fn(*ptrs, *shape, z) == INV and b">= 1" in L.omni_last_error(), shape
        for C in (0, 2, 6, 33, -4):
            assert fn(*ptrs, 2, 8, 8, C, z) == INV and b"multiple of 4" in L.omni_last_error(), C


def test_python_errors():
    from omnifusion_amd import ops
    x, w = torch.rand(2, 3, 8, 8), torch.rand(64, 3, 7, 7)
    a = torch.rand(2, 8, 4, 4)
    for call in (lambda: ops.stem_conv2d(x, w), lambda: ops.StemConv2d()(x), lambda: ops.max_pool2d(a), lambda: ops.MaxPool2d()(a),
                 lambda: ops.upsample_bilinear2x(a), lambda: ops.UpsampleBilinear2x()(a)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.stem_conv2d(x.numpy(), w)
    with pytest.raises(ValueError, match="bias must be a tensor on an MI355X device; there is no CPU path"):
        ops.stem_conv2d(dev(x), dev(w), torch.rand(64))
    X, Wt = dev(x), dev(w)
    for call in (lambda: ops.stem_conv2d(dev(x.double()), Wt), lambda: ops.stem_conv2d(X, dev(w.half())),
                 lambda: ops.max_pool2d(dev(a.double())), lambda: ops.upsample_bilinear2x(dev(a.half()))):
        with pytest.raises(ValueError, match="float32"):
            call()
    for bad in (torch.rand(64, 3, 3, 3), torch.rand(32, 3, 7, 7), torch.rand(64, 4, 7, 7), torch.rand(64, 3, 7, 5), torch.rand(64, 147)):
        with pytest.raises(ValueError, match=r"weight must be \[64,3,7,7\].*7x7 convolution at stride 2 with padding 3"):
            ops.stem_conv2d(X, dev(bad))
    with pytest.raises(ValueError, match=r"\[M,3,H,W\]"):
        ops.stem_conv2d(dev(torch.rand(2, 4, 8, 8)), Wt)
    with pytest.raises(ValueError, match=r"\[M,3,H,W\]"):
        ops.stem_conv2d(dev(torch.rand(3, 8, 8)), Wt)
    with pytest.raises(ValueError, match=r"bias must be \[64\]"):
        ops.stem_conv2d(X, Wt, dev(torch.rand(32)))
    with pytest.raises(ValueError, match="image gradient of the stem is not built"):
        ops.stem_conv2d(dev(x.clone().requires_grad_()), Wt)
    for fn in (ops.max_pool2d, ops.upsample_bilinear2x):
        with pytest.raises(ValueError, match="multiple of 4"):
            fn(dev(torch.rand(2, 6, 4, 4)))
        with pytest.raises(ValueError, match=r"\[M,C,H,W\]"):
            fn(dev(torch.rand(8, 4, 4)))
        with pytest.raises(ValueError, match=r"\[M,C,H,W\]"):
            fn(dev(torch.rand(0, 8, 4, 4)))
    for bad in (dict(out_channels=32), dict(kernel_size=3), dict(stride=1), dict(padding=2), dict(groups=3, in_channels=3, out_channels=63),
                dict(dilation=2), dict(padding_mode="reflect")):
        with pytest.raises(ValueError, match="7x7 convolution at stride 2 with padding 3"):
            ops.StemConv2d(**bad)
    for bad in (dict(kernel_size=2), dict(stride=1), dict(padding=0), dict(dilation=2), dict(ceil_mode=True), dict(return_indices=True)):
        with pytest.raises(ValueError, match="3x3 max-pool at stride 2 with padding 1"):
            ops.MaxPool2d(**bad)


def test_convert_default_is_unchanged():
    from omnifusion_amd import ops
    m = small_model()
    keys = list(m.state_dict())
    m2, names = ops.convert(m)
    assert m2 is m and names == ["1", "4"]
    assert type(m[0]) is torch.nn.Conv2d and type(m[3]) is torch.nn.MaxPool2d and type(m[2]) is torch.nn.ReLU
    assert type(m[1]) is ops.BatchNorm2d and type(m[4]) is ops.Conv2d
    assert list(m.state_dict()) == keys
    assert ops.convert(small_model(), spatial=False)[1] == ["1", "4"]


def test_convert_spatial_swaps_the_stem_and_the_pool():
    from omnifusion_amd import ops
    m = small_model()
    keys = list(m.state_dict())
    params = {k: v for k, v in m.named_parameters()}
    buffers = {k: v for k, v in m.named_buffers()}
    m2, names = ops.convert(m, spatial=True)
    assert m2 is m and names == ["0", "1", "3", "4"]
    assert type(m[0]) is ops.StemConv2d and type(m[1]) is ops.BatchNorm2d and type(m[2]) is torch.nn.ReLU
    assert type(m[3]) is ops.MaxPool2d and type(m[4]) is ops.Conv2d
    assert list(m.state_dict()) == keys
    assert all(v is params[k] for k, v in m.named_parameters()) and set(params) == {k for k, _ in m.named_parameters()}
    assert all(v is buffers[k] for k, v in m.named_buffers())
    assert not hasattr(m[0], "act") and not hasattr(m[3], "act") and m[4].act == "none"
    with_bias = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True))
    b = with_bias[0].bias
    ops.convert(with_bias, spatial=True)
    assert type(with_bias[0]) is ops.StemConv2d and with_bias[0].bias is b
    root, names = ops.convert(torch.nn.MaxPool2d(3, 2, 1), spatial=True)        # a lone layer comes back swapped
    assert type(root) is ops.MaxPool2d and names == [""]


def test_convert_spatial_leaves_other_geometries_alone():
    from omnifusion_amd import ops
    nn = torch.nn
    others = [nn.MaxPool2d(2, 2), nn.Conv2d(3, 32, 7, 2, 3), nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, return_indices=True),
              nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(3, 2, 0), nn.Conv2d(3, 64, 7, 2, 3, padding_mode="reflect"),
              nn.Conv2d(3, 64, 7, 2, 3, dilation=2), nn.Conv2d(3, 64, 7, 1, 3), nn.Conv2d(3, 64, 5, 2, 2), nn.AvgPool2d(3, 2, 1)]
    m = nn.Sequential(*others)
    kinds = [type(c) for c in m]
    _, names = ops.convert(m, spatial=True)
    assert names == [] and [type(c) for c in m] == kinds
