"""GPU: halo2_sh_kernel (omni_conv_halo2.hip, option conv_halo2) — the 64-channel 3x3 halo convolution on 256-pixel tiles with 64 x 64 wave tiles.  Every
accumulator takes the parent's products in the parent's order and the epilogues are the shared helpers', so every output element must have the BITS of the
parent kernels (conv_halo2 = 0), whatever the launch; launches of other shapes must not reach it."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (M, H, W, C1, C2, Cout): the forms IW = 0 (8 x 32 tiles) and IW = 16 (whole images)
SHAPES = [
    (1, 8, 32, 64, 0, 64),         # a single tile, every border at once
    (3, 8, 32, 64, 0, 64),
    (2, 16, 64, 32, 32, 128),      # interior tile edges in both directions, two sources, two channel tiles
    (1, 32, 32, 64, 64, 64),       # the de_conv2_1 form
    (2, 16, 16, 128, 0, 128),      # whole-image tiles
    (5, 16, 16, 128, 0, 128),
    (2, 16, 16, 64, 64, 64),
    (5, 16, 16, 64, 64, 64),
]
POST_SHAPE = (3, 8, 32, 64, 0, 64)
X1_SHAPES = {(2, 16, 64, 32, 32, 128), (5, 16, 16, 64, 64, 64)}


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32)


def _to_sh(lib, t):
    if t is None:
        return None
    o = torch.empty_like(t)
    assert lib.omni_sh_from_f32(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


@functools.lru_cache(maxsize=None)
def _case(M, H, W, C1, C2, Cout, k, stride, pad):
    """Inputs of one convolution (randn, weights / sqrt(K)), made once and shared; nothing below writes to them."""
    from omnifusion_amd.model._engine import split_weights_f16x3
    _, lib = _lib()
    g = torch.Generator().manual_seed(1000 * H + 100 * W + 10 * M + C1 + C2 + Cout + k + stride)
    x1 = torch.randn(M, H, W, C1, generator=g)
    x2 = torch.randn(M, H, W, C2, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, k, k, generator=g) / np.sqrt((C1 + C2) * k * k)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(M, Ho, Wo, Cout, generator=g)
    post = torch.randn(Ho, Wo, Cout, generator=g)               # one image's size: broadcast over the batch
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    return dict(x1=x1, x2=x2, w=w, b=b, res=res, post=post, Ho=Ho, Wo=Wo, X1=_to_sh(lib, d(x1)), X2=_to_sh(lib, d(x2)), B=d(b), R=_to_sh(lib, d(res)), P=d(post),
                W16=split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV))


def _run(lib, c, dims, fmt, use_res, S=1, post=False):
    """One call of omni_conv2d_sh_f16x3_ws (or _post_ws) -> output; output and workspace start as NaN."""
    M, H, W, C1, C2, Cout, k, stride, pad = dims
    out = torch.full((M, c["Ho"], c["Wo"], Cout), float("nan"), device=DEV)
    ws = torch.full((max(S, 1) * out.numel(),), float("nan"), device=DEV)
    args = (_p(c["X1"]), _p(c["X2"]), _p(c["W16"]), _p(c["B"]), _p(c["R"]) if use_res else None, _p(out), fmt,
            M, H, W, C1, C2, Cout, k, k, stride, pad, 1 if use_res else 0, S, _p(ws), ctypes.c_size_t(ws.numel() * 4))
    if post:
        rc = lib.omni_conv2d_sh_f16x3_post_ws(*args, _p(c["P"]), ctypes.c_size_t(c["P"].numel()), _stream())
    else:
        rc = lib.omni_conv2d_sh_f16x3_ws(*args, _stream())
    assert rc == 0, lib.omni_last_error()
    return out


def _both(L, lib, c, dims, fmt, use_res, S=1, post=False):
    shipped = L.get_option("conv_halo2")
    got = {}
    try:
        for h2 in (2, 0):
            L.set_option("conv_halo2", h2)
            got[h2] = _run(lib, c, dims, fmt, use_res, S, post)
    finally:
        L.set_option("conv_halo2", shipped)
    return got[2], got[0]


def _ids(v):
    return "x".join(map(str, v))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_halo2_kernel_gives_the_bits_of_the_parent(shape):
    """conv_halo2 = 2 against 0: with and without residual + ReLU, SH and fp32 output; f16x1 (fmt bit 3) for two of the shapes, the post-activation addend
    (omni_conv2d_sh_f16x3_post_ws, one image's size) for one."""
    L, lib = _lib()
    dims = shape + (3, 1, 1)
    c = _case(*dims)
    for x1 in ((0, 8) if shape in X1_SHAPES else (0,)):
        for use_res in (False, True):
            for dst_sh in (1, 0):
                for post in ((False, True) if shape == POST_SHAPE else (False,)):
                    new, old = _both(L, lib, c, dims, dst_sh | x1, use_res, post=post)
                    what = (x1, use_res, dst_sh, post)
                    assert dst_sh or not torch.isnan(new).any(), what         # (every element was written)
                    assert torch.equal(_bits(new), _bits(old)), what


@pytest.mark.parametrize("shape", [(2, 16, 64, 32, 32, 128), (5, 16, 16, 64, 64, 64)], ids=_ids)
def test_halo2_kernel_against_float64(shape):
    """Parent and child could be wrong together: against F.conv2d in float64 with bias, residual and ReLU, within the bound test_conv2d_vs_torch uses (3e-5)."""
    L, lib = _lib()
    dims = shape + (3, 1, 1)
    c = _case(*dims)
    xin = torch.cat([c["x1"], c["x2"]], -1)
    ref = F.conv2d(xin.permute(0, 3, 1, 2).double(), c["w"].double(), c["b"].double(), stride=1, padding=1).permute(0, 2, 3, 1)
    ref = F.relu(ref + c["res"].double())
    shipped = L.get_option("conv_halo2")
    try:
        L.set_option("conv_halo2", 2)
        out = _run(lib, c, dims, 0, True)
        err = (out.cpu().double() - ref).abs().max().item()
        print(f"{shape}: max |d| = {err:.3g}")
        assert err < 3e-5, err
    finally:
        L.set_option("conv_halo2", shipped)


@pytest.mark.parametrize("dims,S,fmt4", [
    ((2, 12, 32, 64, 0, 64, 3, 1, 1), 1, 0),        # H a multiple of 4, not of 8
    ((2, 8, 48, 64, 0, 64, 3, 1, 1), 1, 0),         # W = 48
    ((2, 16, 64, 64, 0, 64, 3, 2, 1), 1, 0),        # stride 2
    ((2, 8, 32, 64, 0, 64, 1, 1, 0), 1, 0),         # 1 x 1
    ((2, 8, 32, 64, 0, 64, 3, 1, 1), 2, 0),         # split-K
    ((2, 8, 32, 64, 0, 32, 3, 1, 1), 1, 0),         # Cout = 32
    ((4, 8, 8, 64, 0, 64, 3, 1, 1), 1, 0),          # 8 x 8 images
    ((2, 8, 32, 64, 0, 64, 3, 1, 1), 1, 4),         # fmt bit 2: the latency form
], ids=("h12", "w48", "stride2", "1x1", "splitk2", "cout32", "img8", "fmt4"))
def test_launches_the_halo2_kernel_must_not_take(dims, S, fmt4):
    L, lib = _lib()
    c = _case(*dims)
    for fmt in (1, 0):
        new, old = _both(L, lib, c, dims, fmt | fmt4, True, S)
        assert torch.equal(_bits(new), _bits(old)), fmt
    if dims[6] == 3 and dims[7] == 1:       # (and the result is the operator's)
        ref = F.relu(F.conv2d(c["x1"].permute(0, 3, 1, 2).double(), c["w"].double(), c["b"].double(), stride=1, padding=1).permute(0, 2, 3, 1) + c["res"].double())
        assert (new.cpu().double() - ref).abs().max().item() < 3e-5


@pytest.mark.parametrize("precision", ("f16x3", "f16x1"))
def test_model_output_does_not_depend_on_conv_halo2(precision):
    """The single-pass model on 3 panoramas of 128 x 256 and on a lone panorama: conv_halo2 1 and 2 against 0."""
    L, lib = _lib()
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80), precision=precision).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    rgb = torch.rand((3, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    one = rgb[:1].contiguous()
    shipped = L.get_option("conv_halo2")
    try:
        L.set_option("conv_halo2", 0)
        ref, ref1 = net(rgb, confidence=True).clone(), net(one, confidence=True).clone()
        for h2 in (1, 2):
            L.set_option("conv_halo2", h2)
            assert torch.equal(net(rgb, confidence=True), ref), h2
            assert torch.equal(net(one, confidence=True), ref1), (h2, "one panorama")
    finally:
        L.set_option("conv_halo2", shipped)
