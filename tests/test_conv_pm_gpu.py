"""GPU: the position-major form of the convolution tile kernel (conv_pm_sh_kernel, option conv_pm) for 3x3 / stride 1 / pad 1 convolutions of
8 x 8 and 4 x 4 images.  Its GEMM rows are ordered by pixel position, and a tile's K loop drops the taps that are zero padding for all of its rows.  The
dropped products are exact zeros and the remaining K-steps keep their order and their split-K ranges, so every output element — and every split-K
slab — must have the BITS of the image-major kernel (conv_pm = 0)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CHANNELS = ((32, 0, 128), (64, 32, 64), (64, 0, 256))        # one and two sources; 128- and 64-channel tiles
SHAPES = [(hw, mi, ch) for hw in (8, 4) for mi in (3, 18, 37) for ch in CHANNELS] + [(8, 144, (64, 32, 64)), (4, 144, (64, 0, 256))]
X1_SHAPES = {(8, 37, (64, 32, 64)), (4, 18, (64, 0, 256))}    # these also run the f16x1 forms (fmt bit 3)


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
    g = torch.Generator().manual_seed(1000 * H + 10 * M + C1 + C2 + Cout + k + stride)
    x1 = torch.randn(M, H, W, C1, generator=g)
    x2 = torch.randn(M, H, W, C2, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, k, k, generator=g) / np.sqrt((C1 + C2) * k * k)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(M, Ho, Wo, Cout, generator=g)
    d = lambda t: t.contiguous().to(DEV) if t is not None else None
    return dict(x1=x1, x2=x2, w=w, b=b, res=res, Ho=Ho, Wo=Wo, X1=_to_sh(lib, d(x1)), X2=_to_sh(lib, d(x2)), B=d(b), R=_to_sh(lib, d(res)),
                W16=split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV))


def _run(lib, c, dims, fmt, use_res, S):
    """One call of omni_conv2d_sh_f16x3_ws -> (output, split-K slabs or None); output and workspace start as NaN."""
    M, H, W, C1, C2, Cout, k, stride, pad = dims
    out = torch.full((M, c["Ho"], c["Wo"], Cout), float("nan"), device=DEV)
    ws = torch.full((max(S, 1) * out.numel(),), float("nan"), device=DEV)
    rc = lib.omni_conv2d_sh_f16x3_ws(_p(c["X1"]), _p(c["X2"]), _p(c["W16"]), _p(c["B"]), _p(c["R"]) if use_res else None, _p(out), fmt,
                                     M, H, W, C1, C2, Cout, k, k, stride, pad, 1 if use_res else 0, S, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream())
    assert rc == 0, lib.omni_last_error()
    return out, (ws.view(S, M, c["Ho"], c["Wo"], Cout) if S > 1 else None)


def _both(L, lib, c, dims, fmt, use_res, S):
    got = {}
    try:
        for pm in (2, 0):
            L.set_option("conv_pm", pm)
            got[pm] = _run(lib, c, dims, fmt, use_res, S)
    finally:
        L.set_option("conv_pm", 1)
    return got[2], got[0]


@pytest.mark.parametrize("hw,mi,ch", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_position_major_kernel_gives_the_bits_of_the_image_major_one(hw, mi, ch):
    """conv_pm = 2 against conv_pm = 0: with and without residual + ReLU, SH and fp32 output, splitk 1 / 2 / 3 (the second pass included, and the raw
    slabs), f16x1 for two of the shapes.  Row counts that are no multiple of 128, fewer rows than a tile, tiles across many positions, odd image counts;
    144 images (tiles of nearly one border class) once per map size."""
    L, lib = _lib()
    C1, C2, Cout = ch
    dims = (mi, hw, hw, C1, C2, Cout, 3, 1, 1)
    c = _case(*dims)
    G = (C1 + C2) // 32
    for x1 in ((0, 8) if (hw, mi, ch) in X1_SHAPES else (0,)):
        for use_res in (False, True):
            for dst_sh in (1, 0):
                for S in (1, 2, 3):
                    (o_pm, ws_pm), (o_im, ws_im) = _both(L, lib, c, dims, dst_sh | x1, use_res, S)
                    what = (x1, use_res, dst_sh, S)
                    assert dst_sh or not torch.isnan(o_pm).any(), what        # (every element was written)
                    assert torch.equal(_bits(o_pm), _bits(o_im)), what
                    if S > 1:
                        assert torch.equal(_bits(ws_pm), _bits(ws_im)), ("slabs", what)
                    if S == 3:
                        # per = 3 G: slab 0 holds the taps of the window's first row, which lie in the padding for every pixel of an image's first row
                        # (at 144 images the first tile is position (0, 0) alone: its block has no live K-step in that range and must WRITE the zeros)
                        assert (9 * G + 2) // 3 == 3 * G
                        assert (ws_pm[0][:, 0] == 0).all() and (ws_pm[2][:, hw - 1] == 0).all(), ("zero slab", what)
                        assert (ws_pm[1] != 0).any()


def test_position_major_kernel_against_float64():
    """Parent and child could be wrong together: one shape against F.conv2d in float64, within the bound test_conv2d_vs_torch uses (3e-5)."""
    L, lib = _lib()
    dims = (37, 8, 8, 64, 32, 64, 3, 1, 1)
    c = _case(*dims)
    xin = torch.cat([c["x1"], c["x2"]], -1)
    ref = F.conv2d(xin.permute(0, 3, 1, 2).double(), c["w"].double(), c["b"].double(), stride=1, padding=1).permute(0, 2, 3, 1)
    ref = F.relu(ref + c["res"].double())
    try:
        L.set_option("conv_pm", 2)
        for S in (1, 3):
            out, _ = _run(lib, c, dims, 0, True, S)
            err = (out.cpu().double() - ref).abs().max().item()
            print(f"splitk {S}: max |d| = {err:.3g}")
            assert err < 3e-5, (S, err)
    finally:
        L.set_option("conv_pm", 1)


@pytest.mark.parametrize("dims", [
    (18, 8, 8, 64, 0, 64, 3, 2, 1),        # stride 2
    (18, 8, 8, 64, 0, 64, 1, 1, 0),        # 1 x 1
    (5, 16, 16, 64, 0, 64, 3, 1, 1),       # W = 16
    (18, 4, 8, 64, 0, 64, 3, 1, 1),        # H != W
], ids=("stride2", "1x1", "w16", "h_ne_w"))
def test_launches_the_position_major_kernel_must_not_take(dims):
    L, lib = _lib()
    c = _case(*dims)
    ksteps = dims[6] * dims[6] * (dims[3] + dims[4]) // 32
    for S in (1, min(2, ksteps)):
        for fmt in (1, 0):
            (o_pm, _), (o_im, _) = _both(L, lib, c, dims, fmt, True, S)
            assert torch.equal(_bits(o_pm), _bits(o_im)), (S, fmt)
    if dims[6] == 3 and dims[7] == 1:       # (and the result is the operator's)
        ref = F.relu(F.conv2d(c["x1"].permute(0, 3, 1, 2).double(), c["w"].double(), c["b"].double(), stride=1, padding=1).permute(0, 2, 3, 1) + c["res"].double())
        assert (o_pm.cpu().double() - ref).abs().max().item() < 3e-5


@pytest.mark.parametrize("precision", ("f16x3", "f16x1"))
def test_model_output_does_not_depend_on_conv_pm(precision):
    """The single-pass model on 3 panoramas of 128 x 256 and on a lone panorama: conv_pm 1 (and 2: the new kernel wherever the shape allows) against 0."""
    L, lib = _lib()
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80), precision=precision).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    rgb = torch.rand((3, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    one = rgb[:1].contiguous()
    try:
        L.set_option("conv_pm", 0)
        ref, ref1 = net(rgb, confidence=True).clone(), net(one, confidence=True).clone()
        for pm in (1, 2):
            L.set_option("conv_pm", pm)
            assert torch.equal(net(rgb, confidence=True), ref), pm
            assert torch.equal(net(one, confidence=True), ref1), (pm, "one panorama")
    finally:
        L.set_option("conv_pm", 1)
