"""up2_taps_fused_kernel's separable tap sum (vertical sums per tap on the thread's own column, one horizontal stage per kx with the neighbour columns
exchanged through LDS; the specification is tests/test_up2_taps_sep_cpu.py), through omni_conv3x3_up2_taps_sh_f16x3: inputs that localise an exchange
error — single low-resolution pixels at the map's corners, at the wave borders (columns 7 / 8, 15 / 16), at the band border (rows 7 / 8) and inside;
one-hot weights per tap; channels that differ per channel quad — and one randn case per shape.  Every case: < 3e-5 against float64 `direct` and
against omni_conv3x3_up2_sh_f16x3 (the project's bound), every output written (NaN pre-fill), two launches equal in bits."""
import ctypes

import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, taps_repack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 64
# (M, Hl, Wl): one band with the top and the bottom edge in the same thread; two bands and no interior; whole images, M odd
SHAPES = [(1, 8, 32), (2, 16, 32), (3, 16, 16)]
IDS = ["band_m1_8x32", "bands_m2_16x32", "image_m3_16x16"]
BOUND = 3e-5


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from omnifusion_amd import _lib as L
    return L.load()


def _to_sh(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_from_f32(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


def _from_sh(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_to_f32(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


def _weights(w):
    from omnifusion_amd.model._engine import split_weights_f16x3
    return (split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(C, -1).contiguous()).to(DEV), split_weights_f16x3(taps_repack(w).contiguous()).to(DEV))


def _check(lib, x, W, w, b=None, act=0, tag=""):
    """one case: the new kernel twice (NaN pre-fill, same bits), the halo kernel, float64.  Returns (error of the new kernel, error of the halo kernel)
    against float64."""
    M, Hl, Wl, _ = x.shape
    W16, W16T = W
    XS = _to_sh(lib, x.to(DEV))
    xs = _from_sh(lib, XS).cpu()                                  # what the kernels see: x rounded to the SH format
    B = None if b is None else b.to(DEV)
    old = torch.empty((M, 2 * Hl, 2 * Wl, C), device=DEV)
    assert lib.omni_conv3x3_up2_sh_f16x3(_p(XS), _p(W16), _p(B), _p(old), 1, M, Hl, Wl, C, C, act, _stream()) == 0, lib.omni_last_error()
    outs = []
    for _ in range(2):
        o = torch.full((M, 2 * Hl, 2 * Wl, C), float("nan"), device=DEV)
        assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), _p(B), _p(o), 1, M, Hl, Wl, C, C, act, _stream()) == 0, lib.omni_last_error()
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{tag}: two launches differ"
    ref = direct(xs, w, b, relu=act == 1)
    got, was = _from_sh(lib, outs[0]).cpu().double(), _from_sh(lib, old).cpu().double()
    assert not torch.isnan(got).any(), f"{tag}: an output element was not written"
    d64, dold, dhalo = (got - ref).abs().max().item(), (got - was).abs().max().item(), (was - ref).abs().max().item()
    print(f"{tag}: vs float64 {d64:.3g} (the halo kernel: {dhalo:.3g}), vs the halo kernel {dold:.3g}; ref max {ref.abs().max().item():.3g}")
    assert d64 < BOUND, f"{tag}: {d64} against float64"
    assert dold < BOUND, f"{tag}: {dold} against the halo kernel"
    return d64, dhalo, got, ref


@pytest.fixture(scope="module")
def lib():
    return _lib()


@pytest.fixture(scope="module")
def dense():
    """one dense weight set for the single-pixel and randn cases (the inputs of test_up2_taps_fused_gpu.py: randn / sqrt(9 C), a bias)"""
    g = torch.Generator().manual_seed(11)
    w = torch.randn(C, C, 3, 3, generator=g) / np.sqrt(9 * C)
    b = torch.randn(C, generator=g)
    return w, b, _weights(w)


def _pixels(Hl, Wl):
    px = [(0, 0), (0, Wl - 1), (Hl - 1, 0), (Hl - 1, Wl - 1),                  # the four corners
          (3, 7), (3, 8), (4, 15), (4, 16),                                     # wave borders of the tap sum (8 columns per wave)
          (7, 5), (8, 5), (7, 8), (8, 7),                                       # band border (8 rows per band / per thread)
          (5, 11)]                                                              # interior
    return [(i, j) for i, j in px if i < Hl and j < Wl]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_single_pixels(lib, dense, shape):
    """one non-zero low-resolution pixel (in the last image; the others stay zero): a lost or misplaced neighbour column / row shows as an error of the
    size of the result, and outside the pixel's 6 x 6 footprint the result is exactly zero"""
    M, Hl, Wl = shape
    w, _, W = dense
    g = torch.Generator().manual_seed(100 + Hl + Wl)
    for i, j in _pixels(Hl, Wl):
        x = torch.zeros(M, Hl, Wl, C)
        x[M - 1, i, j] = torch.randn(C, generator=g)
        _, _, got, ref = _check(lib, x, W, w, tag=f"{shape} pixel ({i}, {j})")
        assert ref.abs().max().item() > 0.1                       # (the bound means something: results of order 1)
        assert torch.equal(got[ref == 0], ref[ref == 0]), f"pixel ({i}, {j}): something outside the footprint"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_hot_taps(lib, shape):
    """weights with a single live tap, for each of the nine: a tap in the wrong column group or with the wrong row pair shows alone"""
    M, Hl, Wl = shape
    g = torch.Generator().manual_seed(200 + Hl + Wl)
    x = torch.randn(M, Hl, Wl, C, generator=g)
    for t in range(9):
        w = torch.zeros(C, C, 3, 3)
        w[:, :, t // 3, t % 3] = torch.randn(C, C, generator=g) / np.sqrt(C)
        _check(lib, x, _weights(w), w, tag=f"{shape} tap {t}")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_channel_quads(lib, shape):
    """diagonal weights whose scale differs per channel quad (and per channel within it): output channel c sees input channel c alone, so a thread
    that reads a neighbour's sums at another quad's place is off by the ratio of the scales"""
    M, Hl, Wl = shape
    g = torch.Generator().manual_seed(300 + Hl + Wl)
    x = torch.randn(M, Hl, Wl, C, generator=g)
    k = torch.randn(3, 3, generator=g) / 3.0
    w = torch.zeros(C, C, 3, 3)
    for c in range(C):
        w[c, c] = k * (1.0 + 0.5 * (c // 4) + 0.0625 * (c % 4)) / 4.0
    _check(lib, x, _weights(w), w, tag=f"{shape} quads")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_randn(lib, dense, shape):
    """randn inputs, bias, with ReLU and without; prints the largest error against float64, which must not be above the halo kernel's on the same inputs"""
    M, Hl, Wl = shape
    w, b, W = dense
    x = torch.randn(M, Hl, Wl, C, generator=torch.Generator().manual_seed(11 + Hl))
    for act in (1, 0):
        d64, dhalo, _, _ = _check(lib, x, W, w, b, act, tag=f"{shape} randn act {act}")
        assert d64 <= dhalo, (d64, dhalo)


@pytest.mark.parametrize("hw", [(8, 32), (16, 32), (16, 16)], ids=["8x32", "16x32", "16x16"])
def test_image_2_of_3_alone(lib, dense, hw):
    """the third image of a batch of three and the same image alone: the same bits"""
    Hl, Wl = hw
    _, b, (_, W16T) = dense
    B = b.to(DEV)
    XS = _to_sh(lib, torch.randn(3, Hl, Wl, C, generator=torch.Generator().manual_seed(5)).to(DEV))
    o3 = torch.full((3, 2 * Hl, 2 * Wl, C), float("nan"), device=DEV)
    o1 = torch.full((1, 2 * Hl, 2 * Wl, C), float("nan"), device=DEV)
    assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), _p(B), _p(o3), 1, 3, Hl, Wl, C, C, 1, _stream()) == 0
    last = XS[2:].contiguous()
    assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(last), _p(W16T), _p(B), _p(o1), 1, 1, Hl, Wl, C, C, 1, _stream()) == 0
    assert torch.equal(o3[2:].view(torch.int32), o1.view(torch.int32))
