"""GPU: up2_taps_walk_kernel (csrc/omni_conv_up2_taps.hip) — the 64 -> 64 tap-product stages on eight waves and persistent blocks — behind option
`conv_up2_taps_walk` of omni_conv3x3_up2_taps_sh_f16x3.  The parent kernel (option 0, up2_taps_fused_kernel) is the reference for the BITS: every output
element receives the same operations in the same order, whatever the grid (`conv_up2_taps_walk_grid`), so the SH words are compared as 32-bit integers.
Option 2 is the new kernel for both forms wherever the shape allows; option 1 the forms that ship (it may serve a form with the parent kernel: the
comparison then holds trivially, which is why every bit test runs under 2 as well).
Inputs of tests/test_up2_taps_fused_gpu.py: randn, weights / sqrt(9 * 64), a bias; result buffers start as NaN."""
import ctypes

import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, taps_repack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT, GRID = "conv_up2_taps_walk", "conv_up2_taps_walk_grid"


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sh(lib, t, fn):
    o = torch.empty_like(t)
    assert getattr(lib, fn)(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


class _Opt:
    """the two options for the length of a block, restored afterwards"""
    def __init__(self, walk, grid=0):
        self.v = (walk, grid)

    def __enter__(self):
        L, _ = _lib()
        self.saved = (L.get_option(OPT), L.get_option(GRID))
        L.set_option(OPT, self.v[0]); L.set_option(GRID, self.v[1])

    def __exit__(self, *exc):
        L, _ = _lib()
        L.set_option(OPT, self.saved[0]); L.set_option(GRID, self.saved[1])


@pytest.fixture(scope="module")
def weights():
    from omnifusion_amd.model._engine import split_weights_f16x3
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 64, 3, 3, generator=g) / np.sqrt(9 * 64)
    b = torch.randn(64, generator=g)
    return w, b, split_weights_f16x3(taps_repack(w).contiguous()).to(DEV), b.to(DEV)


def _input(lib, M, Hl, Wl, seed):
    x = torch.randn(M, Hl, Wl, 64, generator=torch.Generator().manual_seed(seed))
    return _sh(lib, x.to(DEV), "omni_sh_from_f32")


def _run(lib, XS, W16T, B, act, walk, grid=0):
    M, Hl, Wl, _ = XS.shape
    o = torch.full((M, 2 * Hl, 2 * Wl, 64), float("nan"), device=DEV)
    with _Opt(walk, grid):
        assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), _p(B), _p(o), 1, M, Hl, Wl, 64, 64, act, _stream()) == 0, lib.omni_last_error()
    torch.cuda.synchronize()
    return o


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# band form: one band that is top and bottom; first + last; first, interior, last with an odd image count (18 units).  Whole images: M = 1, 3
@pytest.mark.parametrize("cfg", [(1, 8, 32), (2, 16, 32), (3, 24, 32), (1, 16, 16), (3, 16, 16)],
                         ids=["bands_m1_h8", "bands_m2_h16", "bands_m3_h24", "image_m1", "image_m3"])
def test_bits_of_the_parent(weights, cfg):
    """option 0 against option 1 and 2, default grid and 8 / 16 blocks (grid 8 at (3, 24): 4 units per XCD range at most, one block per range walks them
    all and changes the channel half; ranges without units: blocks that leave at once), with ReLU and without"""
    L, lib = _lib()
    w, b, W16T, B = weights
    XS = _input(lib, *cfg, seed=21)
    for act in (1, 0):
        ref = _run(lib, XS, W16T, B, act, 0)
        assert not torch.isnan(ref).any()
        for walk in (1, 2):
            for grid in (0, 8, 16):
                assert _same(_run(lib, XS, W16T, B, act, walk, grid), ref), (cfg, act, walk, grid)


def test_walk_on_the_real_grid(weights):
    """(16, 96): 384 units on one block per CU — with 256 blocks half the blocks of every XCD walk two — against the parent; and (2, 24) on 8 blocks,
    twice: the same bits"""
    L, lib = _lib()
    w, b, W16T, B = weights
    XS = _input(lib, 16, 96, 32, seed=22)
    ref = _run(lib, XS, W16T, B, 1, 0)
    for walk in (1, 2):
        assert _same(_run(lib, XS, W16T, B, 1, walk), ref), walk
    del ref
    XS = _input(lib, 2, 24, 32, seed=23)
    for walk in (1, 2):
        a, c = _run(lib, XS, W16T, B, 1, walk, 8), _run(lib, XS, W16T, B, 1, walk, 8)
        assert not torch.isnan(a).any() and _same(a, c)


@pytest.mark.parametrize("cfg", [(2, 24, 32), (3, 16, 16)], ids=["bands", "image"])
def test_against_float64(weights, cfg):
    """against `direct`, the bound tests/test_up2_taps_fused_gpu.py uses for this stage and these inputs (< 3e-5)"""
    L, lib = _lib()
    w, b, W16T, B = weights
    XS = _input(lib, *cfg, seed=24)
    xs = _sh(lib, XS, "omni_sh_to_f32").cpu()
    for act in (1, 0):
        ref = direct(xs, w, b, relu=act == 1)
        for walk in (1, 2):
            got = _sh(lib, _run(lib, XS, W16T, B, act, walk), "omni_sh_to_f32").cpu().double()
            assert not torch.isnan(got).any()
            d = (got - ref).abs().max().item()
            print(f"walk {walk} {cfg} act {act}: vs float64 {d:.3g}; ref max {ref.abs().max().item():.3g}")
            assert d < 3e-5


def test_image_bits_do_not_depend_on_the_batch(weights):
    """an image inside a batch of 3 and alone: the same bits (both forms)"""
    L, lib = _lib()
    w, b, W16T, B = weights
    for Hl, Wl in ((16, 16), (16, 32)):
        XS = _input(lib, 3, Hl, Wl, seed=25)
        for walk in (1, 2):
            o3 = _run(lib, XS, W16T, B, 1, walk)
            o1 = _run(lib, XS[2:].contiguous(), W16T, B, 1, walk)
            assert _same(o3[2:], o1)


@pytest.mark.parametrize("shape", [(16, 16), (8, 32)], ids=["image", "bands"])
def test_range_guard(shape):
    """outputs beyond the fp16 range saturate, raise the sticky flag (omni_sh_overflow reports and clears it) and never turn into NaN"""
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    Hl, Wl = shape
    flag = ctypes.c_int(0)
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0                       # clear
    g = torch.Generator().manual_seed(2)
    w = torch.randn(64, 64, 3, 3, generator=g)
    W16T = split_weights_f16x3(taps_repack(w).contiguous()).to(DEV)
    x = torch.randn(1, Hl, Wl, 64, generator=g).to(DEV)
    for walk in (1, 2):
        v = _sh(lib, _run(lib, _sh(lib, x * 1e4, "omni_sh_from_f32"), W16T, None, 0, walk), "omni_sh_to_f32").cpu()   # sums of 576 products of magnitude 1e4
        assert not torch.isnan(v).any() and v.max().item() == 65504.0 and v.min().item() == -65504.0
        assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 1   # raised, then cleared by the reset
        assert lib.omni_sh_overflow(ctypes.byref(flag), 0) == 0 and flag.value == 0
        _run(lib, _sh(lib, x, "omni_sh_from_f32"), W16T, None, 0, walk)
        assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 0   # in range: stays down


def test_models():
    """the single-pass model on 2 panoramas of 128 x 256: option 0, 1 and 2 give the same bits; pipelined(3) and graphed() under 1 and 2 give the bits of
    plain calls"""
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    rgb = torch.rand((2, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    with _Opt(0):
        ref = net(rgb, confidence=True).clone()
    for walk in (1, 2):
        with _Opt(walk):
            assert torch.equal(net(rgb, confidence=True), ref)
            run = net.pipelined(3)
            pend = [run(rgb, confidence=True) for _ in range(3)]
            for p in pend:
                assert torch.equal(p.get(), ref)
            graph = net.graphed(rgb, confidence=True)
            assert torch.equal(graph(rgb), ref)
