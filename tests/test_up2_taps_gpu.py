"""The decoder stages that multiply before up-sampling (Engine.taps_first): omni_up2_tapsum_sh alone, the whole stage (tap GEMM + tap sum)
against the two kernels it replaces and against float64, the range guard, and the models with the stages switched one by one."""
import ctypes

import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, tap_sum, taps_repack
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _n(t):
    return ctypes.c_size_t(t.numel())


def _from_sh(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_to_f32(_p(t), _p(o), _n(t), _stream()) == 0
    return o


def _to_sh(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_from_f32(_p(t), _p(o), _n(t), _stream()) == 0
    return o


@pytest.mark.parametrize("cfg", [(3, 4, 4, 64, 1), (2, 8, 8, 32, 1), (1, 1, 1, 32, 0), (2, 2, 3, 32, 1), (5, 4, 4, 96, 0)])
def test_tapsum_kernel_vs_float64(cfg):
    """omni_up2_tapsum_sh on random fp32 tap products against the float64 restatement: the bound of an SH output, 4e-6 x max |ref|
    (test_sh_range_guard_and_large_magnitudes).  1x1: every source index clamps; 2x3: not square, odd width; 96 channels: three slabs.
    Two launches give the same bits."""
    L, lib = _lib()
    M, Hl, Wl, Cout, act = cfg
    g = torch.Generator().manual_seed(17)
    y = torch.randn(M, Hl, Wl, 9, Cout, generator=g); b = torch.randn(Cout, generator=g)
    ref = tap_sum(y, b, relu=act == 1)
    Y, B = y.to(DEV), b.to(DEV)
    guard = torch.zeros(4096, device=DEV)
    outs = []
    for _ in range(2):
        o = torch.full((M, 2 * Hl, 2 * Wl, Cout), float("nan"), device=DEV)
        assert lib.omni_up2_tapsum_sh(_p(Y), _p(B), _p(o), M, Hl, Wl, Cout, act, _stream()) == 0, lib.omni_last_error()
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    d = (_from_sh(lib, outs[0]).cpu().double() - ref).abs().max().item()
    print(f"tap sum {cfg}: max |d| = {d:.3g}, bound {4e-6 * ref.abs().max().item():.3g}")
    assert d <= 4e-6 * ref.abs().max().item()
    assert guard.abs().max().item() == 0
    nobias = torch.empty_like(outs[0])                                                   # bias is optional
    assert lib.omni_up2_tapsum_sh(_p(Y), None, _p(nobias), M, Hl, Wl, Cout, 0, _stream()) == 0
    assert (_from_sh(lib, nobias).cpu().double() - tap_sum(y)).abs().max().item() <= 4e-6 * ref.abs().max().item()


def test_tapsum_refuses_what_it_does_not_serve():
    L, lib = _lib()
    y = torch.zeros(1 * 16 * 16 * 9 * 64, device=DEV); o = torch.zeros(1 * 32 * 32 * 64, device=DEV)
    assert lib.omni_up2_tapsum_sh(_p(y), None, _p(o), 1, 16, 16, 32, 1, _stream()) == L.OMNI_ERR_UNSUPPORTED   # 256 source pixels: more than a block stages
    assert lib.omni_up2_tapsum_sh(_p(y), None, _p(o), 1, 4, 4, 48, 1, _stream()) == L.OMNI_ERR_UNSUPPORTED     # not a multiple of the 32-channel group
    assert lib.omni_up2_tapsum_sh(_p(y), None, _p(o), 1, 4, 4, 32, 2, _stream()) == L.OMNI_ERR_UNSUPPORTED     # GELU
    assert lib.omni_up2_tapsum_sh(_p(y), None, _p(o), 0, 4, 4, 32, 1, _stream()) == L.OMNI_ERR_INVALID
    assert o.abs().max().item() == 0


@pytest.mark.parametrize("cfg", [(3, 4, 4, 512, 256), (2, 8, 8, 128, 128), (2, 4, 4, 64, 64), (1, 2, 3, 32, 32)])
def test_stage_vs_two_kernels_and_float64(cfg):
    """The whole stage — nine 1x1 tap products on the low-resolution map (omni_conv2d_sh_f16x3_ws on the tap-major operand) + omni_up2_tapsum_sh —
    against omni_upsample_bilinear_sh + omni_conv2d_sh_f16x3_ws and against float64 torch: the convolution bound at these statistics, 3e-5
    (test_conv2d_vs_torch, test_fused_upsample_conv_equals_the_two_kernels)."""
    L, lib = _lib()
    M, Hl, Wl, C, Cout = cfg
    from omnifusion_amd.model._engine import split_weights_f16x3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, Hl, Wl, C, generator=g); w = torch.randn(Cout, C, 3, 3, generator=g) / np.sqrt(9 * C); b = torch.randn(Cout, generator=g)
    X, B = x.to(DEV), b.to(DEV)
    XS = _to_sh(lib, X)
    W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV)
    W16T = split_weights_f16x3(taps_repack(w).contiguous()).to(DEV)
    H, W = 2 * Hl, 2 * Wl
    up = torch.empty((M, H, W, C), device=DEV)
    assert lib.omni_upsample_bilinear_sh(_p(XS), _p(up), M, Hl, Wl, C, H, W, _stream()) == 0
    two = torch.empty((M, H, W, Cout), device=DEV)
    assert lib.omni_conv2d_sh_f16x3_ws(_p(up), None, _p(W16), _p(B), None, _p(two), 1, M, H, W, C, 0, Cout, 3, 3, 1, 1, 1,
                                       1, None, ctypes.c_size_t(0), _stream()) == 0, lib.omni_last_error()
    Y = torch.empty((M, Hl, Wl, 9 * Cout), device=DEV)
    assert lib.omni_conv2d_sh_f16x3_ws(_p(XS), None, _p(W16T), None, None, _p(Y), 0, M, Hl, Wl, C, 0, 9 * Cout, 1, 1, 1, 0, 0,
                                       1, None, ctypes.c_size_t(0), _stream()) == 0, lib.omni_last_error()
    taps = torch.empty((M, H, W, Cout), device=DEV)
    assert lib.omni_up2_tapsum_sh(_p(Y), _p(B), _p(taps), M, Hl, Wl, Cout, 1, _stream()) == 0, lib.omni_last_error()
    ref = direct(_from_sh(lib, XS).cpu(), w, b, relu=True)
    got, old = _from_sh(lib, taps).cpu().double(), _from_sh(lib, two).cpu().double()
    d64, dold = (got - ref).abs().max().item(), (got - old).abs().max().item()
    print(f"stage {cfg}: vs float64 {d64:.3g} (the two kernels: {(old - ref).abs().max().item():.3g}), vs the two kernels {dold:.3g}; ref max {ref.abs().max().item():.3g}")
    assert d64 < 3e-5
    assert dold < 3e-5


def test_tapsum_range_guard():
    """outputs beyond the fp16 range saturate, raise the sticky flag (omni_sh_overflow reports and clears it) and never turn into NaN"""
    L, lib = _lib()
    flag = ctypes.c_int(0)
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0                       # clear
    M, Hl, Wl, Cout = 1, 4, 4, 32
    y = (torch.randn(M, Hl, Wl, 9, Cout, generator=torch.Generator().manual_seed(2)) * 1e5).to(DEV)
    o = torch.empty((M, 2 * Hl, 2 * Wl, Cout), device=DEV)
    assert lib.omni_up2_tapsum_sh(_p(y), None, _p(o), M, Hl, Wl, Cout, 0, _stream()) == 0
    v = _from_sh(lib, o).cpu()
    assert not torch.isnan(v).any() and v.max().item() == 65504.0 and v.min().item() == -65504.0
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 1   # raised, then cleared by the reset
    assert lib.omni_sh_overflow(ctypes.byref(flag), 0) == 0 and flag.value == 0
    assert lib.omni_up2_tapsum_sh(_p(y * 1e-5), None, _p(o), M, Hl, Wl, Cout, 0, _stream()) == 0
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 0   # in range: stays down


# ------------------------------------------------------------------ the models
NONE, L0, L1, BOTH = frozenset(), frozenset(("de_conv0_0",)), frozenset(("de_conv1_0",)), frozenset(("de_conv0_0", "de_conv1_0"))


class _Taps:
    def __init__(self, layers):
        self.layers = layers

    def __enter__(self):
        from omnifusion_amd.model._engine import Engine
        self.saved, Engine.taps_first = Engine.taps_first, self.layers

    def __exit__(self, *exc):
        from omnifusion_amd.model._engine import Engine
        Engine.taps_first = self.saved


@pytest.fixture(scope="module")
def nets():
    """the inputs of test_engine_switches_are_result_neutral, and what the models give with no stage on the new path (computed once, never changed)"""
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    net_it = spherical_fusion_it(4, 18, (128, 128), (80, 80)).cuda()
    net_it.load_state_dict(make_state_dict(42, 18, True))
    rgb = torch.rand((3, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    one = rgb[:1].contiguous()
    with _Taps(NONE):
        ref = (net(rgb, confidence=True).clone(), net(one, confidence=True).clone(), net_it(rgb, 2)[-1].clone())
    return net, net_it, rgb, one, ref


@pytest.mark.parametrize("layers", [L0, L1, BOTH], ids=["de_conv0_0", "de_conv1_0", "both"])
def test_models_agree_between_the_paths(nets, layers):
    """single-pass model, iterative model and a lone panorama: the new path changes the result by rounding only (< 2e-5, the bound of
    test_engine_switches_are_result_neutral for such switches)"""
    net, net_it, rgb, one, ref = nets
    with _Taps(layers):
        out, out1, out_it = net(rgb, confidence=True), net(one, confidence=True), net_it(rgb, 2)[-1]
    d = [(a - b).abs().max().item() for a, b in zip((out, out1, out_it), ref)]
    print(f"taps_first = {sorted(layers)}: max |d| single pass {d[0]:.3g}, lone panorama {d[1]:.3g}, iterative {d[2]:.3g}")
    assert max(d) < 2e-5, d


def test_new_path_keeps_the_bit_for_bit_guarantees(nets):
    """with both stages on: a panorama's bits do not depend on the batch; pipelined(3) and graphed() give the bits of plain calls"""
    net, net_it, rgb, one, ref = nets
    with _Taps(BOTH):
        out = net(rgb, confidence=True).clone()
        two = net(rgb[:2].contiguous(), confidence=True).clone()
        four = net(torch.cat([rgb[:2], rgb[2:], rgb[:1]]), confidence=True)
        assert torch.equal(four[:2], two) and torch.equal(four[:3], out)
        run = net.pipelined(3)
        pend = [run(rgb, confidence=True) for _ in range(3)]
        for p in pend:
            assert torch.equal(p.get(), out)
        graph = net.graphed(rgb, confidence=True)
        assert torch.equal(graph(rgb), out)
        assert torch.equal(graph(rgb.flip(0)), net(rgb.flip(0), confidence=True))


def test_goldens_with_both_stages_on():
    """G6 / G7 (the reference's own outputs) within 1e-3 with both stages on the new path, whatever default ships"""
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
    from omnifusion_amd.weights import make_state_dict
    with _Taps(BOTH):
        g = golden("G6_model_single")
        net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
        net.load_state_dict(make_state_dict(42, 18, False))
        rgb = torch.from_numpy(g["rgb"]).to(DEV)
        assert np.abs(net(rgb, confidence=True).cpu().numpy() - g["depth_conf"]).max() <= 1e-3
        assert np.abs(net(rgb, confidence=False).cpu().numpy() - g["depth_noconf"]).max() <= 1e-3
        g7 = golden("G7_model_iterative")
        net_it = spherical_fusion_it(4, 18, (128, 128), (80, 80)).cuda()
        net_it.load_state_dict(make_state_dict(42, 18, True))
        o = net_it(torch.from_numpy(g7["rgb"]).to(DEV), iter=2)
        assert np.abs(o[0].cpu().numpy() - g7["it0"]).max() <= 1e-3 and np.abs(o[1].cpu().numpy() - g7["it1"]).max() <= 1e-3
