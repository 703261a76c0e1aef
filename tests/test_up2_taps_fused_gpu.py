"""The 64 -> 64 decoder stages as tap products summed in LDS (Engine.taps_fused, omni_conv3x3_up2_taps_sh_f16x3): the kernel against float64 and
against the up-sampling halo kernel it replaces, the range guard, and the models with the stages switched one by one."""
import ctypes

import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, taps_repack

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


# whole-image form: 16 x 16, M = 3 (odd: image strides) and M = 1; band form (Wl = 32, 8-row bands): Hl = 24 has a first, an interior and a last band
@pytest.mark.parametrize("cfg", [(3, 16, 16), (1, 16, 16), (2, 24, 32)], ids=["image_m3", "image_m1", "bands_m2"])
def test_stage_vs_halo_kernel_and_float64(cfg):
    """One launch against float64 torch (`direct`) and against omni_conv3x3_up2_sh_f16x3, with ReLU and without: inputs and the bound of
    test_stage_vs_two_kernels_and_float64 (randn inputs, weights / sqrt(9 C), bias; < 3e-5 to both).  Two launches give the same bits and every
    output element is written (the result buffers start as NaN)."""
    L, lib = _lib()
    M, Hl, Wl = cfg
    C = Cout = 64
    from omnifusion_amd.model._engine import split_weights_f16x3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, Hl, Wl, C, generator=g); w = torch.randn(Cout, C, 3, 3, generator=g) / np.sqrt(9 * C); b = torch.randn(Cout, generator=g)
    X, B = x.to(DEV), b.to(DEV)
    XS = _to_sh(lib, X)
    W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV)
    W16T = split_weights_f16x3(taps_repack(w).contiguous()).to(DEV)
    H, W = 2 * Hl, 2 * Wl
    xs = _from_sh(lib, XS).cpu()
    for act in (1, 0):
        old = torch.empty((M, H, W, Cout), device=DEV)
        assert lib.omni_conv3x3_up2_sh_f16x3(_p(XS), _p(W16), _p(B), _p(old), 1, M, Hl, Wl, C, Cout, act, _stream()) == 0, lib.omni_last_error()
        outs = []
        for _ in range(2):
            o = torch.full((M, H, W, Cout), float("nan"), device=DEV)
            assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), _p(B), _p(o), 1, M, Hl, Wl, C, Cout, act, _stream()) == 0, lib.omni_last_error()
            outs.append(o)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        ref = direct(xs, w, b, relu=act == 1)
        got, was = _from_sh(lib, outs[0]).cpu().double(), _from_sh(lib, old).cpu().double()
        assert not torch.isnan(got).any()
        d64, dold = (got - ref).abs().max().item(), (got - was).abs().max().item()
        print(f"stage {cfg} act {act}: vs float64 {d64:.3g} (the halo kernel: {(was - ref).abs().max().item():.3g}), vs the halo kernel {dold:.3g}; ref max {ref.abs().max().item():.3g}")
        assert d64 < 3e-5
        assert dold < 3e-5
    nobias = torch.empty((M, H, W, Cout), device=DEV)                                    # bias is optional
    assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), None, _p(nobias), 1, M, Hl, Wl, C, Cout, 0, _stream()) == 0
    assert (_from_sh(lib, nobias).cpu().double() - direct(xs, w)).abs().max().item() < 3e-5


def test_image_bits_do_not_depend_on_the_batch():
    """an image inside a batch of 3 and alone: the same bits (both forms)"""
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 64, 3, 3, generator=g) / 24.0
    W16T = split_weights_f16x3(taps_repack(w).contiguous()).to(DEV)
    for Hl, Wl in ((16, 16), (8, 32)):
        XS = _to_sh(lib, torch.randn(3, Hl, Wl, 64, generator=g).to(DEV))
        o3 = torch.empty((3, 2 * Hl, 2 * Wl, 64), device=DEV); o1 = torch.empty((1, 2 * Hl, 2 * Wl, 64), device=DEV)
        assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), None, _p(o3), 1, 3, Hl, Wl, 64, 64, 1, _stream()) == 0
        last = XS[2:].contiguous()
        assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(last), _p(W16T), None, _p(o1), 1, 1, Hl, Wl, 64, 64, 1, _stream()) == 0
        assert torch.equal(o3[2:].view(torch.int32), o1.view(torch.int32))


def test_range_guard():
    """outputs beyond the fp16 range saturate, raise the sticky flag (omni_sh_overflow reports and clears it) and never turn into NaN"""
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    flag = ctypes.c_int(0)
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0                       # clear
    g = torch.Generator().manual_seed(2)
    w = torch.randn(64, 64, 3, 3, generator=g)
    W16T = split_weights_f16x3(taps_repack(w).contiguous()).to(DEV)
    x = torch.randn(1, 16, 16, 64, generator=g).to(DEV)
    XS = _to_sh(lib, x * 1e4)                                                     # sums of 576 products of magnitude 1e4: far beyond 65504
    o = torch.empty((1, 32, 32, 64), device=DEV)
    assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(XS), _p(W16T), None, _p(o), 1, 1, 16, 16, 64, 64, 0, _stream()) == 0
    v = _from_sh(lib, o).cpu()
    assert not torch.isnan(v).any() and v.max().item() == 65504.0 and v.min().item() == -65504.0
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 1   # raised, then cleared by the reset
    assert lib.omni_sh_overflow(ctypes.byref(flag), 0) == 0 and flag.value == 0
    assert lib.omni_conv3x3_up2_taps_sh_f16x3(_p(_to_sh(lib, x)), _p(W16T), None, _p(o), 1, 1, 16, 16, 64, 64, 0, _stream()) == 0
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0 and flag.value == 0   # in range: stays down


# ------------------------------------------------------------------ the models
NONE, L2, L3, BOTH = frozenset(), frozenset(("de_conv2_0",)), frozenset(("de_conv3_0",)), frozenset(("de_conv2_0", "de_conv3_0"))


class _Fused:
    def __init__(self, layers):
        self.layers = layers

    def __enter__(self):
        from omnifusion_amd.model._engine import Engine
        self.saved, Engine.taps_fused = Engine.taps_fused, self.layers

    def __exit__(self, *exc):
        from omnifusion_amd.model._engine import Engine
        Engine.taps_fused = self.saved


@pytest.fixture(scope="module")
def nets():
    """the inputs of test_up2_taps_gpu.py's model tests, and what the models give with no stage on the new path (computed once, never changed)"""
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    net_it = spherical_fusion_it(4, 18, (128, 128), (80, 80)).cuda()
    net_it.load_state_dict(make_state_dict(42, 18, True))
    rgb = torch.rand((3, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    one = rgb[:1].contiguous()
    with _Fused(NONE):
        ref = (net(rgb, confidence=True).clone(), net(one, confidence=True).clone(), net_it(rgb, 2)[-1].clone())
    return net, net_it, rgb, one, ref


@pytest.mark.parametrize("layers", [L2, L3, BOTH], ids=["de_conv2_0", "de_conv3_0", "both"])
def test_models_agree_between_the_paths(nets, layers):
    """single-pass model, a lone panorama and the iterative model: the new path changes the result by rounding only (< 2e-5)"""
    net, net_it, rgb, one, ref = nets
    with _Fused(layers):
        out, out1, out_it = net(rgb, confidence=True), net(one, confidence=True), net_it(rgb, 2)[-1]
    d = [(a - b).abs().max().item() for a, b in zip((out, out1, out_it), ref)]
    print(f"taps_fused = {sorted(layers)}: max |d| single pass {d[0]:.3g}, lone panorama {d[1]:.3g}, iterative {d[2]:.3g}")
    assert max(d) > 0, "the switch changed nothing: the new path did not run"
    assert max(d) < 2e-5, d


def test_new_path_keeps_the_bit_for_bit_guarantees(nets):
    """with both stages on: a panorama's bits do not depend on the batch; pipelined(3) and graphed() give the bits of plain calls"""
    net, net_it, rgb, one, ref = nets
    with _Fused(BOTH):
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


@pytest.mark.parametrize("precision", ["f16x1", "fp32"])
def test_other_modes_keep_the_old_path(precision):
    """f16x1 and fp32: the key set changes no bit"""
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80), precision=precision).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    rgb = torch.rand((2, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    with _Fused(NONE):
        off = net(rgb, confidence=True).clone()
    with _Fused(BOTH):
        on = net(rgb, confidence=True).clone()
    assert torch.equal(on, off)
