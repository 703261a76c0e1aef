"""GPU: the f16x1 precision mode (fmt bit 3, omni_stem_sh_f16x1, omni_conv3x3_up2_heads_sh_f16x1, spherical_fusion(precision="f16x1")).

Kernel semantics: an f16x1 convolution multiplies exactly the hi halves the SH operands carry (activations, the hi split of the up-sampled value
for UP2, the hi split of the weights) with fp32 accumulation.  The reference is that product in float64; the gate is fp32-accumulation level,
relative to sum |a||w|; every case also asserts that the gate is tighter than the gap between the hi-only and the exact product, so that an
f16x3 result (or a silent fall-back to it) fails it — and runs the f16x3 kernel once to show that it does."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _glue_cases import f16x1_check, stem_f16x1_refs
from _util import golden, smooth_erp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X1 = 8                                                   # fmt bit 3
REL = 1e-6                                               # fp32-accumulation gate, relative to sum |a||w| (+ |bias| + |res|)

# model gates (max / mean |d| in metres), ~3x what the first run on MI355X measured:
#   f16x1 vs the reference goldens (64 x 128): G6 depth_conf max 0.0178 / mean 0.0024, depth_noconf 0.0128 / 0.0027, G7 it0 max 0.0089 /
#   mean 0.0020, it0_conf 0.0091 / 0.0018
#   f16x1 vs f16x3 at the benched launch (8 x 512 x 1024, pipelined 3): max 0.0167 / mean 0.0024
GOLDEN_MAX, GOLDEN_MEAN = 5e-2, 7e-3
BENCH_MAX, BENCH_MEAN = 5e-2, 7e-3
# the iterative model's second pass feeds the first pass's depth back in (mlp_points2): its difference compounds — measured it1 max 0.0287 /
# mean 0.0071, it1_conf 0.0273 / 0.0058; gated at 1.7x / 2.1x (the computation is deterministic: the margin covers other boxes, not run-to-run noise)
ITER2_MAX, ITER2_MEAN = 5e-2, 1.5e-2


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sh(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_from_f32(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


def _f32(lib, t):
    o = torch.empty_like(t)
    assert lib.omni_sh_to_f32(_p(t), _p(o), ctypes.c_size_t(t.numel()), _stream()) == 0
    return o


def _hi(t_sh):
    """the hi halves of an SH tensor [..., C] (C % 32 == 0) as float64 [..., C]"""
    shp = t_sh.shape
    h = t_sh.contiguous().view(torch.float16).reshape(*shp[:-1], shp[-1] // 32, 2, 32)[..., 0, :]
    return h.reshape(*shp[:-1], shp[-1]).double().cpu()


def _w_hi(w16, Cout):
    """hi halves of a split weight matrix [Cout][K/32][2][32] -> float64 [Cout, K]"""
    return w16[:, :, 0, :].reshape(Cout, -1).double().cpu()


def _act(x, act):
    return F.relu(x) if act == 1 else (F.gelu(x) if act == 2 else x)


class _Options:
    def __init__(self, L, **kv):
        self.L, self.kv, self.old = L, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = self.L.get_option(k)
            self.L.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.L.set_option(k, v)


def _check(out, ref_hi, ref_exact, scale, what):
    """out within REL * scale of the hi-only reference; the hi-only and exact references at least 3x further apart somewhere (tests/_glue_cases.py
    holds the check: tests/test_glue_float64_gpu.py applies the same one to the stem's other launch forms)"""
    return f16x1_check(out, ref_hi, ref_exact, scale, what, REL)


# the shapes of test_conv2d_vs_torch: M, H, W, C1, C2, Cout, k, stride, pad, act, res
CONV_CFGS = [
    (3, 16, 16, 64, 0, 64, 3, 1, 1, 1, True),
    (2, 17, 13, 32, 0, 32, 3, 1, 1, 1, False),
    (5, 32, 32, 64, 0, 128, 3, 2, 1, 1, False),
    (5, 32, 32, 64, 0, 128, 1, 2, 0, 0, False),
    (4, 8, 8, 256, 256, 128, 3, 1, 1, 1, False),
    (36, 4, 4, 512, 0, 512, 3, 1, 1, 1, True),
    (18, 1, 1, 512, 0, 2048, 1, 1, 0, 2, False),
    (40, 64, 64, 32, 0, 32, 3, 1, 1, 1, False),
    (3, 32, 64, 64, 64, 64, 3, 1, 1, 1, True),
    (2, 8, 32, 32, 96, 128, 3, 1, 1, 0, False),
]
# every kernel form conv2d_sh_impl can dispatch, as omni_set_option reaches them
OPTION_SETS = [dict(conv_sh_tile=t) for t in (-1, 0, 1, 2, 3, 4, 5, 7, 8, 9)] + [
    dict(conv_pingpong=0), dict(conv_big_blocks=1), dict(conv_nohalo=1), dict(conv_halo_th=8), dict(conv_halo_th=8, conv_halo_bn=32),
    dict(conv_halo_bn=32), dict(conv_img=2), dict(conv_img=2, conv_halo_bn=32), dict(conv_deep_loaders=0), dict(conv_nodeep=1),
    dict(conv_epi_lds=0), dict(conv_sh_tile=8, conv_big_blocks=1, conv_pingpong=0)]


@pytest.mark.parametrize("cfg", CONV_CFGS)
def test_conv_f16x1_multiplies_the_hi_halves(cfg):
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    M, H, W, C1, C2, Cout, k, s, pad, act, use_res = cfg
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn(M, H, W, C1, generator=g)
    x2 = torch.randn(M, H, W, C2, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, k, k, generator=g) / np.sqrt((C1 + C2) * k * k)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    res = torch.randn(M, Ho, Wo, Cout, generator=g) if use_res else None
    wt = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    W16 = split_weights_f16x3(wt).to(DEV)
    S1 = _sh(lib, x1.to(DEV))
    S2 = _sh(lib, x2.to(DEV)) if C2 else None
    SR = _sh(lib, res.to(DEV)) if use_res else None
    B = b.to(DEV)
    # references: operands exactly as the kernel sees them
    xh = torch.cat([_hi(S1)] + ([_hi(S2)] if C2 else []), -1).permute(0, 3, 1, 2)
    xe = torch.cat([_f32(lib, S1)] + ([_f32(lib, S2)] if C2 else []), -1).double().cpu().permute(0, 3, 1, 2)
    wh = _w_hi(W16, Cout).reshape(Cout, k, k, C1 + C2).permute(0, 3, 1, 2)
    we = (W16[:, :, 0, :].double() + W16[:, :, 1, :].double() * 2.0 ** -11).reshape(Cout, k, k, C1 + C2).permute(0, 3, 1, 2).cpu()
    conv = lambda x_, w_: F.conv2d(x_, w_, stride=s, padding=pad).permute(0, 2, 3, 1)
    rj = _f32(lib, SR).double().cpu() if use_res else 0.0
    ref_hi = _act(conv(xh, wh) + b.double() + rj, act)
    ref_ex = _act(conv(xe, we) + b.double() + rj, act)
    scale = conv(xh.abs(), wh.abs()) + b.double().abs() + (rj.abs() if use_res else 0.0) + 1e-30
    ksteps = k * k * (C1 + C2) // 32
    worst = 0.0
    for opts in OPTION_SETS:
        with _Options(L, **opts):
            for S in sorted({1, min(3, ksteps)}):
                for fmt in (0, 1, 4, 5):
                    ws = torch.empty(max(1, S * M * Ho * Wo * Cout), device=DEV)
                    out = torch.full((M, Ho, Wo, Cout), float("nan"), device=DEV)
                    rc = lib.omni_conv2d_sh_f16x3_ws(_p(S1), _p(S2), _p(W16), _p(B), _p(SR), _p(out), fmt | X1, M, H, W, C1, C2, Cout,
                                                     k, k, s, pad, act, S, _p(ws), ctypes.c_size_t(ws.numel() * 4), _stream())
                    assert rc == 0, lib.omni_last_error()
                    o = _f32(lib, out) if fmt & 1 else out
                    worst = max(worst, _check(o, ref_hi, ref_ex, scale, (opts, S, fmt)))
    # the f16x3 kernel on the same data fails the gate (the test can tell the two modes apart)
    out = torch.empty((M, Ho, Wo, Cout), device=DEV)
    assert lib.omni_conv2d_sh_f16x3_ws(_p(S1), _p(S2), _p(W16), _p(B), _p(SR), _p(out), 0, M, H, W, C1, C2, Cout, k, k, s, pad, act, 1, None,
                                       ctypes.c_size_t(0), _stream()) == 0
    assert ((out.double().cpu() - ref_hi).abs() / scale).max().item() > REL
    print(f"conv {cfg}: max err / sum|a||w| = {worst:.3g}")


def test_conv_post_and_unsupported_forms():
    """omni_conv2d_sh_f16x3_post_ws honours fmt bit 3; the entry points without an f16x1 form refuse it instead of running f16x3."""
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    M, H, W, C, Cout, per = 4, 32, 32, 64, 64, 2
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, H, W, C, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / 24.0
    b = torch.randn(Cout, generator=g)
    post = torch.randn(per, H, W, Cout, generator=g)
    W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV)
    XS, B, PO = _sh(lib, x.to(DEV)), b.to(DEV), post.to(DEV)
    xh = _hi(XS).permute(0, 3, 1, 2)
    wh = _w_hi(W16, Cout).reshape(Cout, 3, 3, C).permute(0, 3, 1, 2)
    we = (W16[:, :, 0, :].double() + W16[:, :, 1, :].double() * 2.0 ** -11).reshape(Cout, 3, 3, C).permute(0, 3, 1, 2).cpu()
    xe = _f32(lib, XS).double().cpu().permute(0, 3, 1, 2)
    pr = post.double().repeat(M // per, 1, 1, 1)
    conv = lambda x_, w_: F.conv2d(x_, w_, padding=1).permute(0, 2, 3, 1)
    ref_hi, ref_ex = F.relu(conv(xh, wh) + b.double()) + pr, F.relu(conv(xe, we) + b.double()) + pr
    scale = conv(xh.abs(), wh.abs()) + b.double().abs() + pr.abs()
    for fmt in (0, 1):
        out = torch.empty((M, H, W, Cout), device=DEV)
        rc = lib.omni_conv2d_sh_f16x3_post_ws(_p(XS), None, _p(W16), _p(B), None, _p(out), fmt | X1, M, H, W, C, 0, Cout, 3, 3, 1, 1, 1, 1, None,
                                              ctypes.c_size_t(0), _p(PO), ctypes.c_size_t(PO.numel()), _stream())
        assert rc == 0, lib.omni_last_error()
        _check(_f32(lib, out) if fmt else out, ref_hi, ref_ex, scale, fmt)
    OMNI_ERR_UNSUPPORTED = 3
    y = torch.empty(32 * 512, device=DEV)
    wr = torch.zeros(512, 512, dtype=torch.float16, device=DEV)
    assert lib.omni_gemm_rows_sh_f16x3(_p(XS), _p(wr), None, None, _p(y), X1, 18, 512, 512, 0, _stream()) == OMNI_ERR_UNSUPPORTED
    assert lib.omni_conv3x3_wino_sh_f16x3(_p(XS), _p(W16), None, None, _p(y), X1, 1, 4, 4, 64, 64, 0, 1, None, ctypes.c_size_t(0), _stream()) == OMNI_ERR_UNSUPPORTED


# M, Hl, Wl, C, Cout, act, options
UP2_CFGS = [
    (2, 16, 16, 64, 64, 1, {}),
    (3, 8, 16, 64, 32, 1, {}),
    (2, 16, 32, 64, 128, 0, {}),
    (4, 32, 32, 32, 32, 1, {}),                          # de_conv4_0's shape: the persistent kernel
    (4, 32, 32, 32, 32, 1, {"conv_up2_persist": 0}),
    (2, 16, 16, 64, 64, 1, {"conv_halo_up2_bn_lat": 32}),
]


@pytest.mark.parametrize("cfg", UP2_CFGS)
def test_up2_conv_f16x1_multiplies_the_hi_split_of_the_upsampled_value(cfg):
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    M, Hl, Wl, C, Cout, act, opts = cfg
    H, W = 2 * Hl, 2 * Wl
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, Hl, Wl, C, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / np.sqrt(9 * C)
    b = torch.randn(Cout, generator=g)
    W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()).to(DEV)
    XS, B = _sh(lib, x.to(DEV)), b.to(DEV)
    up = torch.empty((M, H, W, C), device=DEV)           # the up-sampled value and its split: the same expression as the fused halo fill
    assert lib.omni_upsample_bilinear_sh(_p(XS), _p(up), M, Hl, Wl, C, H, W, _stream()) == 0
    uh, ue = _hi(up).permute(0, 3, 1, 2), _f32(lib, up).double().cpu().permute(0, 3, 1, 2)
    wh = _w_hi(W16, Cout).reshape(Cout, 3, 3, C).permute(0, 3, 1, 2)
    we = (W16[:, :, 0, :].double() + W16[:, :, 1, :].double() * 2.0 ** -11).reshape(Cout, 3, 3, C).permute(0, 3, 1, 2).cpu()
    conv = lambda x_, w_: F.conv2d(x_, w_, padding=1).permute(0, 2, 3, 1)
    ref_hi, ref_ex = _act(conv(uh, wh) + b.double(), act), _act(conv(ue, we) + b.double(), act)
    scale = conv(uh.abs(), wh.abs()) + b.double().abs()
    with _Options(L, **opts):
        for fmt in (0, 1, 4, 5):
            out = torch.full((M, H, W, Cout), float("nan"), device=DEV)
            rc = lib.omni_conv3x3_up2_sh_f16x3(_p(XS), _p(W16), _p(B), _p(out), fmt | X1, M, Hl, Wl, C, Cout, act, _stream())
            assert rc == 0, lib.omni_last_error()
            _check(_f32(lib, out) if fmt & 1 else out, ref_hi, ref_ex, scale, (opts, fmt))
        out = torch.empty((M, H, W, Cout), device=DEV)
        assert lib.omni_conv3x3_up2_sh_f16x3(_p(XS), _p(W16), _p(B), _p(out), 0, M, Hl, Wl, C, Cout, act, _stream()) == 0
        assert ((out.double().cpu() - ref_hi).abs() / scale).max().item() > REL       # f16x3 fails the f16x1 gate


def _heads_ref(y, hw, bp, bw, confidence):
    """y float64 [M,P,P,32]; hw [2][9][32] -> (a, c) float64 [M,P,P]"""
    wk = torch.as_tensor(hw, dtype=torch.float64).reshape(2, 3, 3, 32).permute(0, 3, 1, 2)
    z = F.conv2d(y.permute(0, 3, 1, 2), wk, padding=1)
    pred, wp = F.relu(z[:, 0] + bp), torch.sigmoid(z[:, 1] + bw)
    return (pred * wp if confidence else pred), wp, z


def test_up2_heads_f16x1():
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    M, P = 3, 64
    g = torch.Generator().manual_seed(13)
    x = torch.randn(M, P // 2, P // 2, 32, generator=g)
    w = torch.randn(32, 32, 3, 3, generator=g) / 17.0
    b = torch.randn(32, generator=g) * 0.1
    hw = (torch.randn(2, 9, 32, generator=g) / 17.0).numpy().astype(np.float32)
    bp, bw = 0.05, -0.1
    W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(32, -1).contiguous()).to(DEV)
    frag = np.zeros(4 * 64 * 8, np.float16)
    assert lib.omni_heads_pack_f16x3(hw.ctypes.data_as(ctypes.c_void_p), frag.ctypes.data_as(ctypes.c_void_p)) == 0
    HW, XS, B = torch.from_numpy(frag).to(DEV), _sh(lib, x.to(DEV)), b.to(DEV)
    up = torch.empty((M, P, P, 32), device=DEV)
    assert lib.omni_upsample_bilinear_sh(_p(XS), _p(up), M, P // 2, P // 2, 32, P, P, _stream()) == 0
    uh, ue = _hi(up).permute(0, 3, 1, 2), _f32(lib, up).double().cpu().permute(0, 3, 1, 2)
    wh = _w_hi(W16, 32).reshape(32, 3, 3, 32).permute(0, 3, 1, 2)
    we = (W16[:, :, 0, :].double() + W16[:, :, 1, :].double() * 2.0 ** -11).reshape(32, 3, 3, 32).permute(0, 3, 1, 2).cpu()
    conv = lambda x_, w_: F.conv2d(x_, w_, padding=1).permute(0, 2, 3, 1)
    y_hi, y_ex = F.relu(conv(uh, wh) + b.double()), F.relu(conv(ue, we) + b.double())
    y_scale = conv(uh.abs(), wh.abs()) + b.double().abs()
    # the heads sum 288 products of y: the gate is relative to their L2 norm (1e-5: the heads' own f16x3 products and fp32 sums), plus the
    # conv's fp32 error carried through (1e-7 of sum |w| y_scale); the hi-only / exact gap of y moves the heads by ~4e-4 of that L2 norm
    _, _, zs = _heads_ref(y_scale, np.abs(hw), 0.0, 0.0, False)
    _, _, z2 = _heads_ref(y_hi ** 2, hw.astype(np.float64) ** 2, 0.0, 0.0, False)
    zt = 1e-5 * z2.sqrt() + 1e-7 * zs + 1e-12
    nb = int(lib.omni_up2_heads_scratch_bytes(M, P))
    scratch = torch.empty((nb + 3) // 4, device=DEV)
    for conf in (1, 0):
        a_hi, c_hi, z_hi = _heads_ref(y_hi, hw, bp, bw, conf)
        a_ex, c_ex, _ = _heads_ref(y_ex, hw, bp, bw, conf)
        tol_p, tol_w = zt[:, 0], zt[:, 1]
        tol_a = tol_p + (z_hi[:, 0] + bp).abs() * tol_w if conf else tol_p
        oa, oc = torch.empty((M, P, P), device=DEV), torch.empty((M, P, P), device=DEV)
        for fn in (lib.omni_conv3x3_up2_heads_sh_f16x1, lib.omni_conv3x3_up2_heads_sh_f16x3):
            rc = fn(_p(XS), _p(W16), _p(B), _p(HW), ctypes.c_float(bp), ctypes.c_float(bw), _p(scratch), ctypes.c_size_t(nb), _p(oa), _p(oc), M, P, conf, _stream())
            assert rc == 0, lib.omni_last_error()
            ea, ec = ((oa.double().cpu() - a_hi).abs() / tol_a).max().item(), ((oc.double().cpu() - c_hi).abs() / tol_w).max().item()
            if fn is lib.omni_conv3x3_up2_heads_sh_f16x1:
                assert ea <= 1 and ec <= 1, (conf, ea, ec)
            else:
                assert max(ea, ec) > 1, (conf, ea, ec)             # f16x3 fails the f16x1 gate
        assert ((a_ex - a_hi).abs() / tol_a).max().item() > 3


@pytest.mark.parametrize("opts", [{}, {"conv_stem_pc": 0}, {"conv_epi_lds": 0}, {"conv_stem_pc": 0, "conv_epi_lds": 0}])
@pytest.mark.parametrize("M", [1, 12])
def test_stem_f16x1(opts, M):
    L, lib = _lib()
    from omnifusion_amd.model._engine import split_weights_f16x3
    P = 128
    g = torch.Generator().manual_seed(17)
    x = torch.rand(M, 3, P, P, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 12.0
    b = torch.randn(64, generator=g) * 0.1
    wk = torch.zeros(64, 3, 7, 8); wk[..., :7] = w
    W16 = split_weights_f16x3(torch.cat([wk.reshape(64, 168), torch.zeros(64, 24)], 1)).to(DEV)
    X, B = x.to(DEV), b.to(DEV)
    ref_hi, ref_ex, scale = stem_f16x1_refs(x, b, W16)
    with _Options(L, **opts):
        out = torch.full((M, P // 2, P // 2, 64), float("nan"), device=DEV)
        assert lib.omni_stem_sh_f16x1(_p(X), _p(W16), _p(B), _p(out), M, P, _stream()) == 0, lib.omni_last_error()
        _check(_f32(lib, out), ref_hi, ref_ex, scale, opts)
        assert lib.omni_stem_sh_f16x3(_p(X), _p(W16), _p(B), _p(out), M, P, _stream()) == 0
        assert ((_f32(lib, out).double().cpu() - ref_hi).abs() / scale).max().item() > REL


# ---------------------------------------------------------------------------------------------------- the model

def _nets():
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
    from omnifusion_amd.weights import make_state_dict
    return spherical_fusion, spherical_fusion_it, make_state_dict


def _report(what, got, want):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print(f"{what}: max |d| = {d.max():.4g} m, mean |d| = {d.mean():.4g} m")
    return d.max(), d.mean()


def test_model_single_f16x1_against_the_golden():
    spherical_fusion, _, make_state_dict = _nets()
    g = golden("G6_model_single")
    net = spherical_fusion(4, 18, (128, 128), (80, 80), precision="f16x1").cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    assert net.precision == "f16x1"
    rgb = torch.from_numpy(g["rgb"]).to(DEV)
    got = {}
    for conf, key in ((True, "depth_conf"), (False, "depth_noconf")):
        got[key] = _report(f"single-pass f16x1 vs G6 {key}", net(rgb, confidence=conf).cpu().numpy(), g[key])
    assert all(mx <= GOLDEN_MAX and mn <= GOLDEN_MEAN for mx, mn in got.values()), got
    assert not net.overflowed()


def test_model_iterative_f16x1_against_the_golden():
    _, spherical_fusion_it, make_state_dict = _nets()
    g = golden("G7_model_iterative")
    net = spherical_fusion_it(4, 18, (128, 128), (80, 80), precision="f16x1").cuda()
    net.load_state_dict(make_state_dict(42, 18, True))
    rgb = torch.from_numpy(g["rgb"]).to(DEV)
    got = {}
    o = net(rgb, iter=2)
    for i, key in enumerate(("it0", "it1")):
        got[key] = _report(f"iterative f16x1 vs G7 {key}", o[i].cpu().numpy(), g[key])
    o = net(rgb, 2, confidence=True)
    for i, key in enumerate(("it0_conf", "it1_conf")):
        got[key] = _report(f"iterative f16x1 vs G7 {key}", o[i].cpu().numpy(), g[key])
    for key, (mx, mn) in got.items():
        gmax, gmean = (ITER2_MAX, ITER2_MEAN) if key.startswith("it1") else (GOLDEN_MAX, GOLDEN_MEAN)
        assert mx <= gmax and mn <= gmean, (key, got)


def _bench_pair():
    spherical_fusion, _, make_state_dict = _nets()
    sd = make_state_dict(42, 18, False)
    nets = {}
    for prec in ("f16x3", "f16x1"):
        n = spherical_fusion(4, 18, (128, 128), (80, 80), precision=prec).cuda()
        n.load_state_dict(sd)
        nets[prec] = n
    rgb = torch.from_numpy(smooth_erp(77, 8, 3, 512, 1024)).to(DEV)
    return nets, rgb


def test_benched_launch_f16x1_against_f16x3_and_determinism():
    """B = 8 panoramas of 512 x 1024, pipelined depth 3 (the launch bench.py times): f16x1 against f16x3 within the gate; two runs bit-identical;
    pipelined equal to a plain call bit for bit; the DataParallel device context carries the mode."""
    nets, rgb = _bench_pair()
    runs = {}
    for prec, net in nets.items():
        run = net.pipelined(3)
        pend = [run(rgb) for _ in range(3)]
        outs = [p.get() for p in pend]
        torch.cuda.synchronize()
        assert all(torch.equal(outs[0], o) for o in outs[1:]), prec
        runs[prec] = outs[0]
    mx, mn = _report("benched launch f16x1 vs f16x3 (B=8, 512x1024, pipelined 3)", runs["f16x1"].cpu().numpy(), runs["f16x3"].cpu().numpy())
    assert 1e-5 < mx <= BENCH_MAX and mn <= BENCH_MEAN, (mx, mn)
    plain = nets["f16x1"](rgb)
    assert torch.equal(plain, runs["f16x1"])
    assert torch.equal(nets["f16x1"](rgb), plain)                   # two plain runs
    assert nets["f16x1"]._device_context(DEV).eng.precision == "f16x1"


def test_graphed_single_panorama_equals_eager_f16x1():
    nets, rgb = _bench_pair()
    net = nets["f16x1"]
    one = rgb[:1].contiguous()
    eager = net(one).clone()
    run = net.graphed(one)
    got = run(one).clone()
    assert torch.equal(got, eager)
    p = net.pipelined(2, graphs=True)
    assert torch.equal(p(one).get(), eager)


def test_modes_interleaved_in_one_process_do_not_interact():
    """An f16x3 module interleaved with an f16x1 module (same stream, then two concurrent streams) gives the bits of an f16x3-only run."""
    nets, rgb = _bench_pair()
    ref = nets["f16x3"](rgb).clone()
    x1_ref = nets["f16x1"](rgb).clone()
    torch.cuda.synchronize()
    for _ in range(2):
        a = nets["f16x3"](rgb)
        b = nets["f16x1"](rgb)
        assert torch.equal(a, ref) and torch.equal(b, x1_ref)
    s3, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    s3.wait_stream(cur); s1.wait_stream(cur)
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s3):
            outs.append(("f16x3", nets["f16x3"](rgb)))
        with torch.cuda.stream(s1):
            outs.append(("f16x1", nets["f16x1"](rgb)))
    torch.cuda.synchronize()
    for prec, o in outs:
        assert torch.equal(o, ref if prec == "f16x3" else x1_ref), prec


def _eval_averages(precision, out):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--batches", "3", "--batch", "4", "--height", "256", "--width", "512",
           "--ply-every", "0", "--out", str(out), "--precision", precision]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    vals = {}
    for line in r.stdout.splitlines():
        if ":" in line and line.strip().startswith(("Avg.", "Inlier")):
            k, v = line.rsplit(":", 1)
            vals[k.strip()] = float(v)
    return vals


def test_eval_tool_f16x1_matches_f16x3(tmp_path):
    a3, a1 = _eval_averages("f16x3", tmp_path), _eval_averages("f16x1", tmp_path)
    print("eval f16x3:", a3, "\neval f16x1:", a1)
    assert abs(a3["Avg. Abs. Rel. Error"] - a1["Avg. Abs. Rel. Error"]) <= 1e-3
    assert abs(a3["Inlier D1"] - a1["Inlier D1"]) <= 1e-3
