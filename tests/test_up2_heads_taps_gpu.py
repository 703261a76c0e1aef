"""GPU: up2_heads_taps_kernel (csrc/omni_conv_up2_heads_taps.hip) — de_conv4_0 + the heads as tap products on the 64 x 64 map — behind option
`conv_up2_heads_taps` of omni_conv3x3_up2_heads_sh_f16x3, against the g1 kernel (option 0) and a float64 restatement of the operator on the CPU.

The tolerance is measured in the same run: the g1 kernel's max |error| against float64 on the same inputs; the new kernel must stay within 1.5 x that,
per output tensor (the margin allows for a different but equally long fp32 summation).  Both errors are printed."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT = "conv_up2_heads_taps"
HB = (0.3, -0.2)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Option:
    """sets the option, puts the shipped value back"""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from omnifusion_amd import _lib
        self.saved = _lib.get_option(OPT)
        _lib.set_option(OPT, self.value)

    def __exit__(self, *exc):
        from omnifusion_amd import _lib
        _lib.set_option(OPT, self.saved)


def _inputs(M, P, seed):
    """image 0: Normal(0, 1); image 1 (if any): scaled so that inputs and, in the channels without a bias, outputs fall below the range guard's 6.1e-5;
    image 2 (if any): zeros but the four corners and the edge midpoints (clamps and padding taps)"""
    g = torch.Generator().manual_seed(seed)
    Pl = P // 2
    x = torch.randn(M, Pl, Pl, 32, generator=g)
    if M > 1:
        x[1] *= 2e-4
    if M > 2:
        keep = torch.zeros(Pl, Pl, dtype=torch.bool)
        for r in (0, Pl // 2, Pl - 1):
            for c in (0, Pl // 2, Pl - 1):
                keep[r, c] = (r, c) != (Pl // 2, Pl // 2)
        x[2] *= keep[:, :, None]
    w = torch.randn(32, 32, 3, 3, generator=g) / np.sqrt(9 * 32)
    b = torch.randn(32, generator=g) * 0.3
    b[:8] = 0.0
    hw = torch.randn(2, 32, 3, 3, generator=g) / np.sqrt(9 * 32) * 2.0
    return x, w, b, hw


class _Case:
    """device operands of one (M, P) and the float64 reference, computed once"""
    def __init__(self, M, P, seed=29):
        from omnifusion_amd import _lib as L
        from omnifusion_amd.model._engine import split_weights_f16x3
        self.lib = lib = L.load()
        self.M, self.P = M, P
        x, w, b, hw = _inputs(M, P, seed)
        self.B = b.to(DEV)
        self.W16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(32, -1).contiguous()).to(DEV)
        X = x.to(DEV)
        self.XS = torch.empty_like(X)
        assert lib.omni_sh_from_f32(_p(X), _p(self.XS), ctypes.c_size_t(X.numel()), _stream()) == 0
        hw_nhwc = np.ascontiguousarray(hw.permute(0, 2, 3, 1).reshape(2, 9, 32).numpy())
        frag = np.zeros(4 * 64 * 8, np.float16)
        assert lib.omni_heads_pack_f16x3(hw_nhwc.ctypes.data_as(ctypes.c_void_p), frag.ctypes.data_as(ctypes.c_void_p)) == 0
        self.HF = torch.from_numpy(frag).to(DEV)
        self.nb = int(lib.omni_up2_heads_scratch_bytes(M, P))
        # float64 on the CPU, from the joined SH input and the fp32 weights
        back = torch.empty_like(X)
        assert lib.omni_sh_to_f32(_p(self.XS), _p(back), ctypes.c_size_t(X.numel()), _stream()) == 0
        up = F.interpolate(back.cpu().double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
        y = F.relu(F.conv2d(up, w.double(), b.double(), padding=1))
        hd = F.conv2d(y, hw.double(), torch.tensor(HB, dtype=torch.float64), padding=1)
        self.pred, self.conf = F.relu(hd[:, 0]), torch.sigmoid(hd[:, 1])

    def run(self, option, confidence, with_c=True, images=None):
        """-> (out_a, out_c or None, hr) of images `images` (a slice; default all)"""
        lib, P = self.lib, self.P
        XS = self.XS if images is None else self.XS[images].contiguous()
        M = XS.shape[0]
        nb = int(lib.omni_up2_heads_scratch_bytes(M, P))
        hr = torch.full((nb // 4,), float("nan"), device=DEV)
        a = torch.full((M, P, P), float("nan"), device=DEV)
        c = torch.full((M, P, P), float("nan"), device=DEV) if with_c else None
        with _Option(option):
            rc = lib.omni_conv3x3_up2_heads_sh_f16x3(_p(XS), _p(self.W16), _p(self.B), _p(self.HF), ctypes.c_float(HB[0]), ctypes.c_float(HB[1]), _p(hr),
                                                     ctypes.c_size_t(nb), _p(a), _p(c), M, P, 1 if confidence else 0, _stream())
        assert rc == 0, lib.omni_last_error()
        torch.cuda.synchronize()
        return a, c, hr

    def errors(self, a, c, confidence, images=slice(None)):
        want = self.pred[images] * self.conf[images] if confidence else self.pred[images]
        return (a.cpu().double() - want).abs().max().item(), (c.cpu().double() - self.conf[images]).abs().max().item()


@pytest.fixture(scope="module")
def three():
    return _Case(3, 128)


def _hr_written(hr):
    """every record holds its 34 sums, the two floats of padding are never written"""
    r = hr.view(-1, 36)
    return bool(torch.isfinite(r[:, :34]).all()) and bool(torch.isnan(r[:, 34:]).all())


def test_one_patch_every_band_and_tile_column(three):
    """M = 1: the first, the inner and the last bands of an image, all four tile columns of `hr`; within 1.5 x the g1 kernel's error"""
    a0, c0, hr0 = three.run(0, True, images=slice(0, 1))
    a1, c1, hr1 = three.run(1, True, images=slice(0, 1))
    assert _hr_written(hr0) and _hr_written(hr1)
    assert not torch.equal(hr0, hr1) or not torch.equal(a0, a1), "the option changed nothing: the new kernel did not run"
    e0, e1 = three.errors(a0, c0, True, slice(0, 1)), three.errors(a1, c1, True, slice(0, 1))
    print(f"M = 1, P = 128: max |error| vs float64, g1 kernel pred*conf {e0[0]:.3g} conf {e0[1]:.3g} | tap kernel pred*conf {e1[0]:.3g} conf {e1[1]:.3g}")
    assert e1[0] <= 1.5 * e0[0] and e1[1] <= 1.5 * e0[1], (e0, e1)


@pytest.mark.parametrize("confidence", [True, False], ids=["confidence", "plain"])
def test_three_images_against_float64_within_the_g1_kernels_error(three, confidence):
    """M = 3 (Normal, small values, corners and edge midpoints only), confidence on and off, out_c NULL and not"""
    a0, c0, _ = three.run(0, confidence)
    a1, c1, hr1 = three.run(1, confidence)
    assert _hr_written(hr1)
    e0, e1 = three.errors(a0, c0, confidence), three.errors(a1, c1, confidence)
    print(f"M = 3, P = 128, confidence {confidence}: max |error| vs float64, g1 kernel out_a {e0[0]:.3g} out_c {e0[1]:.3g} | tap kernel out_a {e1[0]:.3g} out_c {e1[1]:.3g}")
    for m in range(3):
        em0, em1 = three.errors(a0[m:m + 1], c0[m:m + 1], confidence, slice(m, m + 1)), three.errors(a1[m:m + 1], c1[m:m + 1], confidence, slice(m, m + 1))
        print(f"  image {m}: g1 kernel {em0[0]:.3g} {em0[1]:.3g} | tap kernel {em1[0]:.3g} {em1[1]:.3g}")
    assert e1[0] <= 1.5 * e0[0] and e1[1] <= 1.5 * e0[1], (e0, e1)
    a2, c2, _ = three.run(1, confidence, with_c=False)
    assert c2 is None and torch.equal(a2, a1)


def test_other_patch_sizes_take_the_g1_kernel():
    """M = 2, P = 64: outputs and scratch are the g1 kernel's whatever the option says"""
    case = _Case(2, 64)
    a0, c0, hr0 = case.run(0, True)
    a1, c1, hr1 = case.run(1, True)
    assert torch.equal(a0, a1) and torch.equal(c0, c1)
    assert torch.equal(torch.nan_to_num(hr0, nan=-7.0), torch.nan_to_num(hr1, nan=-7.0))
    e = case.errors(a0, c0, True)
    assert e[0] < 3e-5 and e[1] < 3e-5


def test_deterministic_batch_independent_and_in_range(three):
    """two calls give the same bits; image m alone has the bits it has in the batch of three; the sticky range flag stays down"""
    lib = three.lib
    flag = ctypes.c_int(-1)
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1) == 0                       # clear
    a, c, hr = three.run(1, True)
    a2, c2, hr2 = three.run(1, True)
    assert torch.equal(a, a2) and torch.equal(c, c2) and torch.equal(torch.nan_to_num(hr, nan=-7.0), torch.nan_to_num(hr2, nan=-7.0))
    for m in range(3):
        am, cm, _ = three.run(1, True, images=slice(m, m + 1))
        assert torch.equal(am[0], a[m]) and torch.equal(cm[0], c[m]), m
    assert lib.omni_sh_overflow(ctypes.byref(flag), 0) == 0 and flag.value == 0


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def net_and_inputs():
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    rgb = torch.rand((3, 3, 128, 256), generator=torch.Generator().manual_seed(31)).to(DEV)
    return net, rgb, rgb[:1].contiguous()


def test_model_agrees_between_the_kernels_and_keeps_its_bits(net_and_inputs):
    """single-pass model on 3 panoramas and on a lone one, option 1 against 0: max |d depth| < 2e-5 (what DESIGN section 5 grants the fused heads against
    the two-kernel form); bit-reproducible across two runs and across pipelined(3) against plain calls"""
    net, rgb, one = net_and_inputs
    with _Option(0):
        ref, ref1 = net(rgb, confidence=True).clone(), net(one, confidence=True).clone()
    with _Option(1):
        out, out1 = net(rgb, confidence=True).clone(), net(one, confidence=True).clone()
        again = net(rgb, confidence=True).clone()
        run = net.pipelined(3)
        pend = [run(rgb, confidence=True) for _ in range(3)]
        piped = [p.get().clone() for p in pend]
    d, d1 = (out - ref).abs().max().item(), (out1 - ref1).abs().max().item()
    print(f"conv_up2_heads_taps 1 against 0: max |d depth| 3 panoramas {d:.3g}, lone panorama {d1:.3g}")
    assert max(d, d1) > 0, "the option changed nothing: the new kernel did not run"
    assert max(d, d1) < 2e-5, (d, d1)
    assert torch.equal(again, out)
    for p in piped:
        assert torch.equal(p, out)
