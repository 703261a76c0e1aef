"""Host side of the decoder stages that multiply before up-sampling (Engine.taps_first): the float64 restatement the GPU tests compare
with, the tap-major weight operand, and the entry point's declaration.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, tap_products, tap_sum, taps_repack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (2, 3), (4, 4), (8, 8)])
def test_tap_restatement_equals_conv_of_upsampled(hw):
    """conv3x3(up2(x)) = sum over the taps of the shifted, up-sampled 1x1 products: both operators are linear, clamped source indices and
    zero padding included — float64, <= 1e-12."""
    g = torch.Generator().manual_seed(3)
    M, C, Co = 2, 32, 8
    x = torch.randn(M, hw[0], hw[1], C, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64) / np.sqrt(9 * C)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    for relu in (False, True):
        d = (tap_sum(tap_products(x, w), b, relu) - direct(x, w, b, relu)).abs().max().item()
        assert d <= 1e-12, (hw, relu, d)


def test_pack_makes_the_tap_major_operand():
    """Engine.pack: `<name>.taps.w16` holds the folded weights with W[co][t][ci] at row t*Cout + co, in the split operand format."""
    from omnifusion_amd.model._engine import Engine
    from omnifusion_amd.weights import make_state_dict
    sd = make_state_dict(42, 18, False)
    eng = Engine(4, 18, (128, 128), (80, 80), False)
    eng.pack(sd, "cpu")
    for name, cin, cout in (("de_conv0_0", 512, 256), ("de_conv1_0", 128, 128)):
        w16 = eng.w[name + ".taps.w16"]
        assert w16.dtype == torch.float16 and tuple(w16.shape) == (9 * cout, cin // 32, 2, 32)
        joined = (w16[:, :, 0].double() + w16[:, :, 1].double() / 2048.0).reshape(9 * cout, cin)
        w, _ = Engine._fold({k: v for k, v in sd.items()}, name + ".conv", name + ".bn")
        assert (joined - taps_repack(w)).abs().max().item() <= 2.0 ** -21 * w.abs().max().item()
        for t, co in ((0, 0), (4, 7), (8, cout - 1)):                                    # the row order, spelled out
            assert (joined[t * cout + co] - w[co, :, t // 3, t % 3]).abs().max().item() <= 2.0 ** -21 * w.abs().max().item()
        for k in (".w16", ".w", ".b"):                                                   # the other modes and the fallback keep theirs
            assert (name + k) in eng.w
    assert not any(k.endswith(".taps.w16") for k in eng.w if not k.startswith(("de_conv0_0", "de_conv1_0")))


def test_tapsum_entry_point_is_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "omnifusion.h")).read()
    assert re.search(r"^int omni_up2_tapsum_sh\(const float\* y, const float\* bias, void\* dst, int M, int Hl, int Wl, int Cout, int act, omni_stream_t stream\);",
                     header, re.M)
    assert "omni_up2_tapsum_sh" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "omni_up2_tapsum_sh") and L.omni_version() == 200
    assert L.omni_up2_tapsum_sh(None, None, None, 1, 4, 4, 32, 0, None) == _lib.OMNI_ERR_INVALID       # argument checks run before any launch
    assert b"omni_up2_tapsum_sh" in L.omni_last_error()
