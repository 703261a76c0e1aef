"""CPU: ops.point_conv / ops.PointConv2d (csrc/omni_point_conv.hip) as far as they go without a device — every rejection of
the Python layer (raised before anything is launched, shapes before devices so that they can be met here), the host-side rejections and
the workspace plan of the C entry points, and the three new prototypes in the boundary's signature table."""
import ctypes

import numpy as np
import pytest
import torch

from omnifusion_amd import _lib, build, ops


def _w(cout, cin):
    return torch.zeros(cout, cin, 1, 1)


@pytest.mark.parametrize("cout,cin", [(16, 4), (32, 3), (64, 5), (16, 16), (64, 32), (3, 16)])
def test_wrong_channel_pairs_are_rejected(cout, cin):
    with pytest.raises(ValueError, match="the only ones built"):
        ops.point_conv(torch.zeros(2, cin, 4, 4), _w(cout, cin))
    with pytest.raises(ValueError, match="the only ones built"):
        ops.PointConv2d(cin, cout, 1, bias=False)


def test_shape_rejections():
    with pytest.raises(ValueError, match="the only ones built"):
        ops.point_conv(torch.zeros(2, 3, 4, 4), torch.zeros(16, 3, 3, 3))                       # not 1x1
    with pytest.raises(ValueError, match=r"\[Mx,3,h,w\]"):
        ops.point_conv(torch.zeros(2, 5, 4, 4), _w(16, 3))                                      # x's channels against the weight's
    with pytest.raises(ValueError, match=r"\[Mx,16,h,w\]"):
        ops.point_conv(torch.zeros(0, 16, 4, 4), _w(64, 16))                                    # empty
    with pytest.raises(ValueError, match="multiple of x's 2 items"):
        ops.point_conv(torch.zeros(2, 3, 4, 4), _w(16, 3), scale=torch.zeros(5, 1, 4, 4))       # M = 5 is no multiple of Mx = 2
    with pytest.raises(ValueError, match="multiple of x's 2 items"):
        ops.point_conv(torch.zeros(2, 3, 4, 4), _w(16, 3), scale=torch.zeros(4, 1, 4, 5))       # another map size
    with pytest.raises(ValueError, match="multiple of x's 2 items"):
        ops.point_conv(torch.zeros(2, 3, 4, 4), _w(16, 3), scale=torch.zeros(4, 3, 4, 4))       # one value per channel
    with pytest.raises(ValueError, match="only the 3 -> 16 form takes a scale"):
        ops.point_conv(torch.zeros(2, 5, 4, 4), _w(16, 5), scale=torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError, match="only the 3 -> 16 form takes a scale"):
        ops.point_conv(torch.zeros(2, 16, 4, 4), _w(64, 16), scale=torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError, match="bias"):
        ops.PointConv2d(3, 16, 1, bias=True)
    with pytest.raises(ValueError, match="stride 1"):
        ops.PointConv2d(3, 16, 1, stride=2, bias=False)


def test_a_broadcast_x_that_requires_grad_is_not_implemented():
    for cin in (3, 5):
        with pytest.raises(NotImplementedError, match="constants"):
            ops.point_conv(torch.zeros(2, cin, 4, 4, requires_grad=True), _w(16, cin))
    with pytest.raises(NotImplementedError, match="constants"):
        ops.point_conv(torch.zeros(2, 3, 4, 4, requires_grad=True), _w(16, 3), scale=torch.zeros(6, 1, 4, 4))
    with torch.no_grad(), pytest.raises(ValueError, match="no CPU path"):                       # no graph is recorded: the device check is next
        ops.point_conv(torch.zeros(2, 3, 4, 4, requires_grad=True), _w(16, 3))


def test_cpu_tensors_and_float64_are_rejected():
    with pytest.raises(ValueError, match="no CPU path"):
        ops.point_conv(torch.zeros(2, 3, 4, 4), _w(16, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.point_conv(torch.zeros(2, 16, 4, 4, requires_grad=True), _w(64, 16))                # the 16 -> 64 form has a dx: only the device is missing
    with pytest.raises(ValueError, match="no CPU path"):
        ops.PointConv2d(3, 16, 1, bias=False)(torch.zeros(2, 3, 4, 4), scale=torch.zeros(4, 1, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        ops.point_conv(torch.zeros(2, 3, 4, 4, dtype=torch.float64), _w(16, 3).double())
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.point_conv(np.zeros((2, 3, 4, 4), np.float32), _w(16, 3))


def test_the_layer_holds_the_reference_parameter():
    for cin, cout in ((3, 16), (5, 16), (16, 64)):
        m = ops.PointConv2d(cin, cout, kernel_size=1, stride=1, padding=0, bias=False)
        assert isinstance(m, torch.nn.Conv2d) and list(m.state_dict()) == ["weight"] and tuple(m.weight.shape) == (cout, cin, 1, 1)
        assert m.bias is None and m.weight.requires_grad


def test_entry_points_in_the_signature_table_and_host_side_rejections():
    import test_boundary
    test_boundary.test_signature_table_matches_header()                                         # the table check, the new prototypes included
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SIGNATURES["omni_point_conv_fwd_f32"] == (ci, (vp,) * 4 + (ci,) * 5 + (vp,))
    assert _lib.SIGNATURES["omni_point_conv_bwd_workspace_bytes"] == (sz, (ci,) * 4)
    assert _lib.SIGNATURES["omni_point_conv_bwd_f32"] == (ci, (vp,) * 7 + (ci,) * 5 + (vp, sz, vp))
    assert _lib.EXPORTS[-3:] == ["omni_point_conv_fwd_f32", "omni_point_conv_bwd_workspace_bytes", "omni_point_conv_bwd_f32"]
    build.build()
    L = _lib.load()
    # the plan: 64-row tiles, at least 5 to a chunk, at most 1024 chunks; one partial [Cout . Cin] per chunk
    ws = L.omni_point_conv_bwd_workspace_bytes
    assert ws(1, 1, 3, 16) == 48 * 4 and ws(36, 1024, 3, 16) == 116 * 48 * 4 and ws(144, 1024, 16, 64) == 461 * 1024 * 4
    assert ws(10, 16, 5, 16) == 80 * 4 and ws(1024, 1024, 16, 64) == 1024 * 1024 * 4
    assert ws(1, 1, 4, 16) == 0 and ws(1, 1, 16, 16) == 0 and ws(0, 4, 3, 16) == 0 and ws(1 << 16, 1 << 15, 3, 16) == 0
    # every rejection happens before a launch, so the host answers without a device; the pointers are never read
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(vp)
    fwd, bwd = L.omni_point_conv_fwd_f32, L.omni_point_conv_bwd_f32
    assert fwd(None, p, None, p, 1, 1, 1, 3, 16, None) == _lib.OMNI_ERR_INVALID
    assert fwd(p, p, None, p, 1, 1, 1, 4, 16, None) == _lib.OMNI_ERR_UNSUPPORTED and b"3 -> 16" in L.omni_last_error()
    assert fwd(p, p, None, p, 1, 1, 1, 5, 64, None) == _lib.OMNI_ERR_UNSUPPORTED
    assert fwd(p, p, p, p, 2, 5, 4, 3, 16, None) == _lib.OMNI_ERR_INVALID and b"multiple of Mx" in L.omni_last_error()
    assert fwd(p, p, p, p, 2, 2, 4, 5, 16, None) == _lib.OMNI_ERR_UNSUPPORTED                   # a scale on the 5 -> 16 form
    assert fwd(p, p, None, p, 2, 4, 4, 16, 64, None) == _lib.OMNI_ERR_UNSUPPORTED               # a broadcast on the 16 -> 64 form
    assert fwd(p, p, None, p, 1, 1 << 16, 1 << 15, 3, 16, None) == _lib.OMNI_ERR_UNSUPPORTED    # 2^31 rows
    assert bwd(p, p, p, None, None, None, None, 1, 1, 1, 3, 16, None, 0, None) == _lib.OMNI_ERR_INVALID       # nothing asked for
    assert bwd(p, p, p, None, p, None, None, 1, 1, 1, 3, 16, None, 0, None) == _lib.OMNI_ERR_UNSUPPORTED      # dx of a planar form
    assert bwd(p, p, p, None, None, None, p, 1, 1, 1, 3, 16, None, 0, None) == _lib.OMNI_ERR_INVALID          # dscale without a scale
    assert bwd(p, p, p, None, None, p, None, 1, 1, 1, 3, 16, p, 48 * 4 - 1, None) == _lib.OMNI_ERR_INVALID and b"workspace" in L.omni_last_error()
