"""Differentiable operators of libomnifusion_hip.so for torch models: the network's convolution with its backward.

    y = conv2d(x, weight, bias=None, *, x2=None, res=None, stride=1, padding=0, act="none" | "relu")
    layer = Conv2d(64, 64, 3, padding=1, act="relu")          # an nn.Conv2d whose forward is the call above

y = act(conv(cat(x, x2), weight) + bias + res) — the operator that is about 99 % of spherical_fusion's work (csrc/omni_conv.hip, f16x3
products on the matrix cores) — and its gradients w.r.t. x, x2, weight, bias and res (csrc/omni_conv_bwd.hip): the same
products, a fixed summation order, no atomics, no host synchronisation.  Only the gradients autograd asks for are computed.

Tensors: x [M,C1,H,W], x2 [M,C2,H,W], weight [Cout,C1+C2,k,k], res and y [M,Cout,Ho,Wo], float32 on an MI355X.  The storage of a
`torch.channels_last` tensor IS the library's NHWC (and that of a channels-last weight its [Cout][(ky,kx,c)]), so such tensors pass through
without a copy and y is channels-last; other formats are converted.  Limits: C1, C2, Cout multiples of 32 (the concat is never
materialised), k = 1 or 3, stride 1 or 2, no groups, no dilation; act "gelu" has no backward and is rejected (apply GELU outside).
No double backward.  There is no CPU path.
"""
import ctypes

import torch

from . import _lib

ACTS = {"none": 0, "relu": 1}
_empty = torch.empty          # every buffer of this module is allocated through this name (tests fill them with NaN)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nhwc(t):
    """[M,C,H,W] of any memory format -> the contiguous [M,H,W,C] tensor (a view, without a copy, where t is channels-last)"""
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2)


def _check_args(x, weight, bias, x2, res, stride, padding, act):
    """Every rejection of conv2d, raised before anything is launched.  Returns (k, Ho, Wo)."""
    for t, name, opt in ((x, "x", False), (weight, "weight", False), (bias, "bias", True), (x2, "x2", True), (res, "res", True)):
        if t is None and opt:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if act not in ACTS:
        if act == "gelu":
            raise ValueError("act='gelu' is not supported: the convolution's backward covers 'none' and 'relu' only (the forward does not "
                             "keep the pre-activation); apply GELU outside")
        raise ValueError(f"act must be 'none' or 'relu' (got {act!r})")
    if x.dim() != 4 or weight.dim() != 4 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [M,C1,H,W] tensor and weight [Cout,C1+C2,k,k] (got {tuple(x.shape)} and {tuple(weight.shape)})")
    M, C1, H, W = x.shape
    C2 = 0
    if x2 is not None:
        if x2.dim() != 4 or x2.shape[0] != M or tuple(x2.shape[2:]) != (H, W):
            raise ValueError(f"x2 must be [M,C2,H,W] with x's M, H, W (got {tuple(x2.shape)} for x {tuple(x.shape)})")
        C2 = x2.shape[1]
    Cout, Cw, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"kernel size must be 1x1 or 3x3 (got {k}x{k2})")
    if C1 % 32 or C2 % 32 or Cout % 32 or C1 == 0 or Cout == 0:
        raise ValueError(f"channel counts must be multiples of 32 (got C1 = {C1}, C2 = {C2}, Cout = {Cout})")
    if Cw != C1 + C2:
        raise ValueError(f"weight has {Cw} input channels, x and x2 have {C1} + {C2}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2 (got {stride!r})")
    if not isinstance(padding, int) or padding < 0 or H + 2 * padding < k or W + 2 * padding < k:
        raise ValueError(f"padding must be an int >= 0 that leaves room for the kernel (got {padding!r})")
    Ho, Wo = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"bias must be [Cout] = [{Cout}] (got {tuple(bias.shape)})")
    if res is not None and tuple(res.shape) != (M, Cout, Ho, Wo):
        raise ValueError(f"res must have the result's shape {(M, Cout, Ho, Wo)} (got {tuple(res.shape)})")
    return k, Ho, Wo


def _forward_nhwc(x1, x2, w, bias, res, stride, pad, act):
    """x1 [M,H,W,C1], x2 [M,H,W,C2] | None, w [Cout,k,k,C1+C2], res [M,Ho,Wo,Cout] | None, all contiguous -> y [M,Ho,Wo,Cout]"""
    lib = _lib.load()
    M, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    Cout, k = w.shape[0], w.shape[1]
    K = k * k * (C1 + C2)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    w16 = _empty(Cout * K * 2, dtype=torch.float16, device=x1.device)          # the weights change every step: split on the device
    y = _empty((M, Ho, Wo, Cout), dtype=torch.float32, device=x1.device)
    with torch.cuda.device(x1.device):
        st = _lib.stream_of(x1)
        _lib.check(lib.omni_conv2d_split_weights_f16x3(_p(w), _p(w16), Cout, K, st), "conv2d_split_weights")
        _lib.check(lib.omni_conv2d_nhwc_f16x3_ws(_p(x1), _p(x2), _p(w16), _p(bias), _p(res), _p(y), M, H, W, C1, C2, Cout, k, k, stride, pad,
                                                 ACTS[act], 1, None, ctypes.c_size_t(0), st), "conv2d")
    return y


def _backward_nhwc(g, y, x1, x2, w, stride, pad, act, need_x1, need_x2, need_w):
    """The three calls of the backward on contiguous NHWC tensors.  Returns (dx1, dx2, dw, dbias, dz); dz is the residual's gradient."""
    lib = _lib.load()
    M, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    Cout, k = w.shape[0], w.shape[1]
    dev = x1.device
    shape = (M, H, W, C1, C2, Cout, k, k, stride, pad)
    nbytes = lib.omni_conv2d_bwd_workspace_bytes(*shape)
    if nbytes == 0:
        raise ValueError(f"conv2d backward: shape {shape} is outside the operator's scope")
    ws = _empty(nbytes // 4, dtype=torch.float32, device=dev)
    scale = _empty(2, dtype=torch.float32, device=dev)
    dbias = _empty(Cout, dtype=torch.float32, device=dev)
    relu = act == "relu"
    dz = _empty(tuple(g.shape), dtype=torch.float32, device=dev) if relu else None
    dx1 = dx2 = dw = None
    with torch.cuda.device(dev):
        st = _lib.stream_of(x1)
        _lib.check(lib.omni_conv2d_bwd_epilogue_f32(_p(g), _p(y) if relu else None, _p(dz), _p(dbias), _p(scale), g.numel() // Cout, Cout,
                                                    ACTS[act], _p(ws), nbytes, st), "conv2d_bwd_epilogue")
        if not relu:
            dz = g
        if need_x1 or need_x2:
            dx1 = _empty((M, H, W, C1), dtype=torch.float32, device=dev) if need_x1 else None
            dx2 = _empty((M, H, W, C2), dtype=torch.float32, device=dev) if need_x2 else None
            _lib.check(lib.omni_conv2d_bwd_data_f16x3(_p(dz), _p(w), _p(scale), _p(dx1), _p(dx2), *shape, _p(ws), nbytes, st), "conv2d_bwd_data")
        if need_w:
            dw = _empty(tuple(w.shape), dtype=torch.float32, device=dev)
            _lib.check(lib.omni_conv2d_bwd_weight_f16x3(_p(dz), _p(x1), _p(x2), _p(scale), _p(dw), *shape, _p(ws), nbytes, st),
                       "conv2d_bwd_weight")
    return dx1, dx2, dw, dbias, dz


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, weight, bias, res, stride, padding, act):
        x1n, x2n, wn, resn = _nhwc(x), _nhwc(x2), _nhwc(weight), _nhwc(res)
        b = bias.contiguous() if bias is not None else None
        y = _forward_nhwc(x1n, x2n, wn, b, resn, stride, padding, act)
        ctx.conf = (stride, padding, act)
        ctx.save_for_backward(x1n, x2n, wn, y if act == "relu" else None)
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x1n, x2n, wn, y = ctx.saved_tensors
        stride, padding, act = ctx.conf
        need = ctx.needs_input_grad
        g = _nhwc(grad_out.to(torch.float32))
        dx1, dx2, dw, dbias, dz = _backward_nhwc(g, y, x1n, x2n, wn, stride, padding, act, need[0], x2n is not None and need[1], need[2])
        return (_nchw(dx1), _nchw(dx2), _nchw(dw), dbias if need[3] else None, _nchw(dz) if need[4] else None, None, None, None)


def conv2d(x, weight, bias=None, *, x2=None, res=None, stride=1, padding=0, act="none"):
    """act(conv(cat(x, x2), weight) + bias + res), differentiable w.r.t. x, x2, weight, bias and res (module docstring)."""
    _check_args(x, weight, bias, x2, res, stride, padding, act)
    return _Conv2d.apply(x, x2, weight, bias, res, stride, padding, act)


class Conv2d(torch.nn.Conv2d):
    """nn.Conv2d with the library's kernels under forward and backward, so that a torch model can swap its layers: the same parameters and
    state dict.  `act` ("none" | "relu") is fused; forward(x, x2=None, res=None) takes the optional second source and residual."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, act="none", **kw):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        if self.groups != 1 or tuple(self.dilation) != (1, 1) or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise ValueError("ops.Conv2d: no groups, no dilation, zero padding given as a number")
        if self.kernel_size[0] != self.kernel_size[1] or self.stride[0] != self.stride[1] or self.padding[0] != self.padding[1]:
            raise ValueError("ops.Conv2d: square kernels, one stride and one padding for both axes")
        if act not in ACTS:
            raise ValueError(f"ops.Conv2d: act must be 'none' or 'relu' (got {act!r}; GELU has no backward here)")
        self.act = act

    def forward(self, x, x2=None, res=None):
        return conv2d(x, self.weight, self.bias, x2=x2, res=res, stride=self.stride[0], padding=self.padding[0], act=self.act)
