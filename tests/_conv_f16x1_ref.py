"""The rounding model of the f16x1 convolution, shared by the f16x1 tests: an operand is hi16(x) — fp16(x) rounded to
nearest even, 0 where |x| < 2^-14 — products are exact (two halfs multiply exactly in fp32) and sums are float64 here, fp32 on the device.
The backward's operands are hi16(dZ . 2^s) . 2^-s with s = 8 - floor(log2 max|dZ|), the scale rule of the gradient epilogue (§19)."""
import math

import torch
import torch.nn.functional as F

HI_MIN = 2.0 ** -14


def hi16(t):
    """fp16(t), round to nearest even, 0 below the fp16 normal range; returned in t's dtype.  t holds float32 values on the device, so a
    float64 t goes through float32 first (a no-op for values that are float32 already)."""
    h = t.detach().to(torch.float32).to(torch.float16).to(t.dtype)
    return torch.where(t.detach().abs() < HI_MIN, torch.zeros_like(h), h)


class _HiST(torch.autograd.Function):
    """hi16 forward, identity backward (straight through): the device rounds operands, never gradients of operands"""

    @staticmethod
    def forward(ctx, t):
        return hi16(t)

    @staticmethod
    def backward(ctx, g):
        return g


def hi16_st(t):
    return _HiST.apply(t)


def scale_exp(dz):
    """s of the gradient epilogue: 8 - floor(log2 max|dZ|) clamped to [-126, 126]; 0 where dZ is all zero or its maximum is not finite"""
    m = dz.detach().abs().max().item()
    if m == 0.0 or not math.isfinite(m):
        return 0
    return max(-126, min(126, 8 - math.frexp(m)[1] + 1))


def hi16_scaled(dz):
    """hi16(dZ . 2^s) . 2^-s: the backward's gradient operand"""
    s = scale_exp(dz)
    return hi16(dz * 2.0 ** s) * 2.0 ** -s


def conv64(x, w, b=None, stride=1, padding=0):
    """float64 F.conv2d over hi16 operands (the bias is not an operand of a product: unrounded)"""
    return F.conv2d(hi16(x.double()), hi16(w.double()), None if b is None else b.double(), stride, padding)


def model64(d, stride, padding, act, g):
    """The whole operator in the rounding model: d = {x, x2, w, b, res} (float32, None where absent), g = grad_out.
    -> (pre-activation z, {kind: gradient}), all float64."""
    x = d["x"] if d["x2"] is None else torch.cat([d["x"], d["x2"]], 1)
    xq, wq = hi16(x.double()).requires_grad_(True), hi16(d["w"].double()).requires_grad_(True)
    zlin = F.conv2d(xq, wq, None, stride, padding)
    z = zlin.detach()
    if d["b"] is not None:
        z = z + d["b"].double()[None, :, None, None]
    if d["res"] is not None:
        z = z + d["res"].double()
    dz = g.double() * (z > 0) if act == "relu" else g.double()                 # a select on the device: exact
    dxq, dwq = torch.autograd.grad(zlin, (xq, wq), hi16_scaled(dz))
    C1 = d["x"].shape[1]
    grads = {"x": dxq[:, :C1], "x2": dxq[:, C1:] if d["x2"] is not None else None, "w": dwq,
             "b": dz.sum((0, 2, 3)) if d["b"] is not None else None, "res": dz if d["res"] is not None else None}
    return z, grads
