"""calculate_berhu_loss — host-side mirror of /root/reference/supervision/direct.py:3-18 (used at train_erp_depth.py:267).

    loss = calculate_berhu_loss(pred, gt, mask, weights)      # scalar tensor on pred.device, differentiable w.r.t. pred

Same name, arguments and value as the reference.  Everything numeric runs in libomnifusion_hip.so (csrc/omni_losses.hip): a max
pass, a deterministic two-stage masked sum and — for backward — one element-wise gradient pass.  Unlike the reference
(`torch.max(abs_diff).item()`, a device->host synchronisation per step) the threshold c = max|gt - pred| / 5 stays on the device;
like there it is a constant of the backward pass.

calculate_l1_loss — mirror of :20-26 (the gradient term of the depth objective, train_erp_depth.py:272-274; the same unit):

    loss = calculate_l1_loss(pred, gt, mask)                  # mean_b(sum_b(|gt - pred| * mask) / sum_b(mask)), differentiable w.r.t. pred
"""
import torch

from .. import _lib
from .._lib import ptr as _p


class _BerHu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, weights):
        lib = _lib.load()
        B = pred.shape[0]
        per = pred.numel() // B
        ws = torch.empty(lib.omni_berhu_workspace_bytes(B) // 4 + 1, dtype=torch.int32, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_berhu_loss_f32(_p(pred), _p(gt), _p(mask), _p(weights), B, per, _p(ws), _p(loss),
                                               _lib.stream_of(pred)), "berhu_loss")
        ctx.save_for_backward(pred, gt, mask, weights, ws)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, gt, mask, weights, ws = ctx.saved_tensors
        lib = _lib.load()
        B = pred.shape[0]
        per = pred.numel() // B
        g = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_berhu_grad_f32(_p(pred), _p(gt), _p(mask), _p(weights), B, per, _p(ws), _p(g), _p(grad),
                                               _lib.stream_of(pred)), "berhu_grad")
        return grad, None, None, None


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask):
        lib = _lib.load()
        B, C = pred.shape[0], pred.shape[1]
        hw = pred.numel() // (B * C)
        ws = torch.empty(lib.omni_l1_workspace_bytes(B) // 8 + 1, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_l1_loss_f32(_p(pred), _p(gt), _p(mask), B, C, hw, mask.shape[1], _p(ws), _p(loss), _lib.stream_of(pred)), "l1_loss")
        ctx.save_for_backward(pred, gt, mask, ws)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, gt, mask, ws = ctx.saved_tensors
        lib = _lib.load()
        B, C = pred.shape[0], pred.shape[1]
        hw = pred.numel() // (B * C)
        g = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_l1_grad_f32(_p(pred), _p(gt), _p(mask), B, C, hw, mask.shape[1], _p(ws), _p(g), _p(grad), _lib.stream_of(pred)), "l1_grad")
        return grad, None, None


def calculate_l1_loss(pred, gt, mask):
    """Mirror of the reference's supervision/direct.py:20-26 for [B,C,H,W] inputs: mean_b(sum_b(|gt - pred| * mask) / count_b), a 0-d float32
    tensor on the device, differentiable w.r.t. pred (d|x|/dx = 0 at 0).  mask is [B,1,H,W] or [B,C,H,W] (bool, uint8 or float: multiplied in by
    value); count_b is the sum of the mask as it is given, not multiplied by C.  An item whose mask sum is 0 makes the loss NaN, as BerHu."""
    for t, name in ((pred, "pred"), (gt, "gt"), (mask, "mask")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if pred.dim() != 4 or pred.numel() == 0 or pred.shape != gt.shape:
        raise ValueError(f"pred and gt must be non-empty [B,C,H,W] tensors of one shape (got {tuple(pred.shape)} and {tuple(gt.shape)})")
    B, C, H, W = pred.shape
    if mask.dim() != 4 or tuple(mask.shape) not in ((B, 1, H, W), (B, C, H, W)):
        raise ValueError(f"mask must be [B,1,H,W] or [B,C,H,W] (got {tuple(mask.shape)} for pred {tuple(pred.shape)})")
    if gt.requires_grad or mask.requires_grad:
        raise ValueError("calculate_l1_loss is differentiable w.r.t. pred only: gt and mask must not require grad")
    f = lambda t: t.contiguous().to(torch.float32)
    return _L1.apply(f(pred), f(gt), f(mask))


def calculate_berhu_loss(pred, gt, mask, weights):
    """Mirror of the reference's supervision/direct.py:3-18: mean_b(sum_b(berhu(gt - pred) * mask * weights) / sum_b(mask)) with the threshold
    c = max|gt - pred| / 5 over EVERY element (masked-out ones and other batch items included), a 0-d float32 tensor, differentiable w.r.t. pred.
    |d| <= c is decided in float32 and takes the linear branch (gradient sign(d), 0 at d = 0).  An item whose mask sum is 0 makes the loss NaN
    (0 / 0) and its own gradient NaN; the other items' gradients stay finite.  One deliberate difference: where pred == gt everywhere, c is 0 and
    the reference evaluates (d^2 + c^2) / (2 c) = 0 / 0 for every element and returns NaN; here every element takes the linear branch, the loss
    is 0 and the gradient 0."""
    for t, name in ((pred, "pred"), (gt, "gt"), (mask, "mask"), (weights, "weights")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if pred.shape != gt.shape or pred.numel() != mask.numel() or pred.numel() != weights.numel():
        raise ValueError("pred, gt, mask and weights must have the same number of elements")
    if pred.shape[0] < 1 or pred.numel() == 0:
        raise ValueError("empty batch")
    f = lambda t: t.contiguous().to(torch.float32)
    return _BerHu.apply(f(pred), f(gt).detach(), f(mask).detach(), f(weights).detach())
