"""calculate_loss — host-side mirror of the reference's supervision/photometric.py (the photometric loss of view synthesis).

    params = PhotometricLossParameters(alpha=0.85, window=7, std=1.5, ssim_mode='gaussian')
    loss = calculate_loss(pred, gt, params, mask, weights)       # scalar tensor on pred.device, differentiable w.r.t. pred

Same names, arguments and values as the reference: pred and gt are multiplied by the mask, d_ssim = clamp((1 - ssim) / 2, 0, 1),
loss = (alpha d_ssim + (1 - alpha) |gt - pred|) * mask * weights, summed per item over C,H,W, divided by the item's sum(mask) — counted
on the mask as given, [B,1,H,W] or [B,C,H,W] — and averaged over the batch.  Everything numeric runs in libomnifusion_hip.so
(csrc/omni_photometric.hip): one tiled forward kernel that writes no map, a deterministic two-stage sum (the scalar stays on the
device), and for backward two tiled passes.  gt, mask and weights are constants of the backward, as in calculate_berhu_loss.
"""
import torch

from .. import _lib
from .ssim import _p, check_pair, ssim_loss, window_weights  # noqa: F401  (the reference's `from .ssim import *`)


class PhotometricLossParameters(object):
    def __init__(self, alpha=0.85, l1_estimator='none', ssim_estimator='none', window=7, std=1.5, ssim_mode='gaussian'):
        super(PhotometricLossParameters, self).__init__()
        self.alpha = alpha
        self.l1_estimator = l1_estimator
        self.ssim_estimator = ssim_estimator
        self.window = window
        self.std = std
        self.ssim_mode = ssim_mode

    def get_alpha(self):
        return self.alpha

    def get_l1_estimator(self):
        return self.l1_estimator

    def get_ssim_estimator(self):
        return self.ssim_estimator

    def get_window(self):
        return self.window

    def get_std(self):
        return self.std

    def get_ssim_mode(self):
        return self.ssim_mode


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, weights, window, win, code, alpha):
        lib = _lib.load()
        B, C, H, W = pred.shape
        ws = torch.empty(lib.omni_photometric_workspace_bytes(B, C, H, W) // 8 + 1, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_photometric_loss_f32(_p(pred), _p(gt), _p(mask), mask.shape[1], _p(weights), weights.shape[1], B, C, H, W,
                                                     window, win, code, alpha, _p(ws), _p(loss), _lib.stream_of(pred)), "photometric loss")
        ctx.save_for_backward(pred, gt, mask, weights, ws)
        ctx.conf = (window, win, code, alpha)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, gt, mask, weights, ws = ctx.saved_tensors
        window, win, code, alpha = ctx.conf
        lib = _lib.load()
        B, C, H, W = pred.shape
        g = grad_out.contiguous().to(torch.float32)
        scratch = torch.empty(lib.omni_photometric_grad_scratch_bytes(B, C, H, W) // 4, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_photometric_grad_f32(_p(pred), _p(gt), _p(mask), mask.shape[1], _p(weights), weights.shape[1], B, C, H, W,
                                                     window, win, code, alpha, _p(ws), _p(scratch), _p(g), _p(grad), _lib.stream_of(pred)),
                       "photometric grad")
        return grad, None, None, None, None, None, None, None


def _plane(name, t, B, C, H, W, device):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dim() != 4 or t.shape[0] != B or t.shape[1] not in (1, C) or tuple(t.shape[2:]) != (H, W):
        raise ValueError(f"{name} must be [B,1,H,W] or [B,C,H,W] with (B,C,H,W) = {(B, C, H, W)} (got {tuple(t.shape)})")
    if t.device != device:
        raise ValueError(f"{name} must live on pred's device")
    return t.detach().to(torch.float32).contiguous()


def calculate_loss(pred, gt, params, mask, weights):
    win, code = window_weights(params.get_window(), params.get_std(), params.get_ssim_mode())
    B, C, H, W = check_pair(pred, gt, names=("pred", "gt"))
    mask = _plane("mask", mask, B, C, H, W, pred.device)
    weights = _plane("weights", weights, B, C, H, W, pred.device)
    if code == 1 and (H < params.get_window() or W < params.get_window()):
        raise ValueError("the box window does not fit the image")
    return _Photometric.apply(pred.contiguous(), gt.detach().contiguous(), mask, weights, int(params.get_window()), win, code,
                              float(params.get_alpha()))
