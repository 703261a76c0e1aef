"""The two geometry terms of the reference's depth objective (train_erp_depth.py:267-275, train_erp_depth_iterative.py:271-279):

    loss = berhu + 0.2 * normal_loss + 0.05 * grad_loss

    normal_loss, grad_loss = geometry_terms(pred, gt, mask)              # two 0-d float32 tensors on the device, differentiable w.r.t. pred
    normal_loss = 1 - mean_b(sum_b(depth2normal_gpu(pred) * depth2normal_gpu(gt) * mask) / mask.sum())        # the mask sum of the whole BATCH
    grad_loss   = calculate_l1_loss(imgrad_yx(pred), imgrad_yx(gt), mask)

pred, gt, mask are [B,1,H,W], H, W >= 2.  Everything numeric runs in libomnifusion_hip.so (csrc/omni_normals.hip): ONE tiled pass
over pred, gt and mask gives both terms (no normal or Sobel map is written) and ONE gather kernel gives the gradient of any weighted sum of the
two; nothing is copied to the host.  normal_loss(...) and gradient_loss(...) are the same entry with one term switched off — the kernels skip
that term's arithmetic and return the same bits for the other.

erode_mask=True replaces the mask by mask * [mask != 0 at all eight neighbours] (neighbours outside the image count as valid), in the same
kernels.  The loaders zero the ground truth where it is invalid; a normal next to such a hole is the normalised sum of four nearly cancelling
unit vectors — rounding noise — so real, holey data wants erode_mask=True.  The default is the reference's formula.

planefit_normal_loss(pred, gt, mask) is normal_loss's formula over the plane-fit normals of equi_pers.depth2normal (25 vertices per pixel, least squares
in float64; csrc/omni_planefit.hip): one 0-d float32 tensor, H, W >= 1, the same masks and the same erode_mask.

Masks may be bool, uint8 or float (multiplied in by value); non-contiguous inputs are made contiguous, as calculate_berhu_loss does.  A batch
whose mask sum is 0 gives a NaN normal_loss, an item whose mask sum is 0 a NaN grad_loss (0 / 0, as calculate_berhu_loss), with NaN gradients
for the items concerned.
"""
import torch

from .. import _lib
from .._lib import ptr as _p
from ..spherical.grid import ray_tables

NORMAL, GRADIENT = 1, 2


class _GeometryTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, tab, terms, erode):
        lib = _lib.load()
        B, _, H, W = pred.shape
        ws = torch.empty(lib.omni_geometry_terms_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.float64, device=pred.device)
        losses = torch.empty(2, dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_geometry_terms_f32(_p(pred), _p(gt), _p(mask), _p(tab), B, H, W, terms, erode, _p(ws), _p(losses),
                                                   _lib.stream_of(pred)), "geometry_terms")
        ctx.save_for_backward(pred, gt, mask, tab, ws)
        ctx.conf = (terms, erode)
        ctx.set_materialize_grads(False)                 # an output nobody used arrives as None: its term is then not computed
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, grad_normal, grad_grad):
        pred, gt, mask, tab, ws = ctx.saved_tensors
        terms, erode = ctx.conf
        if not terms & NORMAL:
            grad_normal = None
        if not terms & GRADIENT:
            grad_grad = None
        if grad_normal is None and grad_grad is None:
            return None, None, None, None, None, None
        lib = _lib.load()
        B, _, H, W = pred.shape
        gn, gg = (None if g is None else g.contiguous().to(torch.float32) for g in (grad_normal, grad_grad))
        grad = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_geometry_terms_grad_f32(_p(pred), _p(gt), _p(mask), _p(tab), B, H, W, erode, _p(ws), _p(gn), _p(gg), _p(grad),
                                                        _lib.stream_of(pred)), "geometry_terms backward")
        return grad, None, None, None, None, None


class _PlanefitLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask, tab, erode):
        lib = _lib.load()
        B, _, H, W = pred.shape
        ws = torch.empty(lib.omni_planefit_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_planefit_loss_f32(_p(pred), _p(gt), _p(mask), _p(tab), B, H, W, erode, _p(ws), _p(loss), _lib.stream_of(pred)),
                       "planefit_normal_loss")
        ctx.save_for_backward(pred, gt, mask, tab, ws)
        ctx.erode = erode
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, gt, mask, tab, ws = ctx.saved_tensors
        lib = _lib.load()
        B, _, H, W = pred.shape
        go = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.omni_planefit_loss_grad_f32(_p(pred), _p(gt), _p(mask), _p(tab), B, H, W, ctx.erode, _p(ws), _p(go), _p(grad),
                                                       _lib.stream_of(pred)), "planefit_normal_loss backward")
        return grad, None, None, None, None


def _checked(pred, gt, mask):
    """The argument checks of every entry here -> (pred, gt, mask) contiguous float32."""
    for t, name in ((pred, "pred"), (gt, "gt"), (mask, "mask")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if gt.requires_grad or mask.requires_grad:
        raise ValueError("the geometry terms are differentiable w.r.t. pred only: gt and mask must not require grad")
    for t, name in ((pred, "pred"), (gt, "gt"), (mask, "mask")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.numel() == 0:
        raise ValueError(f"pred must be a non-empty [B,1,H,W] tensor (got shape {tuple(pred.shape)})")
    if gt.shape != pred.shape or mask.shape != pred.shape:
        raise ValueError(f"pred, gt and mask must have the same shape [B,1,H,W] (got {tuple(pred.shape)}, {tuple(gt.shape)}, {tuple(mask.shape)})")
    if gt.device != pred.device or mask.device != pred.device:
        raise ValueError("pred, gt and mask must live on the same device")
    if not pred.is_floating_point() or not gt.is_floating_point():
        raise ValueError("pred and gt must be floating-point tensors")
    f = lambda t: t.contiguous().to(torch.float32)
    return f(pred), f(gt), f(mask)


def _run(pred, gt, mask, erode_mask, terms):
    pred, gt, mask = _checked(pred, gt, mask)
    H, W = pred.shape[2:]
    return _GeometryTerms.apply(pred, gt, mask, ray_tables(H, W, pred.device), terms, 1 if erode_mask else 0)


def geometry_terms(pred, gt, mask, erode_mask=False):
    """-> (normal_loss, grad_loss) from one forward pass; one backward launch consumes both upstream scalars."""
    return _run(pred, gt, mask, erode_mask, NORMAL | GRADIENT)


def normal_loss(pred, gt, mask, erode_mask=False):
    """geometry_terms(...)[0], bit for bit, without the Sobel arithmetic."""
    return _run(pred, gt, mask, erode_mask, NORMAL)[0]


def gradient_loss(pred, gt, mask, erode_mask=False):
    """geometry_terms(...)[1], bit for bit, without the normals."""
    return _run(pred, gt, mask, erode_mask, GRADIENT)[1]


def planefit_normal_loss(pred, gt, mask, erode_mask=False):
    """normal_loss's formula over the plane-fit normals of equi_pers.depth2normal (25 vertices per pixel, least squares in float64; csrc/omni_planefit.hip,
    DESIGN.md §18) instead of the four cross products: the normals one wants on real, noisy depth.  Any H, W >= 1; neither normal map is written."""
    pred, gt, mask = _checked(pred, gt, mask)
    H, W = pred.shape[2:]
    return _PlanefitLoss.apply(pred, gt, mask, ray_tables(H, W, pred.device), 1 if erode_mask else 0)
