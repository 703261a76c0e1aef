"""Differentiable free-view sampling: the operators of equi2pers_torch / pers2equi_torch / views_to_erp with a backward on the device.

    from omnifusion_amd.equi_pers import differentiable as fv
    pers       = fv.equi2pers(equi_img, hFOV, wFOV, theta, phi, h, w)          # [B,C,h,N*w]; grad -> equi_img
    pers       = fv.equi2pers_planar(equi_img, hFOV, wFOV, theta, phi, h, w)   # [B,N,C,h,w]
    erp, mask  = fv.pers2equi(pers_img, hFOV, wFOV, theta, phi, H, W)          # grad -> pers_img; mask non-differentiable
    erp, count = fv.views_to_erp(pers, hFOV, wFOV, theta, phi, H, W)           # grad -> pers; count non-differentiable

Same names, signatures, values (bit for bit: the same launches) and argument errors as the plain mirrors, which keep refusing an input
that requires grad.  Without such an input these functions ARE the plain mirrors and save nothing.  The operators are linear in the
image, so a backward is the transpose of the forward's gather: csrc/omni_freeview_bwd.hip scatters w_k * g through the forward's own
tap set and sums in 64-bit fixed point (DESIGN.md §12 "Backward"): the gradient bits do not depend on the order of arrival, on the batch
split or on a graph replay.  A non-finite upstream value makes NaN exactly the gradient elements it reaches (§7 d11).

No gradient with respect to theta / phi / the fields of view (NotImplementedError if an angle requires grad), no double backward.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import _freeview
from . import equi2pers_torch as _e2p
from . import pers2equi_torch as _p2e


def _wants_grad(t):
    return isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled()


def _upstream(g):
    return g.contiguous().to(torch.float32)


class _Equi2Pers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, equi_img, hFOV, wFOV, theta, phi, h, w, layout):
        pers = _freeview.launch_equi2pers(equi_img, hFOV, wFOV, theta, phi, h, w, layout, allow_grad=True)
        hFOV, wFOV, h, w = _freeview.check_view(hFOV, wFOV, h, w)
        ctx.conf = (tuple(equi_img.shape), hFOV, wFOV, theta, phi, h, w, layout)
        return pers

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_pers):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        return (_freeview.launch_equi2pers_bwd(_upstream(grad_pers), *ctx.conf),) + (None,) * 7


class _Pers2Equi(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pers_img, hFOV, wFOV, theta, phi, H, W):
        erp, mask = _freeview.launch_pers2equi(pers_img, hFOV, wFOV, theta, phi, H, W, allow_grad=True)
        hFOV, wFOV, H, W = _freeview.check_view(hFOV, wFOV, H, W)
        ctx.conf = (tuple(pers_img.shape), hFOV, wFOV, theta, phi, H, W)
        mask = mask.to(torch.int64)
        ctx.mark_non_differentiable(mask)
        return erp, mask

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_erp, _grad_mask):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        return (_freeview.launch_pers2equi_bwd(_upstream(grad_erp), *ctx.conf),) + (None,) * 6


class _ViewsToErp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pers, hFOV, wFOV, theta, phi, H, W):
        erp, count = _freeview.views_to_erp(pers, hFOV, wFOV, theta, phi, H, W, allow_grad=True)
        hFOV, wFOV, H, W = _freeview.check_view(hFOV, wFOV, H, W)
        ctx.conf = (tuple(pers.shape), hFOV, wFOV, theta, phi, H, W)
        ctx.mark_non_differentiable(count)
        return erp, count

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_erp, _grad_count):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        return (_freeview.launch_views_to_erp_bwd(_upstream(grad_erp), *ctx.conf),) + (None,) * 6


def equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w):
    if not _wants_grad(equi_img):
        return _e2p.equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w)
    theta, phi = _freeview.angles(theta, phi)
    return _Equi2Pers.apply(equi_img, hFOV, wFOV, theta, phi, output_h, output_w, _lib.LAYOUT_BCHNW)


def equi2pers_planar(equi_img, hFOV, wFOV, theta, phi, output_h, output_w):
    if not _wants_grad(equi_img):
        return _e2p.equi2pers_planar(equi_img, hFOV, wFOV, theta, phi, output_h, output_w)
    theta, phi = _freeview.angles(theta, phi)
    return _Equi2Pers.apply(equi_img, hFOV, wFOV, theta, phi, output_h, output_w, _lib.LAYOUT_BNCHW)


def pers2equi(pers_img, hFOV, wFOV, theta, phi, output_h, output_w):
    if not _wants_grad(pers_img):
        return _p2e.pers2equi(pers_img, hFOV, wFOV, theta, phi, output_h, output_w)
    theta, phi = _freeview.angles(theta, phi)
    return _Pers2Equi.apply(pers_img, hFOV, wFOV, theta, phi, output_h, output_w)


def views_to_erp(pers, hFOV, wFOV, theta, phi, H, W):
    if not _wants_grad(pers):
        return _freeview.views_to_erp(pers, hFOV, wFOV, theta, phi, H, W)
    theta, phi = _freeview.angles(theta, phi)
    return _ViewsToErp.apply(pers, hFOV, wFOV, theta, phi, H, W)
