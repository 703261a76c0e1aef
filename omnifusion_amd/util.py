"""Depth-image-based rendering — host-side mirror of /root/reference/util.py:384-413.

    uvgrid = spherical.create_image_grid(W, H); sgrid = spherical.create_spherical_grid(W)
    right = dibr_horizontal(depth, image, uvgrid, sgrid, baseline)      # [B,C,H,W]: the view from a camera moved sideways
    below = dibr_vertical(depth, image, uvgrid, sgrid, baseline)        # ... moved along the vertical axis

Same names, arguments and values as the reference.  The displacement (spherical/derivatives.py:53-71,93-105,168-177), the
coordinate clean-up and the splat (supervision/splatting.py render, max_depth 8) run in ONE kernel of libomnifusion_hip.so
(csrc/omni_dibr.hip); no coordinate tensor is written.  The reference's quirks are kept: the horizontal mode wraps u modulo the
literal 512 (not W), and non-finite coordinates become the absolute coordinate 0.  uvgrid and sgrid are read, not assumed: each
may be [1,2,H,W] (shared by the batch) or [B,2,H,W].

Differentiable w.r.t. depth and image, like the reference's (photometric self-supervision: render a depth map into a second view,
score it with supervision.photometric.calculate_loss, back-propagate into the depth): a hand-written gather backward chains the
splat's gradient into the depth through the weight and through the displacement, with the reference's rules for its clean-ups and
clamps.  uvgrid / sgrid / baseline get no gradient.  Where depth == 0 the depth gradient is 0 (the reference: NaN).

Free-view sampling — mirror of the reference's util.py:40-60:

    pers = transform_equi(equi, THETA, PHI, output_h, output_w, select_pers, h_fov, v_fov)        # [bs*select_pers, C, output_h, N*output_w]
    equi, mask = transform_pers(pers, THETA, PHI, output_h_pano, output_w_pano, h_fov, v_fov)    # [N,C,H,W], [N,1,1,H,W]

Same names, arguments and shapes; they run equi_pers.equi2pers_torch / pers2equi_torch (csrc/omni_freeview.hip).
"""
import ctypes

import torch

from . import _lib
from .supervision.splatting import _check, _p, check_image_depth, grad_needs_device, run, run_backward

VERTICAL, HORIZONTAL = 0, 1


def _grids(uvgrid, sgrid, B, H, W, device):
    _check("uvgrid", uvgrid)
    _check("sgrid", sgrid)
    for name, g in (("uvgrid", uvgrid), ("sgrid", sgrid)):
        if g.shape[1:] != (2, H, W) or g.shape[0] not in (1, B):
            raise ValueError(f"{name} must be [1,2,H,W] or [B,2,H,W] with (B,H,W) = {(B, H, W)} (got {tuple(g.shape)})")
        if g.device != device:
            raise ValueError(f"{name} must live on the image's device")
    batched = B > 1 and (uvgrid.shape[0] == B or sgrid.shape[0] == B)
    if batched:
        uvgrid, sgrid = uvgrid.expand(B, 2, H, W), sgrid.expand(B, 2, H, W)
    return uvgrid.contiguous(), sgrid.contiguous(), int(batched)


class _Dibr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, image, uv, sg, batched, baseline, mode, want_mask):
        B, C, H, W = image.shape

        def launch(lib, recon, mask, wt, ws, stream):
            _lib.check(lib.omni_dibr_wt_f32(_p(image), _p(depth), _p(uv), _p(sg), batched, float(baseline), mode, _p(recon), _p(mask), _p(wt),
                                            B, C, H, W, _p(ws), stream), "dibr")
        recon, mask, wt = run(image, depth, want_mask, launch, want_wt=True)
        ctx.save_for_backward(depth, image, uv, sg, recon, wt)
        ctx.conf = (batched, float(baseline), mode)
        if mask is None:
            return recon, None
        ctx.mark_non_differentiable(mask)
        return recon, mask

    @staticmethod
    def backward(ctx, grad_recon, _grad_mask):
        depth, image, uv, sg, recon, wt = ctx.saved_tensors
        batched, baseline, mode = ctx.conf
        B, C, H, W = image.shape
        needs = dict(depth=depth.shape if ctx.needs_input_grad[0] else None, img=image.shape if ctx.needs_input_grad[1] else None)

        def launch(lib, g, grads, ws, stream):
            _lib.check(lib.omni_dibr_bwd_f32(_p(g), _p(recon), _p(wt), _p(image), _p(depth), _p(uv), _p(sg), batched, baseline, mode,
                                             _p(grads["img"]), _p(grads["depth"]), B, C, H, W, _p(ws), stream), "dibr backward")
        grads = run_backward(image, grad_recon, needs, launch)
        return grads["depth"], grads["img"], None, None, None, None, None, None


def _dibr(depth, image, uvgrid, sgrid, baseline, mode, want_mask=False):
    grad_needs_device(depth=depth, image=image, uvgrid=uvgrid, sgrid=sgrid)
    B, C, H, W = check_image_depth(image, depth)
    uv, sg, batched = _grids(uvgrid, sgrid, B, H, W, image.device)
    uv, sg = uv.detach(), sg.detach()
    image, depth = image.contiguous(), depth.contiguous()
    if torch.is_grad_enabled() and (image.requires_grad or depth.requires_grad):
        return _Dibr.apply(depth, image, uv, sg, batched, baseline, mode, want_mask)

    def launch(lib, recon, mask, wt, ws, stream):
        _lib.check(lib.omni_dibr_f32(_p(image), _p(depth), _p(uv), _p(sg), batched, float(baseline), mode, _p(recon), _p(mask),
                                     B, C, H, W, _p(ws), stream), "dibr")
    return run(image, depth, want_mask, launch)


def dibr_vertical(depth, image, uvgrid, sgrid, baseline):
    return _dibr(depth, image, uvgrid, sgrid, baseline, VERTICAL)[0]


def dibr_horizontal(depth, image, uvgrid, sgrid, baseline):
    return _dibr(depth, image, uvgrid, sgrid, baseline, HORIZONTAL)[0]


def transform_equi(equi, THETA, PHI, output_h, output_w, select_pers, h_fov, v_fov):
    """The reference repeats every panorama select_pers times before sampling; the copies are equal, so the views are sampled once
    and the result is repeated instead."""
    from .equi_pers.equi2pers_torch import equi2pers
    pers = equi2pers(equi, h_fov, v_fov, THETA, PHI, output_h, output_w)
    return pers.repeat_interleave(int(select_pers), dim=0)


def transform_pers(pers, THETA, PHI, output_h_pano, output_w_pano, h_fov, v_fov):
    from .equi_pers.pers2equi_torch import pers2equi
    equi, mask = pers2equi(pers, h_fov, v_fov, THETA, PHI, output_h_pano, output_w_pano)
    return equi, mask.unsqueeze(1)
