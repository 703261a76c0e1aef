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

Geometry of a depth map — mirror of util.py:332-382 and :426-451 (csrc/omni_normals.hip), forward only:

    normals = depth2normal_gpu(depth)                 # [B,3,H,W]
    grad_y, grad_x = imgrad(img); yx = imgrad_yx(depth)

The differentiable losses built on them are supervision.geometry.geometry_terms / normal_loss / gradient_loss.

Chamfer distance — mirror of util.py:201-257 (csrc/omni_chamfer.hip):

    loss = chamfer_distance_with_batch(p1, p2, debug=False)      # [B,N,D], [B,M,D] -> the sum of p1's nearest-neighbour distances, differentiable

supervision.chamfer has the masked, bidirectional and mean forms and the nearest neighbours themselves.
"""
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


def _forward_only_map(t, name, who, hint):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.requires_grad:
        raise ValueError(f"{who} is forward only; the differentiable entry is {hint}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty [B,C,H,W] tensor (got shape {tuple(t.shape)})")
    if not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor (got {t.dtype})")
    return t.detach().contiguous().to(torch.float32)


def depth2normal_gpu(depth):
    """Mirror of the reference's util.py:332-382: depth [B,1,H,W] -> float32 unit normals [B,3,H,W] of the vertices ray(i, j) * depth, from the
    four one-sided differences (zero where the neighbour lies outside the image, on all four borders; no wrap across the seam), the four
    normalised cross products 2x0, 4x2, 6x4, 0x6 and the normalised sum.  The cross products run over the channel axis for every B (the
    reference's `torch.cross` without `dim` takes the batch axis when B == 3); the result lives on the input's device.
    The curvature map the reference computes and discards is not computed.  Forward only."""
    from .spherical.grid import ray_tables
    x = _forward_only_map(depth, "depth", "depth2normal_gpu", "supervision.geometry.normal_loss")
    B, C, H, W = x.shape
    if C != 1:
        raise ValueError(f"depth must be [B,1,H,W] (got {tuple(depth.shape)})")
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.omni_depth_normals_f32(_p(x), _p(ray_tables(H, W, x.device)), B, H, W, _p(out), _lib.stream_of(x)), "depth2normal_gpu")
    return out


def imgrad(img):
    """Mirror of util.py:426-446: -> (grad_y, grad_x), each [B,1,H,W]: the channel mean of img [B,C,H,W], then the 3x3 Sobel cross-correlations
    with zero padding, [[1,2,1],[0,0,0],[-1,-2,-1]] for y and [[1,0,-1],[2,0,-2],[1,0,-1]] for x.  Forward only."""
    x = _forward_only_map(img, "img", "imgrad", "supervision.geometry.gradient_loss")
    B, C, H, W = x.shape
    gy = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
    gx = torch.empty_like(gy)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.omni_sobel_f32(_p(x), B, C, H, W, _p(gy), _p(gx), _lib.stream_of(x)), "imgrad")
    return gy, gx


def imgrad_yx(img):
    """Mirror of util.py:448-451: cat(grad_y, grad_x) on dim 1, [B,2,H,W].  C must be 1 (the reference's `.view(N, C, h, w)` fails otherwise)."""
    if isinstance(img, torch.Tensor) and img.dim() == 4 and img.shape[1] != 1:
        raise ValueError(f"imgrad_yx needs a single-channel image [B,1,H,W] (got {tuple(img.shape)})")
    return torch.cat(imgrad(img), dim=1)


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


def chamfer_distance_with_batch(p1, p2, debug=False):
    """Mirror of the reference's util.py:201-257: p1 [B,N,D], p2 [B,M,D] -> the sum over batch and points of min_j |p1[b,i] - p2[b,j]|, a 0-d
    float32 tensor on the device, differentiable w.r.t. both clouds.  The reference repeats both clouds to [B,N,M,D] (12 N M bytes per item);
    here nothing of that size exists.  `debug` (the reference prints intermediate tensors) is accepted and ignored."""
    from .supervision.chamfer import chamfer_distance
    return chamfer_distance(p1, p2, reduction="sum")
