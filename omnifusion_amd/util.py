"""Depth-image-based rendering — host-side mirror of /root/reference/util.py:384-413.

    uvgrid = spherical.create_image_grid(W, H); sgrid = spherical.create_spherical_grid(W)
    right = dibr_horizontal(depth, image, uvgrid, sgrid, baseline)      # [B,C,H,W]: the view from a camera moved sideways
    below = dibr_vertical(depth, image, uvgrid, sgrid, baseline)        # ... moved along the vertical axis

Same names, arguments and values as the reference.  The displacement (spherical/derivatives.py:53-71,93-105,168-177), the
coordinate clean-up and the splat (supervision/splatting.py render, max_depth 8) run in ONE kernel of libomnifusion_hip.so
(csrc/omni_dibr.hip); no coordinate tensor is written.  The reference's quirks are kept: the horizontal mode wraps u modulo the
literal 512 (not W), and non-finite coordinates become the absolute coordinate 0.  uvgrid and sgrid are read, not assumed: each
may be [1,2,H,W] (shared by the batch) or [B,2,H,W].  Inference only.
"""
import ctypes

import torch

from . import _lib
from .supervision.splatting import _check, _p, check_image_depth, inference_only, run

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


def _dibr(depth, image, uvgrid, sgrid, baseline, mode, want_mask=False):
    inference_only(depth=depth, image=image, uvgrid=uvgrid, sgrid=sgrid)
    B, C, H, W = check_image_depth(image, depth)
    uv, sg, batched = _grids(uvgrid, sgrid, B, H, W, image.device)
    image, depth = image.contiguous(), depth.contiguous()

    def launch(lib, recon, mask, ws, stream):
        _lib.check(lib.omni_dibr_f32(_p(image), _p(depth), _p(uv), _p(sg), batched, float(baseline), mode, _p(recon), _p(mask),
                                     B, C, H, W, _p(ws), stream), "dibr")
    return run(image, depth, want_mask, launch)


def dibr_vertical(depth, image, uvgrid, sgrid, baseline):
    return _dibr(depth, image, uvgrid, sgrid, baseline, VERTICAL)[0]


def dibr_horizontal(depth, image, uvgrid, sgrid, baseline):
    return _dibr(depth, image, uvgrid, sgrid, baseline, HORIZONTAL)[0]
