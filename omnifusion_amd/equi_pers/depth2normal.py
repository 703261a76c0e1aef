"""Mirror of the reference's equi_pers/depth2normal.py (and model/equi_pers/depth2normal.py): the least-squares normals of a depth map.

    normals = depth2normal(depth)            # [B,1,H,W] -> float32 unit normals [B,3,H,W] on depth's device, differentiable w.r.t. depth

Over the 25 vertices p = ray * depth of a 5 x 5 window at dilation 2 (offsets {-4,-2,0,2,4}^2; a neighbour outside the image is the zero vector,
there is no wrap across the seam) the plane A n = 1 is fitted: M = sum p p^T, s = sum p, n = M^-1 s where det M >= 1e-5 and n = s otherwise (the
reference puts the identity in M's place), then n / max(|n|, 1e-12).  The reference unfolds the vertices to [B,75,H W] and runs batched matmul,
det and inv over them; here one tiled kernel of libomnifusion_hip.so (csrc/omni_planefit.hip) forms the nine moments and solves in
float64, and two kernels give the backward (no atomics: the bits do not change from run to run).  Any H, W >= 1; a NaN depth gives NaN normals at
exactly the centres whose windows hold it.  The loss built on these normals is supervision.geometry.planefit_normal_loss.
"""
import torch

from .. import _lib
from .._lib import ptr as _p
from ..spherical.grid import ray_tables


class _PlanefitNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, tab):
        lib = _lib.load()
        B, _, H, W = depth.shape
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=depth.device)
        with torch.cuda.device(depth.device):
            _lib.check(lib.omni_planefit_normals_f32(_p(depth), _p(tab), B, H, W, _p(out), _lib.stream_of(depth)), "depth2normal")
        ctx.save_for_backward(depth, tab)
        return out

    @staticmethod
    def backward(ctx, grad_normals):
        depth, tab = ctx.saved_tensors
        lib = _lib.load()
        B, _, H, W = depth.shape
        up = grad_normals.contiguous().to(torch.float32)
        ws = torch.empty(lib.omni_planefit_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.float64, device=depth.device)
        grad = torch.empty_like(depth)
        with torch.cuda.device(depth.device):
            _lib.check(lib.omni_planefit_normals_grad_f32(_p(depth), _p(tab), _p(up), B, H, W, _p(ws), _p(grad), _lib.stream_of(depth)),
                       "depth2normal backward")
        return grad, None


def depth2normal(depth):
    if not isinstance(depth, torch.Tensor):
        raise ValueError("depth must be a tensor")
    if not depth.is_cuda:
        raise ValueError("depth must be a tensor on an MI355X device; there is no CPU path")
    if depth.dim() != 4 or depth.shape[1] != 1 or depth.numel() == 0:
        raise ValueError(f"depth must be a non-empty [B,1,H,W] tensor (got shape {tuple(depth.shape)})")
    if not depth.is_floating_point():
        raise ValueError(f"depth must be a floating-point tensor (got {depth.dtype})")
    H, W = depth.shape[2:]
    return _PlanefitNormals.apply(depth.contiguous().to(torch.float32), ray_tables(H, W, depth.device))
