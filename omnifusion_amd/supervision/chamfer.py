"""Chamfer distance between point clouds on the device — the 3-D term of the reference's supervision (util.py:201-257,
chamfer_distance_with_batch), without its [B,N,M,D] intermediate.

    dist, idx = nearest_neighbours(p1, p2, mask1=None, mask2=None)              # [B,N] float32 (differentiable), [B,N] int32
    loss = chamfer_distance(p1, p2, mask1=None, mask2=None, bidirectional=False, reduction="sum")
    loss = depth_chamfer(pred, gt, mask, stride=1)                              # clouds ray * depth of two [B,1,H,W] depth maps

p1 is [B,N,D], p2 [B,M,D] with D = 2 or 3; dist[b,i] = min over the valid j of |p1[b,i] - p2[b,j]|, idx the argmin — the LOWEST index among
equal distances (torch.min leaves that open).  chamfer_distance sums dist over batch and points ("sum", what the reference returns) or divides
each direction by its number of valid queries ("mean"); bidirectional=True adds the call with the clouds (and masks) swapped.  Everything
numeric runs in libomnifusion_hip.so (csrc/omni_chamfer.hip): an all-pairs walk with the targets tiled in LDS, squared
distances from direct differences, the sum in double in a fixed order; the backward sends each query's unit vector to its nearest target
through 64-bit fixed-point sums.  No floating-point atomics, no host synchronisation: every output has the same bits on every run, and an
item's outputs do not depend on the rest of the batch.  Differentiable w.r.t. both clouds; only the requested gradients are computed.

Masks may be bool, uint8 or float ([B,N] / [B,M]); a point is valid where the mask is non-zero.  A masked query has dist 0, idx -1 and no
gradient; a masked target is never a neighbour.  The gradient is 0 where dist == 0 (torch's subgradient of the 2-norm at 0).  A NaN
coordinate of a valid target makes every dist of its item NaN, one of a valid query its own dist; a NaN at a masked point changes nothing.
An item without a valid target has dist = +inf, idx = -1 and no gradient.
"""
import torch

from .. import _lib
from .._lib import ptr as _p


def _workspace(nbytes, device):
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)


class _NearestNeighbours(torch.autograd.Function):
    """-> (dist [B,N], idx [B,N], loss 0-d).  dist and loss are differentiable; their upstream gradients add."""

    @staticmethod
    def forward(ctx, p1, p2, mask1, mask2):
        lib = _lib.load()
        B, N, D = p1.shape
        M = p2.shape[1]
        dist = torch.empty(B, N, dtype=torch.float32, device=p1.device)
        idx = torch.empty(B, N, dtype=torch.int32, device=p1.device)
        loss = torch.empty(1, dtype=torch.float32, device=p1.device)
        ws = _workspace(lib.omni_chamfer_workspace_bytes(B, N, M, D), p1.device)
        with torch.cuda.device(p1.device):
            _lib.check(lib.omni_chamfer_nn_f32(_p(p1), _p(p2), _p(mask1), _p(mask2), B, N, M, D, _p(dist), _p(idx), _p(loss), _p(ws),
                                               _lib.stream_of(p1)), "chamfer nearest neighbours")
        ctx.save_for_backward(p1, p2, mask1, idx)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return dist, idx, loss[0]

    @staticmethod
    def backward(ctx, grad_dist, _grad_idx, grad_loss):
        p1, p2, mask1, idx = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (grad_dist is None and grad_loss is None) or not (need1 or need2):
            return None, None, None, None
        lib = _lib.load()
        B, N, D = p1.shape
        M = p2.shape[1]
        gd = None if grad_dist is None else grad_dist.contiguous().to(torch.float32)
        gl = None if grad_loss is None else grad_loss.contiguous().to(torch.float32)
        g1 = torch.empty_like(p1) if need1 else None
        g2 = torch.empty_like(p2) if need2 else None
        ws = _workspace(lib.omni_chamfer_workspace_bytes(B, N, M, D), p1.device) if need2 else None
        with torch.cuda.device(p1.device):
            _lib.check(lib.omni_chamfer_grad_f32(_p(p1), _p(p2), _p(mask1), _p(idx), _p(gl), _p(gd), B, N, M, D, _p(g1), _p(g2), _p(ws),
                                                 _lib.stream_of(p1)), "chamfer backward")
        return g1, g2, None, None


def _cloud(t, name):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty [B,N,D] tensor (got shape {tuple(t.shape)})")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if t.shape[2] not in (2, 3):
        raise ValueError(f"{name} must hold 2-D or 3-D points, [B,N,2] or [B,N,3] (got shape {tuple(t.shape)})")
    return t.contiguous()


def _mask(mask, name, cloud, cloud_name):
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{name} must be a tensor or None")
    if tuple(mask.shape) != tuple(cloud.shape[:2]):
        raise ValueError(f"{name} must be [B,N] = {tuple(cloud.shape[:2])}, the points of {cloud_name} (got shape {tuple(mask.shape)})")
    if mask.device != cloud.device:
        raise ValueError(f"{name} must live on the device of {cloud_name}")
    if mask.requires_grad:
        raise ValueError(f"{name} must not require grad: the Chamfer term is differentiable w.r.t. the clouds only")
    return mask.contiguous() if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8).contiguous()


def _run(p1, p2, mask1, mask2):
    p1, p2 = _cloud(p1, "p1"), _cloud(p2, "p2")
    if p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError(f"p1 [B,N,D] and p2 [B,M,D] must agree in B and D (got {tuple(p1.shape)}, {tuple(p2.shape)})")
    if p1.device != p2.device:
        raise ValueError("p1 and p2 must live on the same device")
    return _NearestNeighbours.apply(p1, p2, _mask(mask1, "mask1", p1, "p1"), _mask(mask2, "mask2", p2, "p2"))


def nearest_neighbours(p1, p2, mask1=None, mask2=None):
    """-> (dist [B,N] float32, idx [B,N] int32): every valid point of p1 to its nearest valid point of p2; dist is differentiable w.r.t. both
    clouds."""
    dist, idx, _ = _run(p1, p2, mask1, mask2)
    return dist, idx


def _valid(mask, cloud):
    return cloud.shape[0] * cloud.shape[1] if mask is None else (mask != 0).sum()


def chamfer_distance(p1, p2, mask1=None, mask2=None, bidirectional=False, reduction="sum"):
    """-> 0-d float32 tensor on the device.  "sum": the sum over batch and points of p1's nearest-neighbour distances (the reference's value);
    "mean": that sum divided by the number of valid points of p1.  bidirectional=True adds the same term of p2 against p1."""
    if reduction not in ("sum", "mean"):
        raise ValueError(f"reduction must be 'sum' or 'mean' (got {reduction!r})")
    loss = _run(p1, p2, mask1, mask2)[2]
    if reduction == "mean":
        loss = loss / _valid(mask1, p1)
    if bidirectional:
        back = _run(p2, p1, mask2, mask1)[2]
        loss = loss + (back / _valid(mask2, p2) if reduction == "mean" else back)
    return loss


_RAYS = {}


def unit_rays(height, width, device):
    """float32 [H*W, 3] on `device`: the unit ray of every pixel of the default spherical grid (spherical.grid.default_sgrid), in the order
    of coords_3d: (-cos phi cos theta, sin theta, sin phi cos theta).  Built once per size and device."""
    from ..spherical.grid import _index, default_sgrid, direction_factors
    device = torch.device(device)
    key = (int(height), int(width), device.type, _index(device))
    r = _RAYS.get(key)
    if r is None:
        cp, sp, ct, st = direction_factors(default_sgrid(height, width, device), device)
        r = _RAYS[key] = torch.stack((-(cp * ct), st, sp * ct), dim=-1).reshape(height * width, 3).contiguous()
    return r


def depth_points(depth, stride=1):
    """[B,1,H,W] depth -> [B, H' W', 3] points ray * depth of every stride-th row and column (plain torch: autograd reaches the depth)."""
    B, _, H, W = depth.shape
    rays = unit_rays(H, W, depth.device).view(H, W, 3)[::stride, ::stride]
    return (rays.unsqueeze(0) * depth[:, 0, ::stride, ::stride].unsqueeze(-1).to(torch.float32)).reshape(B, -1, 3)


def depth_chamfer(pred, gt, mask, stride=1):
    """The Chamfer term between the point clouds of two depth maps [B,1,H,W] on the default spherical grid: sum over the valid pixels of
    `pred` (every stride-th row and column) of the distance to the nearest valid point of `gt`.  `mask` [B,1,H,W] (bool, uint8 or float)
    is the validity of both clouds.  Differentiable w.r.t. pred (and gt) through the ray * depth product."""
    for t, name in ((pred, "pred"), (gt, "gt"), (mask, "mask")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
        if t.dim() != 4 or t.shape[1] != 1 or t.numel() == 0:
            raise ValueError(f"{name} must be a non-empty [B,1,H,W] tensor (got shape {tuple(t.shape)})")
    if pred.shape != gt.shape or pred.shape != mask.shape:
        raise ValueError(f"pred, gt and mask must have the same shape [B,1,H,W] (got {tuple(pred.shape)}, {tuple(gt.shape)}, {tuple(mask.shape)})")
    if not pred.is_floating_point() or not gt.is_floating_point():
        raise ValueError("pred and gt must be floating-point tensors")
    if not isinstance(stride, int) or stride < 1:
        raise ValueError(f"stride must be a positive integer (got {stride!r})")
    m = mask[:, 0, ::stride, ::stride].reshape(mask.shape[0], -1)
    return chamfer_distance(depth_points(pred, stride), depth_points(gt, stride), m, m)
