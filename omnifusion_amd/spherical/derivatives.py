"""Spatial derivatives of images and of structured point clouds — mirror of the reference's spherical/derivatives.py:7-24,190-214.

    dI_du(img), dI_dv(img)        # [B,C,H,W] -> [B,C,H,W]: t[i,j] - t[i,j+1] / t[i,j] - t[i+1,j], replicate padding (last column / row: 0)
    dI_duv(img)                   # [B,C,H,W] -> [B,1,H,W]: the 2-norm over the 2 C difference channels
    dV_dx / dV_dy / dV_dz(pcloud) # dI_duv of one coordinate of a [B,3,H,W] point cloud
    dV_dxyz(pcloud)               # [B,3,H,W] -> [B,1,H,W]: sqrt(du^2 + dv^2), du = |du_x| + |du_y| + |du_z|, dv likewise

Everything numeric runs in libomnifusion_hip.so (csrc/omni_smoothness.hip); float32 tensors on the device, forward only:
the differentiable path is supervision.smoothness.depth_smoothness.  There is no CPU path.
"""
import torch

from .. import _lib
from .._lib import ptr as _p
from .cartesian import xi, yi, zeta


def _prepare(t, name, channels=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.requires_grad and torch.is_grad_enabled():
        raise ValueError(f"{name} requires grad: the derivative maps are forward only (use supervision.smoothness.depth_smoothness)")
    if t.dim() != 4 or t.numel() == 0 or not t.is_floating_point():
        raise ValueError(f"{name} must be a non-empty floating-point [B,C,H,W] tensor (got shape {tuple(t.shape)}, {t.dtype})")
    if channels is not None and t.shape[1] != channels:
        raise ValueError(f"{name} must have {channels} channels (got shape {tuple(t.shape)})")
    return t.detach().contiguous().to(torch.float32)


def _diff(img, axis, name):
    t = _prepare(img, name)
    B, C, H, W = t.shape
    out = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().omni_image_diff_f32(_p(t), B, C, H, W, axis, _p(out), _lib.stream_of(t)), name)
    return out


def dI_du(img):
    return _diff(img, 0, "dI_du")


def dI_dv(img):
    return _diff(img, 1, "dI_dv")


def dI_duv(img):
    t = _prepare(img, "dI_duv")
    B, C, H, W = t.shape
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().omni_image_diff_norm_f32(_p(t), B, C, H, W, _p(out), _lib.stream_of(t)), "dI_duv")
    return out


def dV_dx(pcloud):
    return dI_duv(xi(pcloud))


def dV_dy(pcloud):
    return dI_duv(yi(pcloud))


def dV_dz(pcloud):
    return dI_duv(zeta(pcloud))


def dV_dxyz(pcloud):
    t = _prepare(pcloud, "dV_dxyz", channels=3)
    B, _, H, W = t.shape
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().omni_vertex_diff_norm_f32(_p(t), B, H, W, _p(out), _lib.stream_of(t)), "dV_dxyz")
    return out
