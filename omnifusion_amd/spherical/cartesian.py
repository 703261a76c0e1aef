"""Cartesian coordinates from spherical ones — mirror of the reference's spherical/cartesian.py:14-50.

    z is the forward axis, y the up axis, x the right axis, r the radius (spherical depth);
    phi is the longitude (on the x-z plane), theta the latitude (on the y-z plane), with the offsets of create_spherical_grid.

    pcloud = coords_3d(sgrid, depth)          # [B,3,H,W] from sgrid [1,2,H,W] and depth [B,1,H,W]

Plain torch on whatever device the tensors live, the reference's operations in the reference's order (differentiable, as the reference's).
The training path does not call these: supervision.smoothness.depth_smoothness evaluates the same products inside its kernel
(csrc/omni_smoothness.hip) and writes no vertex map.
"""
import torch

from .grid import phi, theta


def coord_x(sgrid, depth):
    return depth * torch.cos(phi(sgrid)) * -1 * torch.cos(theta(sgrid))


def coord_y(sgrid, depth):
    return depth * torch.sin(theta(sgrid))


def coord_z(sgrid, depth):
    return depth * torch.sin(phi(sgrid)) * torch.cos(theta(sgrid))


def coords_3d(sgrid, depth):
    return torch.cat((coord_x(sgrid, depth), coord_y(sgrid, depth), coord_z(sgrid, depth)), dim=1)


def xi(pcloud):
    return pcloud[:, 0, :, :].unsqueeze(1)


def yi(pcloud):
    return pcloud[:, 1, :, :].unsqueeze(1)


def zeta(pcloud):
    return pcloud[:, 2, :, :].unsqueeze(1)
