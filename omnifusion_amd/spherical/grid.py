"""Pixel and spherical grids of an equirectangular image — mirror of /root/reference/spherical/grid.py:4-44.

    uvgrid = create_image_grid(W, H)          # [1,2,H,W]: u = column index, v = row index
    sgrid = create_spherical_grid(W)          # [1,2,W//2,W]: phi = u * 2 pi / W - 3 pi / 2, theta = v * pi / H - pi / 2

Built by torch on the host (or on `device=`) with the reference's operations in the reference's order, so the fp32 values are
the same bits.  `device` is keyword-only and not in the reference.
"""
import numpy
import torch


def _ranges(width, height, data_type, device):
    v = torch.arange(0, height, device=device).view(1, height, 1).expand(1, height, width).type(data_type)
    u = torch.arange(0, width, device=device).view(1, 1, width).expand(1, height, width).type(data_type)
    return u, v


def create_image_grid(width, height, data_type=torch.float32, *, device=None):
    u, v = _ranges(width, height, data_type, device)
    return torch.stack((u, v), dim=1)


def create_spherical_grid(width, horizontal_shift=(-numpy.pi - numpy.pi / 2.0), vertical_shift=(-numpy.pi / 2.0),
                          data_type=torch.float32, *, device=None):
    height = int(width // 2.0)
    u, v = _ranges(width, height, data_type, device)
    u = u * (2 * numpy.pi / width)          # [0, 2 pi)
    v = v * (numpy.pi / height)             # [0, pi)
    u = u + horizontal_shift                # standard: [-3 pi / 2, pi / 2)
    v = v + vertical_shift                  # standard: [-pi / 2, pi / 2)
    return torch.stack((u, v), dim=1)
