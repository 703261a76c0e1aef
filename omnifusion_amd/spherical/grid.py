"""Pixel and spherical grids of an equirectangular image — mirror of /root/reference/spherical/grid.py:4-62.

    uvgrid = create_image_grid(W, H)          # [1,2,H,W]: u = column index, v = row index
    sgrid = create_spherical_grid(W)          # [1,2,W//2,W]: phi = u * 2 pi / W - 3 pi / 2, theta = v * pi / H - pi / 2

Built by torch on the host (or on `device=`) with the reference's operations in the reference's order, so the fp32 values are
the same bits.  `device` is keyword-only and not in the reference.

    phi(sgrid), theta(sgrid)                  # [1,1,H,W] views of the two channels; azimuth / longitude and elevation / latitude are aliases
    direction_factors(sgrid, device)          # [4,H,W] float32 = cos phi | sin phi | cos theta | sin theta, what csrc/omni_smoothness.hip reads
"""
import weakref

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


def spherical_grid_of(height, width, data_type=torch.float32, *, device=None):
    """create_spherical_grid for any height (the reference ties it to width // 2): phi = u * 2 pi / W - 3 pi / 2, theta = v * pi / H - pi / 2."""
    u, v = _ranges(width, height, data_type, device)
    return torch.stack((u * (2 * numpy.pi / width) + (-numpy.pi - numpy.pi / 2.0), v * (numpy.pi / height) + (-numpy.pi / 2.0)), dim=1)


def phi(sgrid):  # longitude or azimuth
    return sgrid[:, 0, :, :].unsqueeze(1)


def theta(sgrid):  # latitude or elevation
    return sgrid[:, 1, :, :].unsqueeze(1)


azimuth = longitude = phi
elevation = latitude = theta

_FACTORS = {}


def _index(device):
    if device.index is not None:
        return device.index
    return torch.cuda.current_device() if device.type == "cuda" else -1


def direction_factors(sgrid, device):
    """The four direction factors of coords_3d (spherical/cartesian.py) for one grid tensor [1,2,H,W], as a float32 [4,H,W] tensor on `device`:
    cos phi | sin phi | cos theta | sin theta, evaluated by torch where the grid lives and in its dtype.  Built once per grid TENSOR (and
    per in-place version of it) and kept for as long as the tensor lives, so the kernels evaluate no trigonometry; the first call for a
    grid launches a few element-wise kernels (do it outside a graph capture)."""
    device = torch.device(device)
    key = (id(sgrid), device.type, _index(device))
    hit = _FACTORS.get(key)
    if hit is not None and hit[0]() is sgrid and hit[1] == sgrid._version:
        return hit[2]
    with torch.no_grad():
        p, t = sgrid[0, 0], sgrid[0, 1]
        fac = torch.stack((torch.cos(p), torch.sin(p), torch.cos(t), torch.sin(t))).to(device=device, dtype=torch.float32).contiguous()
    _FACTORS[key] = (weakref.ref(sgrid, lambda _, k=key: _FACTORS.pop(k, None)), sgrid._version, fac)
    return fac


_DEFAULT_GRIDS = {}


def default_sgrid(height, width, device):
    """spherical_grid_of(height, width) on `device`, one tensor per size and device (so its direction factors are built once)."""
    device = torch.device(device)
    key = (int(height), int(width), device.type, _index(device))
    g = _DEFAULT_GRIDS.get(key)
    if g is None:
        g = _DEFAULT_GRIDS[key] = spherical_grid_of(height, width, device=device)
    return g


_RAY_TABLES = {}


def ray_table_values(height, width):
    """The rays of util.py:159-174 (coords2uv of the 1-based pixel coordinates, middle = n / 2 + 0.5, then uv2xyz) are separable:
    xyz(i, j) = (cos v_i sin u_j, cos v_i cos u_j, sin v_i).  -> float32 numpy [2 H + 2 W] = sin v | cos v | sin u | cos u, evaluated with the
    reference's own numpy operations: the angle in float64, stored as float32, then float32 sin / cos."""
    u = ((numpy.arange(width) + 1 - (width / 2 + 0.5)) / width * 2 * numpy.pi).astype(numpy.float32)
    v = (-(numpy.arange(height) + 1 - (height / 2 + 0.5)) / height * numpy.pi).astype(numpy.float32)
    return numpy.concatenate([numpy.sin(v), numpy.cos(v), numpy.sin(u), numpy.cos(u)]).astype(numpy.float32)


def ray_tables(height, width, device):
    """The table above on `device`, built once per (H, W, device) and kept: the kernels of csrc/omni_normals.hip read it instead of evaluating
    any trigonometry.  The first call for a size copies 8 (H + W) bytes to the device (do it outside a graph capture)."""
    device = torch.device(device)
    key = (int(height), int(width), device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _RAY_TABLES.get(key)
    if t is None:
        t = _RAY_TABLES[key] = torch.from_numpy(ray_table_values(height, width)).to(device)
    return t
