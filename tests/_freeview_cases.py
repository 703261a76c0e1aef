"""Free-view sampling fixtures G16a-d (tools/gen_golden_freeview.py -> tests/golden/G16*_freeview.npz): the case table, the seeded inputs
and a plain torch-CPU restatement of the reference's equi_pers/equi2pers_torch.py:37 and equi_pers/pers2equi_torch.py:37 in a chosen
dtype.  The restatement is test infrastructure: the CPU tests pin it against the goldens (which come from the reference itself), the
GPU tests use it where no golden exists (frustum coordinates of the flip predicate, the round trip, views_to_erp)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from _util import golden, rng_uniform

NAMES = ("G16a", "G16b", "G16c", "G16d")
CUBE_THETA = (0.0, 90.0, 180.0, -90.0, 0.0, 0.0)
CUBE_PHI = (0.0, 0.0, 0.0, 0.0, 90.0, -90.0)
#        ERP (B, C, H, W)   view (h, w)  theta                              phi                             hFOV  wFOV
CASES = {
    "G16a": ((2, 3, 32, 64), (16, 24), (20.5, -133.25, 71.0, -8.5), (10.25, -47.5, 33.0, 2.75), 60.0, 90.0),
    "G16b": ((1, 1, 33, 70), (17, 23), (175.0, -179.5, 40.0), (5.0, -12.0, 80.0), 80.0, 80.0),
    "G16c": ((1, 3, 64, 128), (32, 32), CUBE_THETA, CUBE_PHI, 90.0, 90.0),
    "G16d": ((1, 2, 16, 260), (8, 130), (-61.75,), (14.5,), 50.0, 120.0),
}
FLIP_CAP = 1e-4          # cases a, b, d: at most one flipped mask element per 10 000
FLIP_REL = 1e-5          # a mask element may flip only where a float64 frustum coordinate is this close (relative) to its bound ...
FLIP_X = 1e-6            # ... or the ray lies this close to the plane x = 0


def case(name):
    """-> dict(erp [B,C,H,W], pers [N,C,h,w] (random too: not an output of the other direction), theta, phi, hfov, wfov, h, w, H, W)"""
    (B, C, H, W), (h, w), theta, phi, hfov, wfov = CASES[name]
    k = NAMES.index(name)
    return dict(name=name, erp=rng_uniform(1700 + 10 * k, (B, C, H, W)), pers=rng_uniform(1701 + 10 * k, (len(theta), C, h, w)),
                theta=np.asarray(theta, np.float32), phi=np.asarray(phi, np.float32), hfov=hfov, wfov=wfov, h=h, w=w, H=H, W=W)


def load(name):
    return golden(name + "_freeview")


# ---------------------------------------------------------------------------------------------------------------- restatement
def quaternion_rotation(angle, axis):
    """angle [N] (radians), axis [N,3] or [3] -> [N,3,3]: the matrix of the quaternion (cos(a/2), -axis sin(a/2))."""
    axis = F.normalize(axis.to(angle.dtype), dim=-1).reshape(-1, 3)
    a = torch.cos(angle / 2)
    b, c, d = (-axis * torch.sin(angle / 2)[:, None]).unbind(-1)
    rows = [a * a + b * b - c * c - d * d, 2 * (b * c + a * d), 2 * (b * d - a * c),
            2 * (b * c - a * d), a * a + c * c - b * b - d * d, 2 * (c * d + a * b),
            2 * (b * d + a * c), 2 * (c * d - a * b), a * a + d * d - b * b - c * c]
    return torch.stack(rows, -1).reshape(-1, 3, 3)


def view_rotations(theta, phi, dtype):
    """-> (R1, R2) [N,3,3]: yaw about z, then pitch by -phi about the yawed y axis."""
    theta = torch.as_tensor(np.asarray(theta)).to(dtype)
    phi = torch.as_tensor(np.asarray(phi)).to(dtype)
    R1 = quaternion_rotation(torch.deg2rad(theta), torch.tensor([0.0, 0.0, 1.0], dtype=dtype))
    R2 = quaternion_rotation(torch.deg2rad(-phi), R1[:, :, 1])
    return R1, R2


def _lens(hfov, wfov):
    return math.tan(math.radians(hfov / 2.0)), math.tan(math.radians(wfov / 2.0))


def equi2pers(erp, hfov, wfov, theta, phi, h, w, dtype=torch.float64):
    """erp [B,C,H,W] (numpy or tensor) -> [B,C,h,N*w] in `dtype`."""
    erp = torch.as_tensor(np.asarray(erp)).to(dtype)
    B, _, H, W = erp.shape
    h_len, w_len = _lens(hfov, wfov)
    y = torch.linspace(-w_len, w_len, w, dtype=dtype)[None, :].expand(h, w)
    z = -torch.linspace(-h_len, h_len, h, dtype=dtype)[:, None].expand(h, w)
    x = torch.ones(h, w, dtype=dtype)
    ray = torch.stack((x, y, z), -1) / torch.sqrt(x ** 2 + y ** 2 + z ** 2)[..., None]
    R1, R2 = view_rotations(theta, phi, dtype)
    N = R1.shape[0]
    ray = torch.matmul(R2, torch.matmul(R1, ray.reshape(-1, 3).T)).transpose(2, 1)          # [N, h*w, 3]
    lat = torch.asin(ray[..., 2])
    lon = torch.atan2(ray[..., 1], ray[..., 0])
    lon = lon / math.pi * 180
    lat = -lat / math.pi * 180
    lon = lon / 180 * ((W - 1) / 2.0) + (W - 1) / 2.0
    lat = lat / 90 * ((H - 1) / 2.0) + (H - 1) / 2.0
    lon = (lon / W - 0.5) * 2
    lat = (lat / H - 0.5) * 2
    side = lambda t: t.reshape(N, h, w).permute(1, 0, 2).reshape(h, N * w)
    grid = torch.stack([side(lon), side(lat)], -1)[None].expand(B, h, N * w, 2)
    return F.grid_sample(erp, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def frustum_coordinates(theta, phi, H, W, dtype=torch.float64):
    """-> (x, y / x, z / x) [N,H,W]: the ERP rays in each view's frame (x before the division)."""
    lat, lon = torch.meshgrid(torch.linspace(90, -90, H, dtype=dtype), torch.linspace(-180, 180, W, dtype=dtype), indexing="ij")
    lat, lon = torch.deg2rad(lat), torch.deg2rad(lon)
    ray = torch.stack((torch.cos(lon) * torch.cos(lat), torch.sin(lon) * torch.cos(lat), torch.sin(lat)), -1)
    R1, R2 = view_rotations(theta, phi, dtype)
    N = R1.shape[0]
    ray = ray.reshape(1, H * W, 3).transpose(2, 1).expand(N, 3, H * W)
    ray = torch.matmul(torch.inverse(R1), torch.matmul(torch.inverse(R2), ray)).transpose(2, 1).reshape(N, H, W, 3)
    x = ray[..., 0]
    return x, ray[..., 1] / x, ray[..., 2] / x


def pers2equi(pers, hfov, wfov, theta, phi, H, W, dtype=torch.float64):
    """pers [N,C,h,w] -> (erp [N,C,H,W] in `dtype`, mask [N,1,H,W] int64)."""
    pers = torch.as_tensor(np.asarray(pers)).to(dtype)
    _, _, h, w = pers.shape
    h_len, w_len = _lens(hfov, wfov)
    x, y, z = frustum_coordinates(theta, phi, H, W, dtype)
    inside = (-w_len < y) & (y < w_len) & (-h_len < z) & (z < h_len)
    zero = torch.zeros((), dtype=dtype)
    u = torch.where(inside, (y + w_len) / 2 / w_len * float(w), zero)
    v = torch.where(inside, (-z + h_len) / 2 / h_len * float(h), zero)
    grid = torch.stack([(u / w - 0.5) * 2, (v / h - 0.5) * 2], -1)
    mask = (inside & (x > 0)).to(torch.int64)[:, None]
    erp = F.grid_sample(pers, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * mask
    return erp, mask


def flip_allowed(theta, phi, hfov, wfov, H, W):
    """[N,1,H,W] bool: where a float32 evaluation of the mask may differ from the float64 one (FLIP_REL, FLIP_X)."""
    h_len, w_len = _lens(hfov, wfov)
    x, y, z = frustum_coordinates(theta, phi, H, W, torch.float64)
    near = ((y.abs() - w_len).abs() <= FLIP_REL * w_len) | ((z.abs() - h_len).abs() <= FLIP_REL * h_len) | (x.abs() < FLIP_X)
    return near[:, None].numpy()


def merge(erps, masks):
    """sum_v erp_v / max(sum_v mask_v, 1) over dim 0 of [N,C,H,W] / [N,1,H,W] -> ([C,H,W], count [1,H,W])."""
    count = masks.sum(0)
    return erps.sum(0) / count.clamp(min=1).to(erps.dtype), count


def smooth_pattern(C, H, W):
    """A low-order trigonometric panorama [1,C,H,W] in [0,1] (float32), continuous across the seam."""
    lat = np.linspace(90, -90, H)[:, None] * np.pi / 180
    lon = np.linspace(-180, 180, W)[None, :] * np.pi / 180
    planes = [0.5 + 0.25 * np.cos(lat) * np.cos(lon + 0.7 * c) + 0.2 * np.sin(lat) * np.cos(2 * lat + c) + 0.05 * np.cos(lat) ** 2 * np.sin(2 * lon)
              for c in range(C)]
    return np.stack(planes)[None].astype(np.float32)
