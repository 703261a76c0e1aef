"""Seeded inputs of the smoothness fixtures G20a-e, a torch restatement of the guided smoothness term written from its formulae (DESIGN.md §15;
parametrised by dtype: float64 is the yardstick of the GPU tests) and — where the reference checkout is present — the reference's own
functions (tools/gen_golden_smoothness.py writes their results; tests/test_smoothness_*.py regenerate the same inputs and compare).
Only results and float64 input checksums are stored in tests/golden/.

    V    = (-d cos(phi) cos(theta), d sin(theta), d sin(phi) cos(theta))                    the vertices of depth d on the grid (phi, theta)
    du   = sum_k |V_k[i,j] - V_k[i,j+1]|,  dv = sum_k |V_k[i,j] - V_k[i+1,j]|               replicate padding: 0 in the last column / row
    mag  = sqrt(du^2 + dv^2),  g = sqrt(sum_c (I_c[i,j] - I_c[i,j+1])^2 + (I_c[i,j] - I_c[i+1,j])^2)
    loss = sum(mask ? mag exp(-g) w : 0) / sum(mask)
"""
import numpy as np
import torch

from _geometry_cases import directional_residual, rel_error, smooth_field  # noqa: F401  (the same fields and error measures)
from _util import rng_uniform

NAMES = ("G20a", "G20b", "G20c", "G20d", "G20e")
SHAPES = {"G20a": (2, 24, 40), "G20b": (1, 2, 2), "G20c": (2, 17, 67), "G20d": (4, 70, 130), "G20e": (2, 40, 72)}
SEEDS = {"G20a": 2001, "G20b": 2011, "G20c": 2021, "G20d": 2031, "G20e": 2041}
WEIGHTED = ("G20a", "G20c", "G20e")                   # the others pass weights=None: both instantiations of the kernels are covered
CHANNELS = 3
DIRECTION_H = 3e-3                                    # the step of the directional-derivative check (as tests/_geometry_cases.py)
KINK_MARGIN = 1e-4                                    # no interior vertex difference that matters is closer to 0 (kink_margin below)
TINY_FACTOR = 1e-6


def case(name):
    """-> dict(depth [B,1,H,W], image [B,3,H,W], weights [B,1,H,W] or None: float32; mask: bool [B,1,H,W]).  Smooth depth around 2.5 plus a
    checkerboard of +-0.72 and a little noise: about [1.5, 3.5].  A vertex difference d_p f_p - d_q f_q vanishes where d_p / d_q = f_q / f_p,
    and next to a zero crossing of a direction factor f that ratio runs through 2, 3/2, 4/3, ... (a crossing on a pixel) or 3, 5/3, 7/5, ...
    (between two pixels); the checkerboard keeps d_p / d_q within about [1.7, 1.93] or its inverse, between those values, so every
    difference that matters stays off the kink of |.| (kink_margin below; the generator checks it).
    A smooth image in [0, 1] plus noise, a random mask of about 80 %.  G20e: rectangular holes on top of the random mask and
    weights = (1 - a) * mask with a smooth a in [0, 0.8]."""
    B, H, W = SHAPES[name]
    s = SEEDS[name]
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    checker = np.where((ii + jj) % 2 == 0, 1.0, -1.0)[None, None]
    depth = 2.5 + 0.25 * smooth_field(s, B, H, W) + 0.72 * checker + 0.01 * (2 * rng_uniform(s + 2, (B, 1, H, W)).astype(np.float64) - 1)
    image = np.concatenate([0.5 + 0.3 * smooth_field(s + 10 + c, B, H, W) for c in range(CHANNELS)], axis=1) \
        + 0.1 * (rng_uniform(s + 3, (B, CHANNELS, H, W)).astype(np.float64) - 0.5)
    mask = rng_uniform(s + 4, (B, 1, H, W)) < 0.8
    weights = None
    if name == "G20e":
        g = np.random.default_rng(s + 5)
        for b in range(B):
            for _ in range(6):
                y, x = int(g.integers(0, H - 6)), int(g.integers(0, W - 10))
                mask[b, 0, y:y + int(g.integers(2, 7)), x:x + int(g.integers(2, 11))] = False
        weights = (1.0 - 0.4 * (1.0 + smooth_field(s + 6, B, H, W))) * mask
    elif name in WEIGHTED:
        weights = 1.0 + 0.5 * smooth_field(s + 6, B, H, W)
    return dict(depth=depth.astype(np.float32), image=image.astype(np.float32), mask=mask, weights=None if weights is None else weights.astype(np.float32))


def direction(name):
    """The direction of the directional-derivative check: the checkerboard of the depth, smoothly modulated.  (The term is made of differences
    of neighbouring vertices: along a smooth direction they barely move, <grad, v> is a thousand times smaller and the check ill-conditioned.)"""
    B, H, W = SHAPES[name]
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.where((ii + jj) % 2 == 0, 1.0, -1.0)[None, None] * (1.0 + 0.5 * smooth_field(SEEDS[name] + 7, B, H, W))


def checksums(c):
    return {k: np.float64(np.asarray(v, np.float64).sum()) for k, v in c.items() if isinstance(v, np.ndarray)}


def sgrid(H, W):
    """float32 [1,2,H,W]: phi = u 2 pi / W - 3 pi / 2, theta = v pi / H - pi / 2 — the grid of create_spherical_grid for any height."""
    u = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(1, H, W) * (2 * np.pi / W) + (-np.pi - np.pi / 2.0)
    v = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(1, H, W) * (np.pi / H) + (-np.pi / 2.0)
    return torch.stack((u, v), dim=1)


# ------------------------------------------------------------------ the restatement
def directions(sg):
    """[1,3,H,W]: d vertex / d depth in sg's dtype."""
    p, t = sg[:, 0:1], sg[:, 1:2]
    return torch.cat((torch.cos(p) * -1 * torch.cos(t), torch.sin(t), torch.sin(p) * torch.cos(t)), dim=1)


def vertices(sg, depth):
    p, t = sg[:, 0:1], sg[:, 1:2]
    return torch.cat((depth * torch.cos(p) * -1 * torch.cos(t), depth * torch.sin(t), depth * torch.sin(p) * torch.cos(t)), dim=1)


def diff_u(t):
    return t - torch.cat((t[..., 1:], t[..., -1:]), dim=-1)


def diff_v(t):
    return t - torch.cat((t[..., 1:, :], t[..., -1:, :]), dim=-2)


def norm2(a, b):
    """The 2-norm over the channels of a and b together; its autograd gradient is 0 where the norm is 0."""
    return torch.linalg.vector_norm(torch.cat((a, b), dim=1), ord=2, dim=1, keepdim=True)


def image_norm(img):
    return norm2(diff_u(img), diff_v(img))


def vertex_norm(V):
    return norm2(diff_u(V).abs().sum(1, keepdim=True), diff_v(V).abs().sum(1, keepdim=True))


def loss_of_maps(input_duv, guide_duv, mask, weights):
    """The mask selects, the weight included (the reference multiplies the zeroed term by the weight afterwards)."""
    t = input_duv * torch.exp(-guide_duv)
    if weights is not None:
        t = t * weights
    return torch.where(mask, t, torch.zeros_like(t)).sum() / mask.sum()


def loss_of_depth(depth, image, mask, weights, sg):
    return loss_of_maps(vertex_norm(vertices(sg, depth)), image_norm(image), mask, weights)


def grad_by_hand(depth, image, mask, weights, sg):
    """d loss / d depth as the gather the kernel performs, with its selects: a depth pixel receives from its own term, from its left
    neighbour's du and from its upper neighbour's dv; a masked term and a term whose magnitude is 0 send nothing, whatever their values are;
    d|x|/dx = 0 at 0 (and at NaN).  Equal to autograd of loss_of_depth wherever every value is finite (tests/test_smoothness_cpu.py)."""
    f = directions(sg)
    V = f * depth
    dU, dV = diff_u(V), diff_v(V)
    du, dv = dU.abs().sum(1, keepdim=True), dV.abs().sum(1, keepdim=True)
    mag = torch.sqrt(du * du + dv * dv)
    c = torch.exp(-image_norm(image)) / mask.sum()
    if weights is not None:
        c = c * weights
    zero = torch.zeros_like(mag)
    sel = mask & (mag != 0)
    gu, gv = torch.where(sel, c * du / mag, zero), torch.where(sel, c * dv / mag, zero)
    sign0 = lambda x: torch.where(x > 0, torch.ones_like(x), torch.where(x < 0, -torch.ones_like(x), torch.zeros_like(x)))
    sU, sV = sign0(dU), sign0(dV)
    right = lambda t: torch.cat((torch.zeros_like(t[..., :1]), t[..., :-1]), dim=-1)          # [.., j] <- [.., j - 1]
    down = lambda t: torch.cat((torch.zeros_like(t[..., :1, :]), t[..., :-1, :]), dim=-2)     # [.., i, :] <- [.., i - 1, :]
    own = gu * (sU * f).sum(1, keepdim=True) + gv * (sV * f).sum(1, keepdim=True)
    return own - right(gu) * (right(sU) * f).sum(1, keepdim=True) - down(gv) * (down(sV) * f).sum(1, keepdim=True)


def kink_margin(c):
    """The least |vertex difference| over the interior differences that matter (float64): those of the last column (du) and the last row (dv)
    are 0 by construction, and a coordinate whose direction factor is below 1e-6 at both pixels (sin(theta) on the equator row of an even
    H, cos(theta) on the pole row, cos(phi) / sin(phi) on one column each) contributes less than 1e-6 of the depth difference to the value
    and to the gradient whatever its sign is."""
    H, W = c["depth"].shape[2:]
    sg = sgrid(H, W).double()
    f = directions(sg).abs()
    V = vertices(sg, torch.from_numpy(c["depth"]).double())
    tiny = f < TINY_FACTOR
    least = float("inf")
    if W > 1:
        d = (V[..., :-1] - V[..., 1:]).abs()
        keep = ~(tiny[..., :-1] & tiny[..., 1:]).expand_as(d)
        least = min(least, float(d[keep].min()))
    if H > 1:
        d = (V[..., :-1, :] - V[..., 1:, :]).abs()
        keep = ~(tiny[..., :-1, :] & tiny[..., 1:, :]).expand_as(d)
        least = min(least, float(d[keep].min()))
    return least


def poison(c):
    """-> (the case with pixel (b, i, j), its left and its upper neighbour masked, a NaN depth and an infinite weight at (b, i, j)), (b, i, j)."""
    b, i, j = 1, 9, 20
    mask, depth, weights = c["mask"].copy(), c["depth"].copy(), c["weights"].copy()
    mask[b, 0, i, j] = mask[b, 0, i, j - 1] = mask[b, 0, i - 1, j] = False
    depth[b, 0, i, j] = np.nan
    weights[b, 0, i, j] = np.inf
    return dict(c, mask=mask, depth=depth, weights=weights), (b, i, j)


def tensors(c, dtype, device="cpu"):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    H, W = c["depth"].shape[2:]
    return t(c["depth"]), t(c["image"]), torch.from_numpy(c["mask"]).to(device), t(c["weights"]), sgrid(H, W).to(device=device, dtype=dtype)


def run_restatement(c, dtype, device="cpu"):
    """-> dict(loss float; dV_dxyz, dI_duv, grad arrays)."""
    depth, image, mask, weights, sg = tensors(c, dtype, device)
    depth.requires_grad_(True)
    mag, g = vertex_norm(vertices(sg, depth)), image_norm(image)
    loss = loss_of_maps(mag, g, mask, weights)
    grad, = torch.autograd.grad(loss, depth)
    return dict(loss=float(loss.detach()), dV_dxyz=mag.detach().cpu().numpy(), dI_duv=g.cpu().numpy(), grad=grad.cpu().numpy())


# ------------------------------------------------------------------ the reference's own functions
def run_reference(c, dtype):
    """The same quantities from the reference's coords_3d / dV_dxyz / dI_duv / guided_smoothness_loss and its autograd on the CPU (needs the
    reference checkout; used by the generator and by the CPU test only).  The grid holds float32 values cast to `dtype`; weights=None is
    passed as ones (the reference has no default)."""
    import sys
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    if root not in sys.path:
        sys.path.insert(0, root)
    import spherical as S360                                                 # the reference's packages (pure torch)
    import supervision as L
    depth, image, mask, weights, sg = tensors(c, dtype)
    depth.requires_grad_(True)
    if weights is None:
        weights = torch.ones_like(depth)
    mag, g = S360.dV_dxyz(S360.coords_3d(sg, depth)), S360.dI_duv(image)
    loss = L.guided_smoothness_loss(mag, g, mask, weights)
    grad, = torch.autograd.grad(loss, depth)
    return dict(loss=float(loss.detach()), dV_dxyz=mag.detach().numpy(), dI_duv=g.numpy(), grad=grad.numpy())


def reference_loss32(c, depth):
    return run_reference(dict(c, depth=depth), torch.float32)["loss"]
