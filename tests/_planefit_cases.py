"""Seeded inputs of the plane-fit fixtures G22a-g, a torch restatement of the plane-fit normals written from their formulae (DESIGN.md §18;
parametrised by dtype and device: float64 is the yardstick of the GPU tests), of the loss built on them and of the hand-written backward the
kernels implement, and — where the reference checkout is present — the reference's own depth2normal (tools/gen_golden_planefit.py writes its
results; tests/test_planefit_*.py regenerate the same inputs and compare).  Only results and float64 input checksums are stored in tests/golden/."""
import numpy as np
import torch
import torch.nn.functional as F

import _geometry_cases as gc
from _geometry_cases import checksums, directional_residual, eroded, rays, rel_error, smooth_field  # noqa: F401
from _util import rng_uniform

NAMES = ("G22a", "G22b", "G22c", "G22d", "G22e", "G22f", "G22g")
LOSS_NAMES = NAMES[:-1]                               # G22g is a depth map alone: the forward map only
SHAPES = {"G22a": (2, 24, 40), "G22b": (1, 2, 2), "G22c": (2, 17, 67), "G22d": (1, 24, 512), "G22e": (2, 40, 72), "G22f": (2, 24, 40), "G22g": (2, 24, 40)}
RECIPE = {"G22a": "G19a", "G22b": "G19b", "G22c": "G19c", "G22e": "G19e"}       # the inputs of the geometry fixtures, unchanged
SEED_D = 2241
DET_MIN, EPS = 1e-5, 1e-12                            # depth2normal.py:43, F.normalize's eps
OFFSETS = (-4, -2, 0, 2, 4)                           # a 5 x 5 window at dilation 2
F_SCALE, F_COLUMN = 0.005, 20                         # G22f: the columns from 20 on lie at 0.005 of their depth, their windows take the fallback
G_SCALE = 0.0258                                      # G22g: G22a's ground truth at the scale where det M straddles 1e-5
F_BAND, G_BAND = 0.1, 0.01                            # relative half-widths about 1e-5: G22f has no determinant in its band, G22g <= 1 % of its pixels
DIRECTION_H = gc.DIRECTION_H


def case(name):
    """-> dict(pred, gt, mask float32 [B,1,H,W], erode).  G22g's depth map is `pred`; its gt and mask are not used."""
    if name in RECIPE:
        return gc.case(RECIPE[name])
    if name == "G22d":
        B, H, W = SHAPES[name]
        gt = 2.5 + 1.5 * smooth_field(SEED_D, B, H, W)
        pred = gt + 0.2 * smooth_field(SEED_D + 1, B, H, W) + 0.03 * smooth_field(SEED_D + 2, B, H, W, waves=12)
        mask = (rng_uniform(SEED_D + 3, (B, 1, H, W)) < 0.8).astype(np.float32)
        return dict(pred=pred.astype(np.float32), gt=gt.astype(np.float32), mask=mask, erode=False)
    c = gc.case("G19a")
    if name == "G22f":
        s = np.ones(SHAPES[name][2], np.float32)
        s[F_COLUMN:] = F_SCALE
        return dict(c, pred=c["pred"] * s, gt=c["gt"] * s)
    assert name == "G22g"
    return dict(c, pred=(c["gt"].astype(np.float64) * G_SCALE).astype(np.float32))


def upstream(name):
    """The seeded upstream U [B,3,H,W] of the map's gradient d sum(normals * U) / d depth, in [-1, 1)."""
    B, H, W = SHAPES[name]
    return rng_uniform(2200 + NAMES.index(name), (B, 3, H, W)) * 2 - 1


def direction(name):
    return gc.direction(RECIPE[name])


# ------------------------------------------------------------------ the restatement
_RAYS = {}


def ray_grid(H, W, like):
    key = (H, W, like.dtype, like.device)
    if key not in _RAYS:
        _RAYS[key] = torch.from_numpy(rays(H, W)).to(like)[None]
    return _RAYS[key]


def _window(x):
    """x [B,C,H,W] -> the 25 shifted copies x(i + a, j + b), zero outside the image, row-major over (a, b)."""
    H, W = x.shape[2:]
    p = F.pad(x, (4, 4, 4, 4))
    return [p[:, :, 4 + a:4 + a + H, 4 + b:4 + b + W] for a in OFFSETS for b in OFFSETS]


def fit(depth, branch=None):
    """depth [B,1,H,W] -> dict(out, n, length [B,3|1,H,W]; M [B,H,W,3,3] with the identity where the fallback is taken; det, solved [B,H,W]; V the
    vertices).  branch: None — solved where det >= 1e-5, as the reference; True / False — the solve (where det != 0) / the fallback at every pixel."""
    H, W = depth.shape[2:]
    V = ray_grid(H, W, depth) * depth
    M = torch.zeros(depth.shape[0], 3, 3, H, W, dtype=depth.dtype, device=depth.device)
    s = torch.zeros_like(V)
    for P in _window(V):
        M = M + P[:, :, None] * P[:, None, :]
        s = s + P
    M = M.permute(0, 3, 4, 1, 2)
    det = torch.det(M)
    solved = det >= DET_MIN if branch is None else (det != 0 if branch else torch.zeros_like(det, dtype=torch.bool))
    M = torch.where(solved[..., None, None], M, torch.eye(3, dtype=depth.dtype, device=depth.device))
    n = torch.linalg.solve(M, s.permute(0, 2, 3, 1)[..., None])[..., 0].permute(0, 3, 1, 2)
    length = n.norm(dim=1, keepdim=True)
    return dict(out=n / length.clamp_min(EPS), n=n, length=length, M=M, det=det, solved=solved, V=V)


def normals(depth, branch=None):
    return fit(depth, branch)["out"]


def map_backward(depth, U):
    """The closed form the kernels implement: per centre g_n = (g - o (o.g)) / max(|n|, eps), lambda = M^-1 g_n (g_n in the fallback branch); pixel
    k gathers lambda_c (1 - p_k . n_c) - n_c (lambda_c . p_k) over the 25 centres c at the window's offsets (n_c = 0 in the fallback branch) and
    multiplies by its ray.  -> d sum(normals * U) / d depth."""
    with torch.no_grad():
        f = fit(depth)
        o = f["out"]
        gn = (U - o * (o * U).sum(1, keepdim=True)) / f["length"].clamp_min(EPS)
        lam = torch.linalg.solve(f["M"], gn.permute(0, 2, 3, 1)[..., None])[..., 0].permute(0, 3, 1, 2)
        n = f["n"] * f["solved"][:, None].to(depth.dtype)
        acc = torch.zeros_like(lam)
        for L, N in zip(_window(lam), _window(n)):
            acc = acc + L * (1 - (f["V"] * N).sum(1, keepdim=True)) - N * (L * f["V"]).sum(1, keepdim=True)
        H, W = depth.shape[2:]
        return (ray_grid(H, W, depth) * acc).sum(1, keepdim=True)


def loss_of_normals(pn, gn, mask):
    """train_erp_depth.py:271 — the mask sum is the whole batch's."""
    m = mask.to(pn.dtype)
    return 1 - ((pn * gn * m).sum(dim=[1, 2, 3], keepdim=True) / m.sum()).mean()


def loss(pred, gt, mask, erode=False):
    if erode:
        mask = eroded(mask)
    return loss_of_normals(normals(pred), normals(gt), mask)


def loss_backward(pred, gt, mask, erode=False):
    """d loss / d pred by the closed form: the upstream of a centre is -(1 / B) N(gt) m / sum(m)."""
    with torch.no_grad():
        if erode:
            mask = eroded(mask)
        m = mask.to(pred.dtype)
        return map_backward(pred, -normals(gt) * m / m.sum() / pred.shape[0])


def run_restatement(c, dtype, device="cpu", name=None, hand=False):
    """-> dict(normals, det arrays; and unless the case is G22g: loss float, grad_loss array; with `name`: grad_map for upstream(name); with `hand`:
    hand_grad_loss / hand_grad_map from the closed form)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    p = t(c["pred"]).requires_grad_(True)
    f = fit(p)
    out = dict(normals=f["out"].detach().cpu().numpy(), det=f["det"].detach().cpu().numpy())
    if name is not None:
        U = t(upstream(name))
        out["grad_map"] = torch.autograd.grad((f["out"] * U).sum(), p, retain_graph=True)[0].cpu().numpy()
        if hand:
            out["hand_grad_map"] = map_backward(p.detach(), U).cpu().numpy()
    if name != "G22g":
        l = loss(p, t(c["gt"]), t(c["mask"]), c["erode"])
        out["loss"] = float(l.detach())
        out["grad_loss"] = torch.autograd.grad(l, p)[0].cpu().numpy()
        out["det_gt"] = fit(t(c["gt"]))["det"].cpu().numpy()
        if hand:
            out["hand_grad_loss"] = loss_backward(p.detach(), t(c["gt"]), t(c["mask"]), c["erode"]).cpu().numpy()
    return out


def band(det, width):
    """The pixels whose determinant lies within `width` (relative) of the threshold."""
    return np.abs(np.asarray(det, np.float64) - DET_MIN) <= width * DET_MIN


# ------------------------------------------------------------------ the reference's own function
def run_reference(c, dtype, name=None):
    """The same quantities from the reference's equi_pers/depth2normal.py and the formula of train_erp_depth.py:271 on the CPU (needs the reference
    checkout; used by the generator and by the CPU test only).  coords2uv / uv2xyz of util.py and the body of depth2normal are exec'd alone — here
    only, never stored.  The reference's rays, its right-hand side of ones and its identity are float32: they are cast to `dtype` where they meet
    the data.  The determinants the function computes and drops are recorded through torch.det."""
    import os
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    util = open(os.path.join(root, "util.py")).read()
    body = open(os.path.join(root, "equi_pers", "depth2normal.py")).read()
    code = util[util.index("def coords2uv"):util.index("def xyz2uv")] + body[body.index("def depth2normal"):]
    if dtype != torch.float32:
        for a, b in (("torch.from_numpy(xyz).to(device)", "torch.from_numpy(xyz).to(device).to(depth.dtype)"),
                     ("kernel_size*kernel_size, 1], device=device)", "kernel_size*kernel_size, 1], device=device, dtype=depth.dtype)"),
                     ("torch.ones([3], dtype=torch.float32, device=device)", "torch.ones([3], dtype=depth.dtype, device=device)")):
            assert code.count(a) == 1, a
            code = code.replace(a, b)
    ns = {"torch": torch, "np": np, "F": F}
    exec(compile(code, "depth2normal", "exec"), ns)
    dets = []
    real_det = torch.det

    def det(x):
        d = real_det(x)
        dets.append(d.detach().numpy().copy())
        return d
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    torch.det = det
    try:
        p = t(c["pred"]).requires_grad_(True)
        pn = ns["depth2normal"](p)
        out = dict(normals=pn.detach().numpy(), det=dets[0])
        if name is not None:
            out["grad_map"] = torch.autograd.grad((pn * t(upstream(name))).sum(), p, retain_graph=True)[0].numpy()
        if name != "G22g":
            mask = eroded(t(c["mask"])) if c["erode"] else t(c["mask"])
            gn = ns["depth2normal"](t(c["gt"]))
            l = 1 - torch.mean(torch.sum((pn * gn * mask), dim=[1, 2, 3], keepdim=True) / mask.sum())           # train_erp_depth.py:271
            out["loss"] = float(l.detach())
            out["grad_loss"] = torch.autograd.grad(l, p)[0].numpy()
            out["det_gt"] = dets[1]
    finally:
        torch.det = real_det
    return out
