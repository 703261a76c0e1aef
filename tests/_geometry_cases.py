"""Seeded inputs of the geometry fixtures G19a-e, a torch restatement of the two geometry terms written from their formulae (DESIGN.md §14;
parametrised by dtype: float64 is the yardstick of the GPU tests) and — where the reference checkout is present — the reference's own
functions (tools/gen_golden_geometry.py writes their results; tests/test_geometry_*.py regenerate the same inputs and compare).
Only results and float64 input checksums are stored in tests/golden/."""
import numpy as np
import torch
import torch.nn.functional as F

from _util import rng_uniform

NAMES = ("G19a", "G19b", "G19c", "G19d", "G19e")
SHAPES = {"G19a": (2, 24, 40), "G19b": (1, 2, 2), "G19c": (2, 17, 67), "G19d": (4, 70, 130), "G19e": (2, 40, 72)}
SEEDS = {"G19a": 1901, "G19b": 1911, "G19c": 1921, "G19d": 1971, "G19e": 1941}
AMPLITUDE = {"G19d": 0.6}                             # of the perturbation (default 0.2): 58 000 masked Sobel differences must all stay off 0
DIRECTION_H = 3e-3                                    # the step of the directional-derivative check (as tests/test_photometric_gpu.py)


def smooth_field(seed, B, H, W, waves=6):
    """A seeded sum of low-frequency sinusoids in [-1, 1], float64 [B,1,H,W]; defined for every size, 2 x 2 included."""
    g = np.random.default_rng(seed)
    y = (np.arange(H, dtype=np.float64)[:, None] + 0.5) / max(H, 8)
    x = (np.arange(W, dtype=np.float64)[None, :] + 0.5) / max(W, 8)
    out = np.zeros((B, 1, H, W))
    for b in range(B):
        amp = g.random(waves) + 0.2
        fy, fx, ph = g.random(waves) * 9.0, g.random(waves) * 9.0, g.random(waves) * 2 * np.pi
        for k in range(waves):
            out[b, 0] += amp[k] / amp.sum() * np.sin(fy[k] * y + fx[k] * x + ph[k])
    return out


def case(name):
    """-> dict(pred, gt, mask float32 [B,1,H,W], erode).  G19a-d: hole-free ground truth in about [1, 4], pred = gt + a smooth perturbation, a
    random mask of about 80 %.  G19e: about 8 % of the ground truth zeroed (what the loaders do to invalid depth), mask = gt > 0, erode_mask=True."""
    B, H, W = SHAPES[name]
    s = SEEDS[name]
    gt = 2.5 + 1.5 * smooth_field(s, B, H, W)
    pred = gt + AMPLITUDE.get(name, 0.2) * smooth_field(s + 1, B, H, W) + 0.03 * smooth_field(s + 2, B, H, W, waves=12)
    if name == "G19e":
        valid = rng_uniform(s + 3, (B, 1, H, W)) >= 0.08
        gt = gt * valid
        mask = valid.astype(np.float32)
    else:
        mask = (rng_uniform(s + 3, (B, 1, H, W)) < 0.8).astype(np.float32)
    return dict(pred=pred.astype(np.float32), gt=gt.astype(np.float32), mask=mask, erode=name == "G19e")


def b3_case():
    """B = 3, 8 x 12: the batch size at which the reference's `torch.cross` (no dim) takes the batch axis; in no golden."""
    B, H, W = 3, 8, 12
    gt = 2.5 + 1.5 * smooth_field(1951, B, H, W)
    pred = gt + 0.2 * smooth_field(1952, B, H, W)
    return dict(pred=pred.astype(np.float32), gt=gt.astype(np.float32), mask=(rng_uniform(1953, (B, 1, H, W)) < 0.8).astype(np.float32), erode=False)


def direction(name):
    """The smooth direction of the directional-derivative check: the main component of pred - gt.  (A direction unrelated to pred - gt meets the
    gradient's sign pattern at random: <grad, v> is then 100 times smaller and the check ill-conditioned.)"""
    B, H, W = SHAPES[name]
    return smooth_field(SEEDS[name] + 1, B, H, W)


def checksums(c):
    return {k: np.float64(np.asarray(v, np.float64).sum()) for k, v in c.items() if isinstance(v, np.ndarray)}


# ------------------------------------------------------------------ the restatement
def rays(H, W):
    """float32 [3,H,W]: uv2xyz(coords2uv(1-based pixel coordinates)) — the angle in float64, stored as float32, float32 sin / cos and products."""
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    u = ((jj + 1 - (W / 2 + 0.5)) / W * 2 * np.pi).astype(np.float32)
    v = (-(ii + 1 - (H / 2 + 0.5)) / H * np.pi).astype(np.float32)
    return np.stack([np.cos(v) * np.sin(u), np.cos(v) * np.cos(u), np.sin(v)]).astype(np.float32)


_RAYS = {}


def normals(depth):
    """depth [B,1,H,W] -> [B,3,H,W] in depth's dtype and on its device; the rays are float32 values whatever the dtype.  Crosses over channels."""
    H, W = depth.shape[2:]
    key = (H, W, depth.dtype, depth.device)
    if key not in _RAYS:
        _RAYS[key] = torch.from_numpy(rays(H, W)).to(depth)[None]
    V = _RAYS[key] * depth
    v0 = F.pad(V[:, :, :, :-1] - V[:, :, :, 1:], (0, 1))
    v2 = F.pad(V[:, :, :-1, :] - V[:, :, 1:, :], (0, 0, 0, 1))
    v4 = F.pad(V[:, :, :, 1:] - V[:, :, :, :-1], (1, 0))
    v6 = F.pad(V[:, :, 1:, :] - V[:, :, :-1, :], (0, 0, 1, 0))
    unit = lambda a, b: F.normalize(torch.cross(a, b, dim=1), dim=1)
    return F.normalize(unit(v2, v0) + unit(v4, v2) + unit(v6, v4) + unit(v0, v6), dim=1)


SOBEL_X = [[1, 0, -1], [2, 0, -2], [1, 0, -1]]
SOBEL_Y = [[1, 2, 1], [0, 0, 0], [-1, -2, -1]]


def imgrad(img):
    """-> (grad_y, grad_x) of the channel mean; the float32 weights of the reference cast to img's dtype."""
    m = img.mean(1, keepdim=True)
    w = lambda k: torch.tensor(k, dtype=torch.float32)[None, None].to(m)
    return F.conv2d(m, w(SOBEL_Y), padding=1), F.conv2d(m, w(SOBEL_X), padding=1)


def imgrad_yx(img):
    return torch.cat(imgrad(img), dim=1)


def l1_loss(pred, gt, mask):
    count = mask.sum(dim=[1, 2, 3], keepdim=True).to(pred.dtype)
    return ((gt - pred).abs() * mask.to(pred.dtype)).sum(dim=[1, 2, 3], keepdim=True).div(count).mean()


def eroded(mask):
    """mask * [mask != 0 at all eight neighbours], neighbours outside the image counting as valid."""
    hole = F.pad((mask == 0).to(torch.float32), (1, 1, 1, 1))
    near = F.max_pool2d(hole, 3, stride=1)
    return mask * (near == 0).to(mask.dtype)


def terms(pred, gt, mask, erode=False):
    """-> (normal_loss, grad_loss, normals(pred)) in pred's dtype."""
    if erode:
        mask = eroded(mask)
    m = mask.to(pred.dtype)
    pn, gn = normals(pred), normals(gt)
    normal_loss = 1 - ((pn * gn * m).sum(dim=[1, 2, 3], keepdim=True) / m.sum()).mean()
    return normal_loss, l1_loss(imgrad_yx(pred), imgrad_yx(gt), m), pn


def run_restatement(c, dtype, device="cpu"):
    """-> dict(normal_loss, grad_loss float; normals, grad_normal, grad_grad arrays; min_dsobel: the least |gt' - pred'| over masked pixels)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    p = t(c["pred"]).requires_grad_(True)
    nl, gl, pn = terms(p, t(c["gt"]), t(c["mask"]), c["erode"])
    gn, = torch.autograd.grad(nl, p, retain_graph=True)
    gg, = torch.autograd.grad(gl, p)
    with torch.no_grad():
        m = eroded(t(c["mask"])) if c["erode"] else t(c["mask"])
        d = (imgrad_yx(t(c["gt"])) - imgrad_yx(p)).abs()
        min_d = float(d[(m != 0).expand_as(d)].min()) if bool((m != 0).any()) else float("inf")
    return dict(normal_loss=float(nl.detach()), grad_loss=float(gl.detach()), normals=pn.detach().cpu().numpy(), grad_normal=gn.cpu().numpy(), grad_grad=gg.cpu().numpy(),
                min_dsobel=min_d)


# ------------------------------------------------------------------ the reference's own functions
def run_reference(c, dtype):
    """The same quantities from the reference's depth2normal_gpu / imgrad_yx / calculate_l1_loss and the formula of train_erp_depth.py:271 on the
    CPU (needs the reference checkout; used by the generator and by the CPU test only).  util.py imports the whole model zoo at module level, so the
    functions needed are exec'd alone — here only, never stored; `.cuda()` is the identity for the duration of the call.  The reference's rays are
    float32 numpy values and its Sobel weights float32 tensors: they are cast to `dtype` (what the restatement does too)."""
    import os
    import torch.nn as nn
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    src = open(os.path.join(root, "util.py")).read()
    cut = lambda a, b: src[src.index(a):src.index(b)] if b else src[src.index(a):]
    code = cut("def coords2uv", "def xyz2uv") + cut("def depth2normal_gpu", "def dibr_vertical") + cut("def imgrad(", None)
    cast = dtype != torch.float32
    if cast:                                                                # float32 constants of the reference, cast where they meet the data
        code = code.replace("torch.from_numpy(xyz).cuda()", "torch.from_numpy(xyz).to(depth.dtype)")
        code = code.replace(".float().unsqueeze(0).unsqueeze(0)", ".float().unsqueeze(0).unsqueeze(0).to(img.dtype)")
    ns = {"torch": torch, "np": np, "F": F, "nn": nn}
    direct = {"torch": torch}
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        exec(compile(code, "util_geometry", "exec"), ns)
        exec(compile(open(os.path.join(root, "supervision", "direct.py")).read(), "direct", "exec"), direct)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        p, gt, mask = t(c["pred"]).requires_grad_(True), t(c["gt"]), t(c["mask"])
        if c["erode"]:
            mask = eroded(mask)
        pn, gn = ns["depth2normal_gpu"](p), ns["depth2normal_gpu"](gt)
        nl = 1 - torch.mean(torch.sum((pn * gn * mask), dim=[1, 2, 3], keepdim=True) / mask.sum())           # train_erp_depth.py:271
        gl = direct["calculate_l1_loss"](ns["imgrad_yx"](p), ns["imgrad_yx"](gt), mask)                      # :272-274
        g_n, = torch.autograd.grad(nl, p, retain_graph=True)
        g_g, = torch.autograd.grad(gl, p)
    finally:
        torch.Tensor.cuda = saved
    return dict(normal_loss=float(nl.detach()), grad_loss=float(gl.detach()), normals=pn.detach().numpy(), grad_normal=g_n.numpy(), grad_grad=g_g.numpy())


def reference_loss32(c, pred):
    """normal_loss + grad_loss of the reference in float32 for another prediction (the directional-derivative residual of the generator)."""
    r = run_reference(dict(c, pred=pred), torch.float32)
    return r["normal_loss"] + r["grad_loss"]


def rel_error(got, want64):
    """|g - g_ref64| / max|g_ref64|: the error measure of the project's gradient gates."""
    got = np.asarray(got, np.float64); want = np.asarray(want64, np.float64)
    return np.abs(got - want) / np.abs(want).max()


def directional_residual(loss_of, grad, pred, v, h):
    """|central difference - <grad, step>| / |<grad, step>|, the step being the one actually taken after rounding to float32."""
    plus = (pred.astype(np.float64) + h * v).astype(np.float32)
    minus = (pred.astype(np.float64) - h * v).astype(np.float32)
    dot = float((np.asarray(grad, np.float64) * (plus.astype(np.float64) - minus.astype(np.float64))).sum())
    fd = loss_of(plus) - loss_of(minus)
    return abs(fd - dot) / abs(dot), fd, dot
