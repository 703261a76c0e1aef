"""Seeded view-synthesis cases off the tile grid (tests/test_vs_restatement_cpu.py, tests/test_vs_shapes_gpu.py): ragged images,
images smaller than a tile, C in {1, 2, 3, 4, 5, 8}, the LDS window of the splat at and over equality, the 512 wrap inside the image,
and the photometric windows, modes and mask / weight layouts no fixture covers.  All inputs come from _util.smooth_erp / rng_uniform.

GAPS below is the restatement's own float32 run against its float64 run (tests/_vs_restatement.py, on the CPU) per case and
quantity: (largest error, elements over the ceiling of the quantity's gate).  Errors of recon and the SSIM map are absolute, the
loss's absolute, gradients' relative to the largest float64 gradient of the tensor (_vs_cases.rel_error).  The ceilings are the
existing gates of the same quantities (CEILING); `tolerance` turns a row into the gate of the GPU test.
test_float32_restatement_stays_inside_the_gates recomputes the table and holds it to these figures.
"""
import numpy as np

import _dibr_cases as dc
from _util import rng_uniform, smooth_erp

DIBR_WIN, TILE_R, TILE_C = 6144, 16, 64            # csrc/omni_dibr.hip: int64 words of LDS per block; source rows x columns per block

# quantity -> (tolerance of one element, largest share of a tensor's elements over it, bound on every element)
CEILING = {
    "recon": (1e-4, 1e-3, 1e-2),       # test_dibr_gpu.py: samples over 1e-4 counted, none over 1e-2; the share is _util's `frac` for this family
    "grad": (1e-4, 2e-4, 1e-2),        # test_dibr_bwd_gpu.py: share over 1e-4 (relative) <= 2e-4, none over 1e-2
    "loss": (2e-6, 0.0, 2e-6),         # test_photometric_gpu.py
    "pgrad": (1e-4, 0.0, 1e-4),        # test_photometric_gpu.py: relative, every element
    "ssim": (2e-6, 0.0, 2e-6),         # test_photometric_gpu.py
}
# the device's outputs are float32 and every one is the end of at least three roundings (a product, a sum converted from fixed point or
# float64, a division): no gate is set below 8 half-units of the last place of the tensor's largest magnitude
FORMAT_FLOOR = 8 * 2.0 ** -24

GAPS = {
    # case: {quantity: (max error, elements over the ceiling's tolerance, elements)}
    "R1": {"recon": (1.86e-07, 0, 5760), "mask": (0, 0, 2880), "grad_img": (7.96e-08, 0, 5760), "grad_depth": (2.77e-05, 0, 2880), "grad_coords": (1.95e-05, 0, 5760)},
    "R2": {"recon": (1.18e-07, 0, 1188), "mask": (0, 0, 297), "grad_img": (8.41e-08, 0, 1188), "grad_depth": (6.08e-06, 0, 297), "grad_coords": (3.52e-06, 0, 594)},
    "R3": {"recon": (5.96e-08, 0, 40960), "mask": (0, 0, 8192), "grad_img": (6.19e-08, 0, 40960), "grad_depth": (1.59e-07, 0, 8192), "grad_coords": (1.58e-07, 0, 16384)},
    "R3h": {"recon": (1.68e-07, 0, 40960), "mask": (0, 0, 8192), "grad_img": (8.73e-08, 0, 40960), "grad_depth": (4.93e-05, 0, 8192), "grad_coords": (1.13e-05, 0, 16384)},
    "R4": {"recon": (2.27e-07, 0, 8840), "mask": (0, 0, 1105), "grad_img": (1.04e-07, 0, 8840), "grad_depth": (2.27e-05, 0, 1105), "grad_coords": (7.16e-06, 0, 2210)},
    "R5": {"recon": (1.73e-07, 0, 8640), "mask": (0, 0, 2880), "grad_img": (8.43e-08, 0, 8640), "grad_depth": (5.00e-07, 0, 2880), "grad_coords": (6.61e-07, 0, 5760)},
    "V1": {"recon": (4.46e-07, 0, 10368), "grad_img": (4.85e-06, 0, 10368), "grad_depth": (3.50e-05, 0, 5184)},
    "V2": {"recon": (1.68e-07, 0, 36992), "grad_img": (3.02e-06, 0, 36992), "grad_depth": (1.09e-05, 0, 9248)},
    "Hz1": {"recon": (2.42e-06, 0, 5184), "grad_img": (1.90e-05, 0, 5184), "grad_depth": (7.80e-05, 0, 2592)},
    "Hz2": {"recon": (1.98e-04, 9, 443904), "grad_img": (2.66e-04, 12, 443904), "grad_depth": (8.78e-04, 9, 147968)},
    ("P1", 0.85): {"loss": (4.64e-08, 0, 1), "grad": (1.21e-05, 0, 1122), "ssim": (1.96e-05, 215, 1122)},
    ("P2", 0.85): {"loss": (3.63e-08, 0, 1), "grad": (5.61e-07, 0, 189), "ssim": (1.67e-06, 0, 189)},
    ("P2b", 0.85): {"loss": (1.82e-08, 0, 1), "grad": (1.51e-06, 0, 189), "ssim": (1.28e-06, 0, 189)},
    ("P3", 0.85): {"loss": (2.62e-08, 0, 1), "grad": (2.60e-05, 0, 17280), "ssim": (7.87e-05, 2271, 17280)},
    ("P4", 0.85): {"loss": (7.76e-08, 0, 1), "grad": (2.90e-05, 0, 9200), "ssim": (8.08e-05, 2704, 9200)},
    ("P5", 0.85): {"loss": (4.12e-08, 0, 1), "grad": (2.95e-07, 0, 9), "ssim": (2.43e-07, 0, 9)},
    ("P6", 0.85): {"loss": (1.50e-08, 0, 1), "grad": (3.20e-06, 0, 4800), "ssim": (5.40e-06, 118, 4800)},
    ("P6", 0.0): {"loss": (1.99e-09, 0, 1), "grad": (6.84e-08, 0, 4800), "ssim": (5.40e-06, 118, 4800)},
    ("P6", 1.0): {"loss": (1.99e-08, 0, 1), "grad": (2.50e-06, 0, 4800), "ssim": (5.40e-06, 118, 4800)},
}


def tolerance(case, quantity, kind, scale=1.0):
    """-> (tol, share, max_tol) for `quantity` ('recon', 'grad_img', 'loss', ...) of `case`; `kind` names the row of CEILING.
    Twice the restatement's own float32 gap where that gap is below half the ceiling and no element left it (the factor of
    test_directional_derivative for "the reference's own residual"), with no share left out then; the ceiling otherwise."""
    tol, share, max_tol = CEILING[kind]
    gap, over, _ = GAPS[case][quantity]
    if over == 0 and gap < 0.5 * tol:
        t = max(2.0 * gap, FORMAT_FLOOR * scale)
        return t, 0.0, t
    return tol, share, max_tol


def _k(H, W):
    """The box filter of smooth_erp wraps along W and needs k // 2 <= W: the widest odd window <= 31 that fits the image."""
    m = min(H, W)
    return min(31, m if m % 2 else m - 1)


def smooth(seed, B, C, H, W):
    return smooth_erp(seed, B, C, H, W, k=_k(H, W))


def smooth_depth(seed, B, H, W, lo=0.3, hi=8.0):
    return (lo + (hi - lo) * smooth(seed, B, 1, H, W)).astype(np.float32)


def safe_fraction(coords):
    """Fractional parts into [0.05, 0.95): every corner weight >= 0.05^2 = 2.5e-3, clear of the 1e-3 step, and floor() clear of an integer."""
    c = coords.astype(np.float64)
    f = np.floor(c)
    return (f + 0.05 + 0.9 * (c - f)).astype(np.float32)


def _render(seed, B, C, H, W, amp, max_depth=20.0):
    disp = (smooth(seed + 2, B, 2, H, W) - 0.5) * np.array(amp, np.float32)[None, :, None, None]
    return dict(kind="render", img=smooth(seed, B, C, H, W), depth=smooth_depth(seed + 1, B, H, W),
                coords=safe_fraction(dc.image_grid(H, W) + disp), max_depth=max_depth)


def _r5():
    """Noise displacement: every source aims anywhere in the image, drawn towards the centre (a cubic of a uniform variable), so every
    tile's box is the image (global path) and the centre pixels take many contributions.  Row 0 carries the edge sources."""
    B, C, H, W = 1, 3, 40, 72
    a, b = rng_uniform(1723, (B, 1, H, W)).astype(np.float64), rng_uniform(1724, (B, 1, H, W)).astype(np.float64)
    u = W / 2 + (2 * a - 1) ** 3 * (W / 2 + 2)                       # reaches beyond the image on both sides
    v = H / 2 + (2 * b - 1) ** 3 * (H / 2 + 2)
    coords = safe_fraction(np.concatenate([u, v], 1))
    edge = [(-1.0, 5.25), (0.0, 6.5), (W - 1.0, 7.5), (10.5, -1.0), (11.5, 0.0), (12.5, H - 1.0), (W - 1.0, H - 1.0), (0.0, 0.0), (-1.0, -1.0),
            (W + 3.5, 8.5), (13.5, H + 2.5), (-7.5, 9.5), (1e30, 3.5), (np.nan, 4.5), (5.5, np.nan), (np.inf, 6.5), (7.5, -np.inf), (np.nan, np.inf)]
    for i, (eu, ev) in enumerate(edge):
        coords[0, :, 0, 2 * i] = (eu, ev)
    return dict(kind="render", img=smooth(1721, B, C, H, W), depth=smooth_depth(1722, B, H, W), coords=coords, max_depth=20.0)


R5_EDGE_SOURCES = 18


def _shift(half):
    B, C, H, W = 2, 5, 32, 128
    s = np.array([3.0, -2.0], np.float32) + (0.5 if half else 0.0)
    return dict(kind="render", img=smooth(1711, B, C, H, W), depth=smooth_depth(1712, B, H, W),
                coords=np.broadcast_to(dc.image_grid(H, W) + s[None, :, None, None], (B, 2, H, W)).astype(np.float32).copy(), max_depth=20.0)


R3_SHIFT = (3, -2)


def gradient_scale(name, k, ref):
    """The scale of the relative error of gradient `k` of case `name` (ref: the float64 restatement): the largest float64 gradient, as
    _vs_cases.rel_error.  R3 apart: one source per target at corner weight 1 makes recon = img whatever the weight and the coordinate,
    so the depth and coordinate gradients are exactly 0 in exact arithmetic (float64 leaves 1e-17) and their scale is that of the terms
    that cancel: sum_c |img_c dL/dimg_c| per source (times 2 / max_depth through the weight)."""
    want = ref["grad_" + k]
    if name == "R3" and k in ("depth", "coords"):
        c = dibr_case(name)
        terms = float(np.abs(c["img"].astype(np.float64) * ref["grad_img"]).sum(1).max())
        return terms * (2.0 / c["max_depth"] if k == "depth" else 1.0)
    return float(np.abs(want[np.isfinite(want)]).max())


def rel_error(name, k, got, ref):
    want = ref["grad_" + k]
    ok = np.isfinite(want)
    return np.where(ok, np.abs(np.where(ok, np.asarray(got, np.float64), 0.0) - np.where(ok, want, 0.0)), 0.0) / gradient_scale(name, k, ref)

DIBR_NAMES = ("R1", "R2", "R3", "R3h", "R4", "R5", "V1", "V2", "Hz1", "Hz2")


def dibr_case(name):
    """-> dict(kind, img, depth, coords (render), max_depth (render), baseline (DIBR modes), grad_out)."""
    if name == "R1":
        c = _render(1701, 2, 2, 20, 72, (24.0, 10.0))
    elif name == "R2":
        c = _render(1705, 1, 4, 9, 33, (10.0, 5.0))
    elif name == "R3":
        c = _shift(False)
    elif name == "R3h":
        c = _shift(True)
    elif name == "R4":
        c = _render(1715, 1, 8, 17, 65, (16.0, 8.0))
    elif name == "R5":
        c = _r5()
    elif name == "V1":                        # a near scene, depths 0.08 .. 0.5: the targets of one tile spread over all 36 rows (over the window)
        c = dict(kind="vertical", img=smooth(1731, 2, 2, 36, 72), depth=smooth_depth(1756, 2, 36, 72, lo=0.08, hi=0.5), baseline=dc.BASELINE)
    elif name == "V2":
        c = dict(kind="vertical", img=smooth(1735, 1, 4, 68, 136), depth=dc.zero_block(smooth_depth(1736, 1, 68, 136)), baseline=dc.BASELINE)
    elif name == "Hz1":
        c = dict(kind="horizontal", img=smooth(1741, 1, 2, 36, 72), depth=dc.zero_block(smooth_depth(1743, 1, 36, 72)), baseline=dc.BASELINE)
    elif name == "Hz2":
        c = dict(kind="horizontal", img=smooth(1745, 1, 3, 272, 544), depth=smooth_depth(1746, 1, 272, 544), baseline=dc.BASELINE)
    else:
        raise KeyError(name)
    c["grad_out"] = (smooth(1777, *c["img"].shape) - 0.5).astype(np.float32)
    return c


def grids(c, dtype=None):
    """The float32 grids the device reads (widened to `dtype` if given)."""
    from omnifusion_amd import spherical
    H, W = c["img"].shape[-2:]
    uv, sg = spherical.create_image_grid(W, H), spherical.create_spherical_grid(W)
    return (uv, sg) if dtype is None else (uv.to(dtype), sg.to(dtype))


def target_coordinates(c):
    """[B,2,H,W] float64 numpy: where every source aims, from the restatement."""
    import torch
    import _vs_restatement as rs
    if c["kind"] == "render":
        return c["coords"].astype(np.float64)
    uv, sg = grids(c)
    return rs.dibr_coords(c["kind"], c["depth"], uv, sg, c["baseline"], torch.float64).numpy()


def survivors(coords, H, W):
    """-> list of four (alive [B,H,W] bool, column, row int64) for the corners that the splat keeps, from float64 coordinates."""
    import torch
    import _vs_restatement as rs
    t = torch.from_numpy(coords)
    u, v = t[:, 0:1], t[:, 1:2]
    ok = torch.isfinite(u) & torch.isfinite(v)
    cs = rs.corners(torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v)), H, W)
    return [(((cw > 0) & ok)[:, 0].numpy(), cu[:, 0].numpy(), cv[:, 0].numpy()) for cw, cu, cv in cs]


def tile_words(c):
    """box * (C + 1) of every splat tile (16 x 64 sources of one item) that keeps a corner: what dibr_splat_kernel compares with DIBR_WIN.
    -> list of (item, tile row, tile column, words)."""
    B, C, H, W = c["img"].shape
    cs = survivors(target_coordinates(c), H, W)
    out = []
    for b in range(B):
        for r0 in range(0, H, TILE_R):
            for c0 in range(0, W, TILE_C):
                sl = np.s_[b, r0:r0 + TILE_R, c0:c0 + TILE_C]
                xs = np.concatenate([cu[sl][alive[sl]] for alive, cu, cv in cs])
                ys = np.concatenate([cv[sl][alive[sl]] for alive, cu, cv in cs])
                if xs.size:
                    out.append((b, r0 // TILE_R, c0 // TILE_C, int((xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)) * (C + 1)))
    return out


def contributions(c):
    """[B,H,W] int: the number of surviving corners that land on every target."""
    B, C, H, W = c["img"].shape
    n = np.zeros((B, H * W), np.int64)
    for alive, cu, cv in survivors(target_coordinates(c), H, W):
        for b in range(B):
            np.add.at(n[b], (cv[b] * W + cu[b])[alive[b]], 1)
    return n.reshape(B, H, W)


# ------------------------------------------------------------------ photometric loss
PHOTO_CONF = {            # B, C, H, W, window, std, mode, channels of the mask, channels of the weights
    "P1": (2, 1, 17, 33, 11, 1.5, "gaussian", 1, 1),
    "P2": (1, 3, 7, 9, 7, 1.5, "gaussian", 1, 1),
    "P2b": (1, 3, 7, 9, 7, 1.5, "box", 1, 1),
    "P3": (3, 2, 40, 72, 5, 1.5, "box", 2, 1),
    "P4": (2, 4, 23, 50, 9, 0.8, "gaussian", 1, 4),
    "P5": (1, 1, 3, 3, 3, 1.5, "box", 1, 1),
    "P6": (2, 3, 20, 40, 7, 1.5, "gaussian", 1, 1),
}
PHOTO_NAMES = tuple(PHOTO_CONF)
P6_ALPHAS = (0.0, 0.85, 1.0)
P6_EQUAL_BLOCK = np.s_[..., 6:14, 16:24]


def photo_case(name, alpha=0.85):
    """As _vs_cases.photo_case: two views of one smooth scene that differ by a smooth field and a little texture, a random validity
    mask (about 90 % ones) and smooth positive weights.  P6: mask values 0 / 0.5 / 1 and an 8 x 8 block where pred == gt bit for bit."""
    B, C, H, W, window, std, mode, mask_c, wts_c = PHOTO_CONF[name]
    s = 1800 + 10 * PHOTO_NAMES.index(name)
    # P4's window (std 0.8) is nearly a point: with 0.06 of texture sigma^2 cancels against C2 and the restatement's own float32 gradient
    # leaves the 1e-4 gate (1.5e-4); 0.15 of texture keeps it inside
    base, tex = (0.6, 0.15) if name == "P4" else (0.7, 0.06)
    gt = (0.15 + base * smooth(s + 1, B, C, H, W) + tex * (rng_uniform(s + 2, (B, C, H, W)) - 0.5)).astype(np.float32)
    pred = (gt + 0.2 * (smooth(s + 3, B, C, H, W) - 0.5) + tex * (rng_uniform(s + 4, (B, C, H, W)) - 0.5)).astype(np.float32)
    r = rng_uniform(s + 5, (B, mask_c, H, W))
    mask = (r < 0.9).astype(np.float32)
    if name == "P5":
        mask[:] = 1.0                                  # nine pixels: keep them all
    if name == "P6":
        mask = np.where(r < 0.1, 0.0, np.where(r < 0.4, 0.5, 1.0)).astype(np.float32)
        pred[P6_EQUAL_BLOCK] = gt[P6_EQUAL_BLOCK]
    weights = (0.5 + smooth(s + 6, B, wts_c, H, W)).astype(np.float32)
    return dict(pred=pred, gt=gt, mask=mask, weights=weights, window=window, std=std, mode=mode, alpha=alpha)


def p6_with_empty_item():
    """P6 and one further item (a copy of item 0) whose mask is all zero: its term is 0 / 0."""
    c = photo_case("P6")
    for k in ("pred", "gt", "mask", "weights"):
        c[k] = np.concatenate([c[k], c[k][:1]], 0)
    c["mask"][2] = 0.0
    return c


# ------------------------------------------------------------------ the restatement's results, computed once per process
def run_dibr(c, dtype, grad=True):
    """The restatement on a case -> dict(recon, mask (render), grad_img, grad_depth[, grad_coords]) of numpy arrays in `dtype`."""
    import torch
    import _vs_restatement as rs
    names = ("img", "depth", "coords") if c["kind"] == "render" else ("img", "depth")
    leaf = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dtype).requires_grad_(grad) for k in names}
    if c["kind"] == "render":
        recon, mask, _ = rs.render(leaf["img"], leaf["depth"], leaf["coords"], c["max_depth"], dtype)
        out = dict(mask=mask.numpy())
    else:
        uv, sg = grids(c)
        recon, out = rs.dibr(c["kind"], leaf["depth"], leaf["img"], uv, sg, c["baseline"], dtype), {}
    out["recon"] = recon.detach().numpy()
    if grad:
        recon.backward(torch.from_numpy(c["grad_out"]).to(dtype))
        out.update({"grad_" + k: v.grad.numpy() for k, v in leaf.items()})
    return out


def run_photo(c, dtype, grad=True, window_2d_float32=False):
    """-> dict(loss (float), grad (numpy), ssim (numpy, of the masked images), dssim_min, dssim_max)."""
    import torch
    import _vs_restatement as rs
    p = torch.from_numpy(np.ascontiguousarray(c["pred"])).to(dtype).requires_grad_(grad)
    loss = rs.photometric(p, c["gt"], c["mask"], c["weights"], c["window"], c["std"], c["mode"], c["alpha"], dtype, window_2d_float32)
    out = dict(loss=float(loss.detach()))
    if grad:
        loss.backward()
        out["grad"] = p.grad.numpy()
    with torch.no_grad():
        m = torch.from_numpy(c["mask"]).to(dtype)
        s = rs.ssim_map(p.detach() * m, torch.from_numpy(c["gt"]).to(dtype) * m, c["window"], c["std"], c["mode"], dtype, window_2d_float32)
    out.update(ssim=s.numpy(), dssim_min=float(((1 - s) / 2).min()), dssim_max=float(((1 - s) / 2).max()))
    return out


_CACHE = {}


def reference64(name, alpha=0.85):
    """The float64 restatement of a case by name (DIBR_NAMES / PHOTO_NAMES), shared by every test of the process; read-only."""
    import torch
    key = (name, alpha)
    if key not in _CACHE:
        r = run_photo(photo_case(name, alpha), torch.float64) if name in PHOTO_CONF else run_dibr(dibr_case(name), torch.float64)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]
