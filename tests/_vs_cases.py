"""Seeded inputs of the view-synthesis backward fixtures: G15a-e (the gradients of render / dibr_* for the G14a-e inputs,
tools/gen_golden_dibr_bwd.py) and G16a-c (the photometric loss and its gradient, tools/gen_golden_photometric.py).  The tests
regenerate the same inputs; only the reference's results and float64 input checksums are stored in tests/golden/."""
import numpy as np

import _dibr_cases as dc
from _util import rng_uniform, smooth_erp

# ------------------------------------------------------------------ G15: DIBR / render backward
DIBR_NAMES = ("G15a", "G15b", "G15c", "G15d", "G15e")


def dibr_case(name):
    """G15x = the G14x inputs + the upstream gradient dL/drecon = smooth_erp(77, B, C, H, W) - 0.5."""
    c = dc.case("G14" + name[-1])
    B, C, H, W = c["img"].shape
    c["grad_out"] = (smooth_erp(77, B, C, H, W) - 0.5).astype(np.float32)
    return c


def dibr_grad_names(c):
    return ("img", "depth", "coords") if c["kind"] == "render" else ("img", "depth")


def _reference_modules():
    import os
    import sys
    import torch
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    if root not in sys.path:
        sys.path.insert(0, root)
    import spherical as S360                                                 # the reference's packages (pure torch)
    import supervision as L
    # util.py imports the whole model zoo at module level: its two DIBR functions are exec'd alone (executed here only, never stored)
    src = open(os.path.join(root, "util.py")).read()
    ns = {"torch": torch, "S360": S360, "L": L}
    exec(compile(src[src.index("def dibr_vertical"):src.index("def get_sobel_kernel")], "util_dibr", "exec"), ns)
    return S360, L, ns


def reference_dibr_forward(c, dtype, tensors=None):
    """The reference's own render / dibr_* on the CPU in `dtype` (needs the reference checkout; test infrastructure only).
    -> (recon, dict of the leaf tensors that require grad).  `tensors` overrides inputs by name (numpy arrays)."""
    import torch
    S360, L, ns = _reference_modules()
    src = dict(c, **(tensors or {}))
    leaf = {k: torch.from_numpy(np.ascontiguousarray(src[k])).to(dtype).requires_grad_(True) for k in dibr_grad_names(c)}
    if c["kind"] == "render":
        recon, _ = L.splatting.render(leaf["img"], leaf["depth"], leaf["coords"], max_depth=c["max_depth"])
        return recon, leaf
    B, C, H, W = c["img"].shape
    uvgrid = S360.create_image_grid(W, H).to(dtype)                          # the float32 grids the device reads, widened
    sgrid = S360.create_spherical_grid(W).to(dtype)
    fn = ns["dibr_vertical" if c["kind"] == "vertical" else "dibr_horizontal"]
    return fn(leaf["depth"], leaf["img"], uvgrid, sgrid, c["baseline"]), leaf


def reference_dibr_grads(c, dtype):
    """-> dict name -> gradient (numpy, `dtype`) of sum(recon * grad_out) by the reference's autograd."""
    import torch
    recon, leaf = reference_dibr_forward(c, dtype)
    recon.backward(torch.from_numpy(c["grad_out"]).to(dtype))
    return {k: v.grad.numpy() for k, v in leaf.items()}


def rel_error(got, want64):
    """The error measure of the parity gates: |g - g_ref64| / max|g_ref64| over the elements where the reference is finite (others: 0)."""
    got = np.asarray(got, np.float64); want = np.asarray(want64, np.float64)
    ok = np.isfinite(want)
    scale = np.abs(want[ok]).max()
    return np.where(ok, np.abs(np.where(ok, got, 0.0) - np.where(ok, want, 0.0)), 0.0) / scale


# ------------------------------------------------------------------ G16: photometric loss
PHOTO_NAMES = ("G16a", "G16b", "G16c")
PHOTO_CONF = {                      # window, std, mode, channels of the mask
    "G16a": (7, 1.5, "gaussian", 1),
    "G16b": (5, 1.5, "gaussian", 3),
    "G16c": (3, 1.5, "box", 1),
}


def photo_case(name):
    """-> dict(pred, gt, mask, weights, window, std, mode, alpha): two views of one smooth scene that differ by a smooth field and a
    little texture, a random validity mask (about 90 % ones; [B,1,H,W] or [B,C,H,W]) and smooth positive weights."""
    k = PHOTO_NAMES.index(name)
    B, C, H, W = 2, 3, 64, 128
    window, std, mode, mask_c = PHOTO_CONF[name]
    s = 1600 + 10 * k
    gt = (0.15 + 0.7 * smooth_erp(s + 1, B, C, H, W, k=9) + 0.06 * (rng_uniform(s + 2, (B, C, H, W)) - 0.5)).astype(np.float32)
    pred = (gt + 0.2 * (smooth_erp(s + 3, B, C, H, W, k=15) - 0.5) + 0.06 * (rng_uniform(s + 4, (B, C, H, W)) - 0.5)).astype(np.float32)
    mask = (rng_uniform(s + 5, (B, mask_c, H, W)) < 0.9).astype(np.float32)
    weights = (0.5 + smooth_erp(s + 6, B, 1, H, W)).astype(np.float32)
    return dict(pred=pred, gt=gt, mask=mask, weights=weights, window=window, std=std, mode=mode, alpha=0.85)


def reference_photo(c, dtype, pred=None):
    """The reference's calculate_loss on the CPU in `dtype` -> (loss tensor, pred leaf, min and max of (1 - ssim) / 2)."""
    import torch
    _, L, _ = _reference_modules()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    p = t(c["pred"] if pred is None else pred).requires_grad_(True)
    params = L.photometric.PhotometricLossParameters(alpha=c["alpha"], window=c["window"], std=c["std"], ssim_mode=c["mode"])
    loss = L.photometric.calculate_loss(p, t(c["gt"]), params, t(c["mask"]), t(c["weights"]))
    with torch.no_grad():
        m = t(c["mask"])
        h = (1 - L.ssim.ssim_loss(p * m, t(c["gt"]) * m, kernel_size=c["window"], std=c["std"], mode=c["mode"])) / 2
    return loss, p, float(h.min()), float(h.max())


def checksums(c):
    return {k: np.float64(np.asarray(v, np.float64).sum()) for k, v in c.items() if isinstance(v, np.ndarray)}


# ------------------------------------------------------------------ structure checks: smooth inputs, no zero block
def direction_case(kind):
    """Smooth inputs and smooth unit-scale directions for the directional-derivative check of `kind` ('render', 'vertical',
    'horizontal'): L(x) = sum(recon(x) * grad_out) along x + h v for x = (img, depth[, coords]) jointly."""
    B, C, H, W = 2, 3, 64, 128
    c = dict(kind=kind, img=smooth_erp(1501, B, C, H, W), depth=dc.smooth_depth(1502, B, H, W), baseline=dc.BASELINE, max_depth=8.0)
    c["grad_out"] = (smooth_erp(1503, B, C, H, W) - 0.5).astype(np.float32)
    v = dict(img=(smooth_erp(1504, B, C, H, W) - 0.5).astype(np.float32), depth=(smooth_erp(1505, B, 1, H, W) - 0.5).astype(np.float32))
    if kind == "render":
        disp = (smooth_erp(1506, B, 2, H, W) - 0.5) * np.array([24.0, 12.0], np.float32)[None, :, None, None]
        c["coords"] = (dc.image_grid(H, W) + disp).astype(np.float32)
        v["coords"] = (smooth_erp(1507, B, 2, H, W) - 0.5).astype(np.float32)
    return c, v


def directional_residual(loss_of, grads, x, v, h):
    """|central difference - <grad, v>| / |<grad, v>| with L evaluated by `loss_of(dict of float32 arrays) -> float`."""
    plus = {k: (x[k].astype(np.float64) + h * v[k]).astype(np.float32) for k in v}
    minus = {k: (x[k].astype(np.float64) - h * v[k]).astype(np.float32) for k in v}
    # the step actually taken after rounding to float32
    dot = sum(float((np.asarray(grads[k], np.float64) * (plus[k].astype(np.float64) - minus[k].astype(np.float64))).sum()) for k in v)
    fd = loss_of(plus) - loss_of(minus)
    return abs(fd - dot) / abs(dot), fd, dot


def e2e_case():
    """Depth refinement by view synthesis at 128 x 256: (image, true depth, starting depth = true * (1 + 0.15 * smooth noise))."""
    B, C, H, W = 1, 3, 128, 256
    img = (0.1 + 0.8 * smooth_erp(1511, B, C, H, W, k=9)).astype(np.float32)
    true = (1.0 + 5.0 * smooth_erp(1512, B, 1, H, W)).astype(np.float32)
    start = (true * (1.0 + 0.15 * (2.0 * smooth_erp(1513, B, 1, H, W) - 1.0))).astype(np.float32)
    return img, true, start


E2E_STEPS, E2E_LR, E2E_BASELINE = 30, 0.05, 0.26
