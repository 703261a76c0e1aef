"""A plain restatement of the view-synthesis operators in stock torch on the CPU, float32 or float64, differentiable by stock autograd:
the yardstick of tests/test_vs_shapes_gpu.py at shapes no fixture covers.  Restated from DESIGN.md §11 and the header comments of
csrc/omni_dibr.hip and csrc/omni_photometric.hip; tests/test_vs_restatement_cpu.py first proves it against the fixtures G14 - G16.

    render(img, depth, coords, max_depth, dtype)                       -> recon, mask, wsum
    dibr(kind, depth, img, uvgrid, sgrid, baseline, dtype)             -> recon                 kind: 'vertical' | 'horizontal'
    photometric(pred, gt, mask, weights, window, std, mode, alpha, dtype) -> loss (scalar)
    ssim_map(x, y, window, std, mode, dtype)                           -> the SSIM map [B,C,H,W]

Inputs are numpy arrays or tensors; a tensor that requires grad stays the leaf it is (it must already be of `dtype`).

The documented quirks, kept: corner weights below 1e-3 are dropped and corners off the image gated out (both gates are constants of
the backward); a non-finite displacement becomes 0 and a non-finite coordinate the ABSOLUTE coordinate 0; the horizontal mode clamps
d phi to [-H, H] and d theta to [0, H] (a NaN d theta passes the clamp) and wraps u modulo the literal 512; den = w + 1e-8 (w <= 1e-8);
the 'box' SSIM map is zero-padded by window // 2; the Gaussian window is built in float64, stored as float32 and widened.  A render
coordinate that is not finite drops its source, as the kernel does.  Where depth == 0 stock autograd gives NaN for the depth gradient of
the DIBR modes (0 * inf behind the clean-up) — the reference does too; the device gives 0 there."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _t(a, dtype):
    if isinstance(a, torch.Tensor):
        return a if a.dtype == dtype else a.to(dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def corners(u, v, H, W):
    """The four corners of the bilinear splat of sources at (u, v) [B,1,H,W]: a list of (weight, column, row) with the in-image and
    1e-3 gates applied to the weight (gates detached) and the indices clamped into the image (a clamped corner has weight 0)."""
    u0, v0 = torch.floor(u), torch.floor(v)
    u1, v1 = u0 + 1, v0 + 1
    inside = lambda x, n: ((x >= 0) & (x <= n - 1)).to(u.dtype)
    u0w, u1w = (u1 - u) * inside(u0, W), (u - u0) * inside(u1, W)
    v0w, v1w = (v1 - v) * inside(v0, H), (v - v0) * inside(v1, H)
    out = []
    for uw, vw, cu, cv in ((u0w, v0w, u0, v0), (u1w, v0w, u1, v0), (u0w, v1w, u0, v1), (u1w, v1w, u1, v1)):
        cw = uw * vw
        cw = cw * (cw >= 1e-3).to(u.dtype)
        out.append((cw, cu.clamp(0, W - 1).long(), cv.clamp(0, H - 1).long()))
    return out


def _splat(values, cs, H, W):
    B, C = values.shape[:2]
    out = torch.zeros(B, C, H * W, dtype=values.dtype)
    for cw, cu, cv in cs:
        idx = (cv * W + cu).reshape(B, 1, H * W).expand(B, C, H * W)
        out = out.scatter_add(2, idx, (values * cw).reshape(B, C, H * W))
    return out.view(B, C, H, W)


def render(img, depth, coords, max_depth=20.0, dtype=torch.float64):
    img, depth, coords = _t(img, dtype), _t(depth, dtype), _t(coords, dtype)
    B, C, H, W = img.shape
    u, v = coords[:, 0:1], coords[:, 1:2]
    ok = torch.isfinite(u) & torch.isfinite(v)                    # a source without a finite coordinate is dropped
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    cs = [(cw * ok.to(dtype), cu, cv) for cw, cu, cv in corners(u, v, H, W)]
    w = 1.0 / torch.exp(2 * depth / max_depth)
    acc, wsum = _splat(img * w, cs, H, W), _splat(w, cs, H, W)
    recon = acc / (wsum + 1e-8 * (wsum <= 1e-8).to(dtype))
    return recon, (wsum > 1e-3).detach(), wsum


def dibr_coords(kind, depth, uvgrid, sgrid, baseline, dtype=torch.float64):
    """The target coordinates [B,2,H,W] of dibr_vertical / dibr_horizontal (uvgrid, sgrid: the float32 grids, widened)."""
    depth, uv, sg = _t(depth, dtype), _t(uvgrid, dtype), _t(sgrid, dtype)
    H = depth.shape[2]
    ph, th = sg[:, 0:1], sg[:, 1:2]
    clean = lambda x: torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    if kind == "vertical":
        dth = clean(torch.cos(th) * baseline / depth * (H / math.pi))
        u, v = uv[:, 0:1] + torch.zeros_like(depth), uv[:, 1:2] + dth
    elif kind == "horizontal":
        dph = clean(torch.clamp(torch.sin(ph) / (depth * torch.cos(th)) * baseline * (H / math.pi), -H, H))
        dth = torch.clamp(torch.cos(ph) * torch.sin(th) * baseline / depth * (H / math.pi), 0, H)
        u, v = torch.fmod(uv[:, 0:1] + dph + 512, 512), uv[:, 1:2] + dth
    else:
        raise KeyError(kind)
    return torch.cat((clean(u), clean(v)), 1)


def dibr(kind, depth, img, uvgrid, sgrid, baseline, dtype=torch.float64):
    depth = _t(depth, dtype)
    return render(img, depth, dibr_coords(kind, depth, uvgrid, sgrid, baseline, dtype), 8.0, dtype)[0]


def window_1d(window, std, dtype):
    g = np.array([math.exp(-(x - window // 2) ** 2 / float(2 * std ** 2)) for x in range(window)])
    return torch.from_numpy((g / g.sum()).astype(np.float32)).to(dtype)


def ssim_map(x, y, window=5, std=1.5, mode="gaussian", dtype=torch.float64, window_2d_float32=False):
    """window_2d_float32: the 2-D Gaussian as the REFERENCE builds it, the product of the float32 1-D values rounded to float32 (one more
    rounding of every weight than the kernel's separable float64 product) — for the comparison with the reference only."""
    x, y = _t(x, dtype), _t(y, dtype)
    C, r = x.shape[1], window // 2
    if mode == "gaussian":
        g = window_1d(window, std, dtype)
        k = (torch.outer(g.float(), g.float()).to(dtype) if window_2d_float32 else torch.outer(g, g))[None, None].expand(C, 1, window, window).contiguous()
        win = lambda z: F.conv2d(z, k, padding=r, groups=C)
    elif mode == "box":
        win = lambda z: F.avg_pool2d(z, window, stride=1)
    else:
        raise KeyError(mode)
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    return F.pad(s, (r, r, r, r)) if mode == "box" else s


def photometric(pred, gt, mask, weights, window=7, std=1.5, mode="gaussian", alpha=0.85, dtype=torch.float64, window_2d_float32=False):
    pred, gt, mask, weights = _t(pred, dtype), _t(gt, dtype), _t(mask, dtype), _t(weights, dtype)
    x, y = pred * mask, gt * mask
    dss = torch.clamp((1 - ssim_map(x, y, window, std, mode, dtype, window_2d_float32)) / 2, 0, 1)
    loss = (dss * alpha + (y - x).abs() * (1 - alpha)) * mask * weights
    return torch.mean(loss.sum(dim=[1, 2, 3]) / mask.sum(dim=[1, 2, 3]))
