"""DIBR timing: the HIP render / dibr_vertical / dibr_horizontal (csrc/omni_dibr.hip) against a torch-eager restatement of the
reference's algorithm (supervision/splatting.py:9-80 + util.py:384-413: per-channel scatter_add_ of four corners, element-wise passes),
both on the same GPU in the same run, by device events over a warm loop.

    python tools/dibr_bench.py [--iters 20] [--out profiles/r07b_dibr.json] [--quick]
    python tools/dibr_bench.py --bwd [--out profiles/r08a_view_synthesis_bwd.json] [--quick]

--bwd: forward + backward of the three operators (gradients for every differentiable input) and the photometric loss forward /
forward + backward, against the autograd of the same torch-eager restatements (B = 8, C = 3; 512 x 1024 and 256 x 512; smooth and
noise inputs).  The backward alone is the difference of the two legs.

Compulsory bytes per call: image + depth (+ coords for render, + both [1,2,H,W] grids for DIBR) read once, recon + mask written once;
the fraction printed is bytes / time / 8 TB/s.  --quick: one shape, few iterations (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


# ------------------------------------------------------------------ the torch-eager restatement (this project's code)
def torch_splat(values, coords, out):
    b, c, h, w = out.shape
    u, v = coords[:, 0:1], coords[:, 1:2]
    u0, v0 = torch.floor(u), torch.floor(v)
    u1, v1 = u0 + 1, v0 + 1
    u0c, v0c, u1c, v1c = u0.clamp(0.0, w - 1), v0.clamp(0.0, h - 1), u1.clamp(0.0, w - 1), v1.clamp(0.0, h - 1)
    wu0 = (u1 - u) * (u0 == u0c).to(values.dtype)
    wu1 = (u - u0) * (u1 == u1c).to(values.dtype)
    wv0 = (v1 - v) * (v0 == v0c).to(values.dtype)
    wv1 = (v - v0) * (v1 == v1c).to(values.dtype)
    corners = [(wu0 * wv0, u0c, v0c), (wu1 * wv0, u1c, v0c), (wu0 * wv1, u0c, v1c), (wu1 * wv1, u1c, v1c)]
    corners = [(cw * (cw >= 1e-3).to(values.dtype), cu, cv) for cw, cu, cv in corners]
    for ch in range(c):                                                   # the reference recomputes the indices per channel
        flat = out[:, ch].reshape(b, -1)
        for cw, cu, cv in corners:
            flat.scatter_add_(1, (cu + cv * w).reshape(b, -1).long(), (values[:, ch:ch + 1] * cw).reshape(b, -1))
        out[:, ch] = flat.view(b, h, w)


def torch_render(img, depth, coords, max_depth):
    wts = 1.0 / torch.exp(2 * depth / max_depth)
    acc, wacc = torch.zeros_like(img), torch.zeros_like(depth)
    torch_splat(img * wts, coords, acc)
    torch_splat(wts, coords, wacc)
    recon = acc / (wacc + 1e-8 * (wacc <= 1e-8).to(img.dtype))
    return recon, wacc > 1e-3


def torch_dibr(depth, img, uv, sg, baseline, mode):
    h = depth.shape[2]
    ph, th = sg[:, 0:1], sg[:, 1:2]
    if mode == 0:
        dth = torch.cos(th) * baseline / depth * (h / np.pi)
        dth[~torch.isfinite(dth)] = 0.0
        coords = uv + torch.cat((torch.zeros_like(depth), dth), 1)
    else:
        dph = torch.clamp(torch.sin(ph) / (depth * torch.cos(th)) * baseline * (h / np.pi), -h, h)
        dph[~torch.isfinite(dph)] = 0.0
        dth = torch.clamp(torch.cos(ph) * torch.sin(th) * baseline / depth * (h / np.pi), 0, h)
        coords = uv + torch.cat((dph, dth), 1)
        coords[:, 0] = torch.fmod(coords[:, 0] + 512, 512)
    coords[~torch.isfinite(coords)] = 0
    return torch_render(img, depth, coords, 8.0)[0]


def torch_photometric(pred, gt, mask, weights, window=7, std=1.5, alpha=0.85):
    """The reference's algorithm in stock torch ops (supervision/photometric.py:34-51 with the gaussian SSIM of ssim.py:23-63)."""
    import math
    C = pred.shape[1]
    g = torch.tensor([math.exp(-(x - window // 2) ** 2 / float(2 * std ** 2)) for x in range(window)], dtype=torch.float64)
    g = (g / g.sum()).float().to(pred.device)
    k = torch.outer(g, g)[None, None].expand(C, 1, window, window).contiguous()
    x, y = pred * mask, gt * mask
    win = lambda z: torch.nn.functional.conv2d(z, k, padding=window // 2, groups=C)
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    ssim = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    loss = (torch.clamp((1 - ssim) / 2, 0, 1) * alpha + (y - x).abs() * (1 - alpha)) * mask * weights
    return torch.mean(loss.sum(dim=[1, 2, 3], keepdim=True) / mask.sum(dim=[1, 2, 3], keepdim=True))


def bench_bwd(a):
    from omnifusion_amd import spherical
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    from omnifusion_amd.supervision.splatting import render
    from omnifusion_amd.util import dibr_horizontal, dibr_vertical
    cases = [(8, 3, 512, 1024, "smooth")] if a.quick else [(8, 3, 512, 1024, "smooth"), (8, 3, 256, 512, "smooth"), (8, 3, 512, 1024, "noise"),
                                                             (8, 3, 256, 512, "noise")]
    iters = 3 if a.quick else a.iters
    rows = []
    for B, C, H, W, kind in cases:
        g = torch.Generator(device=DEV).manual_seed(1)

        def field(ch):
            if kind == "noise":
                return torch.rand(B, ch, H, W, device=DEV, generator=g)
            low = torch.rand(B, ch, H // 32 + 1, W // 32 + 1, device=DEV, generator=g)
            return torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).contiguous()
        img = torch.rand(B, C, H, W, device=DEV, generator=g).requires_grad_(True)
        depth = (0.5 + 7.5 * field(1)).requires_grad_(True)
        uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
        coords = (uv + 20.0 * (field(2) - 0.5)).contiguous().requires_grad_(True)
        G = torch.rand(B, C, H, W, device=DEV, generator=g) - 0.5
        gt = torch.rand(B, C, H, W, device=DEV, generator=g)
        ones = torch.ones(B, 1, H, W, device=DEV)
        params = PhotometricLossParameters()

        def fb(fn, inputs):
            return lambda: torch.autograd.grad(fn(), inputs, G)
        legs = {
            "render": (lambda: render(img, depth, coords, 8.0)[0], lambda: torch_render(img, depth, coords, 8.0)[0], [img, depth, coords]),
            "dibr_vertical": (lambda: dibr_vertical(depth, img, uv, sg, 0.26), lambda: torch_dibr(depth, img, uv, sg, 0.26, 0), [img, depth]),
            "dibr_horizontal": (lambda: dibr_horizontal(depth, img, uv, sg, 0.26), lambda: torch_dibr(depth, img, uv, sg, 0.26, 1), [img, depth]),
        }
        for name, (hip, ref, inputs) in legs.items():
            gh, gr = fb(hip, inputs)(), fb(ref, inputs)()
            dmax = max(float(torch.nan_to_num(x - y).abs().max() / y[torch.isfinite(y)].abs().max()) for x, y in zip(gh, gr))
            with torch.no_grad():
                tf_h, tf_t = timeit(hip, iters), timeit(ref, max(2, iters // 4))
            t_h, t_t = timeit(fb(hip, inputs), iters), timeit(fb(ref, inputs), max(2, iters // 4))
            row = dict(op=name, inputs=kind, B=B, C=C, H=H, W=W, hip_fwd_us=round(tf_h * 1e6, 1), hip_fwd_bwd_us=round(t_h * 1e6, 1),
                       hip_bwd_us=round((t_h - tf_h) * 1e6, 1), torch_fwd_us=round(tf_t * 1e6, 1), torch_fwd_bwd_us=round(t_t * 1e6, 1),
                       torch_bwd_us=round((t_t - tf_t) * 1e6, 1), speedup_fwd_bwd=round(t_t / t_h, 2),
                       speedup_bwd=round((t_t - tf_t) / max(t_h - tf_h, 1e-9), 2), max_rel_grad_diff_vs_torch=dmax)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if kind == "smooth":
            pred = img
            hip = lambda: calculate_loss(pred, gt, params, ones, ones)
            ref = lambda: torch_photometric(pred, gt, ones, ones)
            fbl = lambda fn: (lambda: torch.autograd.grad(fn(), pred))
            dmax = float((fbl(hip)()[0] - fbl(ref)()[0]).abs().max() / fbl(ref)()[0].abs().max())
            with torch.no_grad():
                tf_h, tf_t = timeit(hip, iters), timeit(ref, max(2, iters // 4))
            t_h, t_t = timeit(fbl(hip), iters), timeit(fbl(ref), max(2, iters // 4))
            row = dict(op="photometric_loss", inputs="noise", B=B, C=C, H=H, W=W, hip_fwd_us=round(tf_h * 1e6, 1), hip_fwd_bwd_us=round(t_h * 1e6, 1),
                       hip_bwd_us=round((t_h - tf_h) * 1e6, 1), torch_fwd_us=round(tf_t * 1e6, 1), torch_fwd_bwd_us=round(t_t * 1e6, 1),
                       torch_bwd_us=round((t_t - tf_t) * 1e6, 1), speedup_fwd_bwd=round(t_t / t_h, 2),
                       speedup_bwd=round((t_t - tf_t) / max(t_h - tf_h, 1e-9), 2), loss_diff_vs_torch=abs(float(hip().detach()) - float(ref().detach())),
                       max_rel_grad_diff_vs_torch=dmax)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), iters=iters, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dibr_bench measures on an MI355X; there is no CPU timing"
    if a.bwd:
        return bench_bwd(a)
    from omnifusion_amd import spherical
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.supervision.splatting import render
    from omnifusion_amd.util import HORIZONTAL, VERTICAL, _dibr
    # "smooth": depth and render displacement are low-frequency fields (bilinear up-sampling of a 1/32-size random grid) — the shape
    # of a real depth map, under which a tile's targets stay close together; "noise": i.i.d. per pixel, the worst case of scattered targets
    cases = [(8, 3, 512, 1024, "smooth")] if a.quick else [(8, 3, 512, 1024, "smooth"), (8, 3, 256, 512, "smooth"), (8, 3, 512, 1024, "noise")]
    iters = 3 if a.quick else a.iters
    rows = []
    for B, C, H, W, kind in cases:
        g = torch.Generator(device=DEV).manual_seed(1)

        def field(ch):
            if kind == "noise":
                return torch.rand(B, ch, H, W, device=DEV, generator=g)
            low = torch.rand(B, ch, H // 32 + 1, W // 32 + 1, device=DEV, generator=g)
            return torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).contiguous()
        img = torch.rand(B, C, H, W, device=DEV, generator=g)
        depth = 0.5 + 7.5 * field(1)
        uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
        coords = (uv + 20.0 * (field(2) - 0.5)).contiguous()
        n = B * H * W
        base = 4 * n * C + 4 * n + 4 * n * C + n                          # img + depth read, recon + uint8 mask written
        legs = {
            "render": (lambda: render(img, depth, coords, 8.0), lambda: torch_render(img, depth, coords, 8.0),
                       base + 8 * n),
            "dibr_vertical": (lambda: _dibr(depth, img, uv, sg, 0.26, VERTICAL, want_mask=True),
                              lambda: torch_dibr(depth, img, uv, sg, 0.26, 0), base + 2 * 8 * H * W),
            "dibr_horizontal": (lambda: _dibr(depth, img, uv, sg, 0.26, HORIZONTAL, want_mask=True),
                                lambda: torch_dibr(depth, img, uv, sg, 0.26, 1), base + 2 * 8 * H * W),
        }
        for name, (hip, ref, nbytes) in legs.items():
            got, want = hip()[0], ref()
            want = want[0] if isinstance(want, tuple) else want
            dmax = float((got - want).abs().max())
            th = timeit(hip, iters)
            tt = timeit(ref, max(2, iters // 4))
            row = dict(op=name, inputs=kind, B=B, C=C, H=H, W=W, hip_us=round(th * 1e6, 1), torch_eager_us=round(tt * 1e6, 1),
                       speedup=round(tt / th, 2), compulsory_bytes=nbytes, hip_frac_of_8TBps=round(nbytes / th / 8e12, 4),
                       max_abs_diff_vs_torch=dmax)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), iters=iters, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
