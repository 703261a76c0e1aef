"""Free-view sampling timing: the HIP equi2pers / pers2equi / views_to_erp (csrc/omni_freeview.hip) against a torch-eager restatement of
the reference's functions (equi_pers/equi2pers_torch.py:37, pers2equi_torch.py:37: grid build with asin / atan2 / rotations on every
call + F.grid_sample), both on the same GPU in the same run, by device events over a warm loop.

    python tools/freeview_bench.py [--iters 20] [--out profiles/r09a_freeview.json] [--quick]
    python tools/freeview_bench.py --bwd [--iters 20] [--out profiles/r10a_freeview_bwd.json] [--quick]

--bwd: the backwards of equi_pers.differentiable (csrc/omni_freeview_bwd.hip) against the autograd of the same restatement: for each
operator forward and forward + backward are timed (the input requires grad, `out.backward(G)`), backward = their difference; the HIP
backward also with the option fv_bwd_lds = 0 (global atomics only).

Shapes: B = 8, C = 3, 512 x 1024 <-> 6 cube faces of 256^2, and B = 1, C = 3, 2048 x 4096 <-> 6 x 1024^2.  pers2equi has no batch
dimension (one image per view): the batch rides in its channels (B * C planes per view).  views_to_erp is also timed against
pers2equi + the torch reduction sum_v erp_v / max(sum_v mask_v, 1) it replaces.

Compulsory bytes per call: the input read once and the outputs (with the uint8 mask / count) written once; the fraction printed is
bytes / time / 8 TB/s.  --quick: the small shape, few iterations (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


# ------------------------------------------------------------------ the torch-eager restatement (this project's code)
def torch_rotation(angle, axis):
    axis = F.normalize(axis, dim=-1).reshape(-1, 3)
    a = torch.cos(angle / 2)
    b, c, d = (-axis * torch.sin(angle / 2)[:, None]).unbind(-1)
    rows = [a * a + b * b - c * c - d * d, 2 * (b * c + a * d), 2 * (b * d - a * c),
            2 * (b * c - a * d), a * a + c * c - b * b - d * d, 2 * (c * d + a * b),
            2 * (b * d + a * c), 2 * (c * d - a * b), a * a + d * d - b * b - c * c]
    return torch.stack(rows, -1).reshape(-1, 3, 3)


def torch_rotations(theta, phi):
    R1 = torch_rotation(torch.deg2rad(theta), torch.tensor([0.0, 0.0, 1.0], device=theta.device))
    return R1, torch_rotation(torch.deg2rad(-phi), R1[:, :, 1])


def torch_equi2pers(erp, hfov, wfov, theta, phi, h, w):
    B, _, H, W = erp.shape
    h_len, w_len = math.tan(math.radians(hfov / 2.0)), math.tan(math.radians(wfov / 2.0))
    y = torch.linspace(-w_len, w_len, w)[None, :].repeat(h, 1)                      # built on the host and moved, as the reference does
    z = -torch.linspace(-h_len, h_len, h)[:, None].repeat(1, w)
    x = torch.ones(h, w)
    ray = (torch.stack((x, y, z), -1) / torch.sqrt(x ** 2 + y ** 2 + z ** 2)[..., None]).reshape(-1, 3).T.to(erp.device)
    R1, R2 = torch_rotations(theta, phi)
    N = R1.shape[0]
    ray = torch.matmul(R2, torch.matmul(R1, ray)).transpose(2, 1)
    lat = -torch.asin(ray[..., 2]) / math.pi * 180
    lon = torch.atan2(ray[..., 1], ray[..., 0]) / math.pi * 180
    lon = lon / 180 * ((W - 1) / 2.0) + (W - 1) / 2.0
    lat = lat / 90 * ((H - 1) / 2.0) + (H - 1) / 2.0
    lon = ((lon / W - 0.5) * 2).view(N, h, w).permute(1, 0, 2).reshape(h, N * w)
    lat = ((lat / H - 0.5) * 2).view(N, h, w).permute(1, 0, 2).reshape(h, N * w)
    grid = torch.stack([lon, lat], -1)[None].repeat(B, 1, 1, 1)
    return F.grid_sample(erp, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def torch_pers2equi(pers, hfov, wfov, theta, phi, H, W):
    N, _, h, w = pers.shape
    h_len, w_len = math.tan(math.radians(hfov / 2.0)), math.tan(math.radians(wfov / 2.0))
    lat, lon = torch.meshgrid(torch.linspace(90, -90, H), torch.linspace(-180, 180, W), indexing="ij")
    lat, lon = torch.deg2rad(lat), torch.deg2rad(lon)
    ray = torch.stack((torch.cos(lon) * torch.cos(lat), torch.sin(lon) * torch.cos(lat), torch.sin(lat)), 2)
    ray = ray[None].repeat(N, 1, 1, 1).to(pers.device).view(N, H * W, 3).transpose(2, 1)
    R1, R2 = torch_rotations(theta, phi)
    ray = torch.matmul(torch.inverse(R1), torch.matmul(torch.inverse(R2), ray)).transpose(2, 1).view(N, H, W, 3)
    front = ray[..., 0] > 0
    ray = ray / ray[..., 0:1]
    y, z = ray[..., 1], ray[..., 2]
    inside = (-w_len < y) & (y < w_len) & (-h_len < z) & (z < h_len)
    zero = torch.zeros((), device=pers.device)
    u = torch.where(inside, (y + w_len) / 2 / w_len * float(w), zero)
    v = torch.where(inside, (-z + h_len) / 2 / h_len * float(h), zero)
    grid = torch.stack([(u / w - 0.5) * 2, (v / h - 0.5) * 2], -1)
    mask = (inside & front).to(torch.int64)[:, None]
    return F.grid_sample(pers, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * mask, mask


def reduce_views(erps, masks, B, C):
    """[N, B*C, H, W], [N,1,H,W] -> [B,C,H,W]: the torch reduction views_to_erp replaces."""
    out = erps.sum(0) / masks.sum(0).clamp(min=1).to(erps.dtype)
    return out.view(B, C, *out.shape[-2:])


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


def main_bwd(a):
    from omnifusion_amd import _lib
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.equi_pers import cubemap_views
    from omnifusion_amd.equi_pers import differentiable as fv
    cases = [(8, 3, 512, 1024, 256)] if a.quick else [(8, 3, 512, 1024, 256), (1, 3, 2048, 4096, 1024)]
    iters = 3 if a.quick else a.iters
    theta, phi = cubemap_views()
    theta_d, phi_d = theta.to(DEV), phi.to(DEV)
    N, fov = 6, 90.0
    rows = []
    for B, C, H, W, P in cases:
        g = torch.Generator(device=DEV).manual_seed(1)
        erp = torch.rand(B, C, H, W, device=DEV, generator=g)
        views = torch.rand(B, N, C, P, P, device=DEV, generator=g)
        folded = views.permute(1, 0, 2, 3, 4).reshape(N, B * C, P, P).contiguous()          # pers2equi's [N, planes, h, w]
        legs = {
            "equi2pers": (lambda x: fv.equi2pers_planar(x, fov, fov, theta, phi, P, P),
                          lambda x: torch_equi2pers(x, fov, fov, theta_d, phi_d, P, P).view(B, C, P, N, P).permute(0, 3, 1, 2, 4), erp),
            "pers2equi": (lambda x: fv.pers2equi(x, fov, fov, theta, phi, H, W)[0], lambda x: torch_pers2equi(x, fov, fov, theta_d, phi_d, H, W)[0], folded),
            "views_to_erp": (lambda x: fv.views_to_erp(x, fov, fov, theta, phi, H, W)[0],
                             lambda x: reduce_views(*torch_pers2equi(x.permute(1, 0, 2, 3, 4).reshape(N, B * C, P, P), fov, fov, theta_d, phi_d, H, W), B, C), views),
        }
        for name, (hip, ref, x0) in legs.items():
            x = x0.clone().requires_grad_(True)
            with torch.no_grad():
                G = torch.rand(hip(x0).shape, device=DEV, generator=g) * 2 - 1

            def both(f):
                x.grad = None
                f(x).backward(G)
                return x.grad

            def fwd(f):
                with torch.no_grad():
                    return f(x0)
            gh, gt = both(hip).clone(), both(ref).clone()
            rel = float((gh - gt).abs().max() / gt.abs().max())
            t = {}
            for tag, f, n in (("hip", hip, iters), ("torch", ref, max(2, iters // 4))):
                t[tag + "_fwd"] = timeit(lambda: fwd(f), n)
                t[tag + "_both"] = timeit(lambda: both(f), n)
            _lib.set_option("fv_bwd_lds", 0)
            try:
                same = bool(torch.equal(both(hip), gh))
                t["hip_both_global"] = timeit(lambda: both(hip), iters)
            finally:
                _lib.set_option("fv_bwd_lds", 1)
            us = lambda v: round(v * 1e6, 1)
            hb, tb = t["hip_both"] - t["hip_fwd"], t["torch_both"] - t["torch_fwd"]
            row = dict(op=name, B=B, C=C, H=H, W=W, views=N, view_size=P, hip_fwd_us=us(t["hip_fwd"]), hip_fwd_bwd_us=us(t["hip_both"]), hip_bwd_us=us(hb),
                       hip_bwd_global_atomics_only_us=us(t["hip_both_global"] - t["hip_fwd"]), global_only_same_bits=same,
                       torch_eager_fwd_us=us(t["torch_fwd"]), torch_eager_fwd_bwd_us=us(t["torch_both"]), torch_eager_bwd_us=us(tb),
                       speedup_bwd=round(tb / hb, 2), speedup_fwd_bwd=round(t["torch_both"] / t["hip_both"], 2), max_rel_diff_vs_torch=rel)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), iters=iters, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "freeview_bench measures on an MI355X; there is no CPU timing"
    if a.bwd:
        return main_bwd(a)
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.equi_pers import _freeview, cubemap_views, views_to_erp
    from omnifusion_amd.equi_pers.equi2pers_torch import equi2pers_planar
    cases = [(8, 3, 512, 1024, 256)] if a.quick else [(8, 3, 512, 1024, 256), (1, 3, 2048, 4096, 1024)]
    iters = 3 if a.quick else a.iters
    theta, phi = cubemap_views()
    theta_d, phi_d = theta.to(DEV), phi.to(DEV)
    N, fov = 6, 90.0
    rows = []
    for B, C, H, W, P in cases:
        g = torch.Generator(device=DEV).manual_seed(1)
        erp = torch.rand(B, C, H, W, device=DEV, generator=g)
        views = torch.rand(B, N, C, P, P, device=DEV, generator=g)
        folded = views.permute(1, 0, 2, 3, 4).reshape(N, B * C, P, P).contiguous()          # pers2equi's [N, planes, h, w]
        ne, nv = B * C * H * W, B * N * C * P * P

        def hip_p2e():
            return _freeview.launch_pers2equi(folded, fov, fov, theta, phi, H, W)

        def hip_p2e_reduce():
            e, m = hip_p2e()
            return reduce_views(e, m, B, C)

        def torch_e2p():
            return torch_equi2pers(erp, fov, fov, theta_d, phi_d, P, P)

        def torch_p2e():
            return torch_pers2equi(folded, fov, fov, theta_d, phi_d, H, W)

        def torch_merge():
            return reduce_views(*torch_p2e(), B, C)
        legs = {
            "equi2pers": (lambda: equi2pers_planar(erp, fov, fov, theta, phi, P, P), torch_e2p, 4 * ne + 4 * nv,
                          lambda x, y: (x - y.view(B, C, P, N, P).permute(0, 3, 1, 2, 4)).abs().max()),
            "pers2equi": (hip_p2e, torch_p2e, 4 * nv + 4 * N * ne + N * H * W, lambda x, y: (x[0] - y[0]).abs().max()),
            "views_to_erp": (lambda: views_to_erp(views, fov, fov, theta, phi, H, W), torch_merge, 4 * nv + 4 * ne + H * W,
                             lambda x, y: (x[0] - y).abs().max()),
        }
        for name, (hip, ref, nbytes, diff) in legs.items():
            dmax = float(diff(hip(), ref()))
            th = timeit(hip, iters)
            tt = timeit(ref, max(2, iters // 4))
            row = dict(op=name, B=B, C=C, H=H, W=W, views=N, view_size=P, hip_us=round(th * 1e6, 1), torch_eager_us=round(tt * 1e6, 1),
                       speedup=round(tt / th, 2), compulsory_bytes=nbytes, hip_frac_of_8TBps=round(nbytes / th / 8e12, 4), max_abs_diff_vs_torch=dmax)
            if name == "views_to_erp":
                tr = timeit(hip_p2e_reduce, iters)
                row.update(hip_pers2equi_plus_torch_reduction_us=round(tr * 1e6, 1), speedup_vs_unmerged=round(tr / th, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), iters=iters, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
