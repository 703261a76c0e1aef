"""Plane-fit normals timing: the HIP map (equi_pers.depth2normal) and loss (supervision.geometry.planefit_normal_loss), forward and forward +
backward (csrc/omni_planefit.hip), against a torch-eager restatement of the reference's formulation (equi_pers/depth2normal.py: unfold to
[B,75,H W], a [B,H,W,25,3] matrix and its transpose, batched matmul, det, where, inv, two more matmuls, autograd) on the same GPU in the same run.

    python tools/planefit_bench.py [--rounds 5] [--iters 10] [--eager-iters 2] [--out profiles/r16a_planefit.json] [--quick]

Method (as tools/geometry_bench.py): device events over warm loops; the legs ALTERNATE (every round times each leg once, the median over the
rounds is reported with the spread) and every call of a loop takes the next of `--bufs` copies of the inputs.  The eager legs run
`--eager-iters` calls per round: one call is hundreds of milliseconds.

Shape: B = 8 at 512 x 1024, hole-free smooth ground truth, pred = gt + a smooth perturbation, an 80 % random float mask.
Compulsory bytes: map forward = depth read + three planes written, 16 B per pixel; map backward = depth + upstream read + gradient written, 20 B;
loss forward = pred + gt + mask read, 12 B; loss backward = the same three read + the gradient written, 16 B.  The fraction printed is
bytes / time / 8 TB/s.  Peak memory: torch.cuda.max_memory_allocated over one forward + backward of each form, above what the inputs hold.
Parity: the map and the loss against the eager form in float64 on the device, on the first timed input (B = 1 of it: float64 eager holds 2.5 GB per item).
--quick: B = 1, few iterations.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.geometry_bench import DEV, make_inputs, time_loop  # noqa: E402


def eager_normals(depth, rays):
    """The reference's formulation in stock torch operations, in depth's dtype: rays [1,3,H,W] of that dtype."""
    B, _, H, W = depth.shape
    cols = F.unfold(rays * depth, kernel_size=5, dilation=2, padding=4)                      # [B, 75, H W], channel-major: 3 x 25
    A = cols.view(B, 3, 25, H, W).permute(0, 3, 4, 2, 1)                                     # [B, H, W, 25, 3]
    At = A.transpose(3, 4)
    M = At @ A
    ok = (torch.det(M) >= 1e-5)[..., None, None]
    M = torch.where(ok, M, torch.eye(3, dtype=depth.dtype, device=depth.device))
    n = torch.linalg.inv(M) @ At @ torch.ones(B, H, W, 25, 1, dtype=depth.dtype, device=depth.device)
    return F.normalize(n, dim=3).squeeze(-1).permute(0, 3, 1, 2)


def eager_loss(pred, gt, mask, rays):
    return 1 - ((eager_normals(pred, rays) * eager_normals(gt, rays) * mask).sum(dim=[1, 2, 3], keepdim=True) / mask.sum()).mean()


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(0)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eager-iters", type=int, default=2)
    ap.add_argument("--bufs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "planefit_bench measures on an MI355X; there is no CPU timing"
    import _planefit_cases as pc
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.equi_pers.depth2normal import depth2normal
    from omnifusion_amd.supervision import planefit_normal_loss
    H, W = 512, 1024
    B = 1 if a.quick else 8
    rounds, iters, eager_iters = (2, 3, 1) if a.quick else (a.rounds, a.iters, a.eager_iters)
    bufs = [make_inputs(B, H, W, 220 + k) for k in range(a.bufs)]
    ups = [torch.randn(B, 3, H, W, device=DEV) for _ in range(a.bufs)]
    n = a.bufs
    npix = B * H * W
    rays = torch.from_numpy(pc.rays(H, W)).to(DEV)[None]

    def no_grad(fn):
        def run(k):
            with torch.no_grad():
                fn(k)
        return run

    def map_step(normals):
        def run(k):
            p = bufs[k % n][0].detach().requires_grad_(True)
            (normals(p) * ups[k % n]).sum().backward()
        return run

    def loss_step(loss):
        def run(k):
            pred, gt, mask = bufs[k % n]
            loss(pred.detach().requires_grad_(True), gt, mask).backward()
        return run
    # ---- parity on the first item of the first buffer
    pred, gt, mask = (x[:1] for x in bufs[0])
    want = eager_normals(pred.double(), rays.double())
    want_l = float(eager_loss(pred.double(), gt.double(), mask.double(), rays.double()))
    e32 = eager_normals(pred, rays)
    parity = dict(normals_max_err_vs_f64=float((depth2normal(pred).double() - want).abs().max()),
                  eager_f32_normals_max_err_vs_f64=float((e32.double() - want).abs().max()),
                  eager_f32_normals_median_err_vs_f64=float((e32.double() - want).abs().amax(dim=1).median()),
                  loss_err_vs_f64=abs(float(planefit_normal_loss(pred, gt, mask)) - want_l),
                  eager_f32_loss_err_vs_f64=abs(float(eager_loss(pred, gt, mask, rays)) - want_l))
    del want, e32
    hip = {"hip_map_fwd": no_grad(lambda k: depth2normal(bufs[k % n][0])), "hip_map_fwd_bwd": map_step(depth2normal),
           "hip_loss_fwd": no_grad(lambda k: planefit_normal_loss(*bufs[k % n])), "hip_loss_fwd_bwd": loss_step(planefit_normal_loss)}
    eager = {"eager_map_fwd": no_grad(lambda k: eager_normals(bufs[k % n][0], rays)), "eager_map_fwd_bwd": map_step(lambda p: eager_normals(p, rays)),
             "eager_loss_fwd": no_grad(lambda k: eager_loss(*bufs[k % n], rays)), "eager_loss_fwd_bwd": loss_step(lambda p, g, m: eager_loss(p, g, m, rays))}
    legs = dict(hip, **eager)
    for name, fn in legs.items():                                           # warm every leg (the eager ones once: a call is long)
        for k in range(n if name in hip else 1):
            fn(k)
    torch.cuda.synchronize()
    peak = {name: peak_of(legs[name]) for name in ("hip_map_fwd_bwd", "eager_map_fwd_bwd", "hip_loss_fwd_bwd", "eager_loss_fwd_bwd")}
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(time_loop(fn, iters if name in hip else eager_iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = {"hip_map_fwd": 16 * npix, "hip_map_fwd_bwd": (16 + 20) * npix, "hip_loss_fwd": 12 * npix, "hip_loss_fwd_bwd": (12 + 16) * npix}
    row = dict(B=B, H=H, W=W, rounds=rounds, iters=iters, eager_iters=eager_iters, bufs=n, parity=parity)
    for name, v in times.items():
        row[name + "_us"] = round(med[name], 1)
        row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    for name, nb in nbytes.items():
        row[name + "_compulsory_bytes"] = nb
        row[name + "_frac_of_8TBps"] = round(nb / (med[name] * 1e-6) / 8e12, 4)
        row["speedup_" + name[4:]] = round(med["eager" + name[3:]] / med[name], 1)
    for name, v in peak.items():
        row[name + "_peak_bytes"] = int(v)
    print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), rows=[row])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
