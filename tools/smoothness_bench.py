"""Smoothness-term timing: the fused HIP forward and forward + backward of supervision.smoothness.depth_smoothness (csrc/omni_smoothness.hip)
against the torch-eager restatement of the same formulae (tests/_smoothness_cases.py: vertices, six difference maps, two magnitudes, the
guide's norm, exp, select, reductions, autograd) on the same GPU in the same run.

    python tools/smoothness_bench.py [--rounds 5] [--iters 10] [--out profiles/r13a_smoothness.json] [--quick]

Method (as tools/geometry_bench.py): device events over warm loops; the legs ALTERNATE (every round times each leg once, the median over the
rounds is reported with the spread) and every call of a loop takes the next of `--bufs` copies of the inputs.

Shape: B = 8 at 512 x 1024, C = 3, smooth depth plus a checkerboard, an 80 % random float mask, weights = spherical_confidence-like [B,1,H,W].
Compulsory bytes: forward = depth + image + float mask + weights read, 24 B per pixel (101 MB: about 13 us at 8 TB/s); backward = the same
read + the gradient written, 28 B per pixel.  The direction factors (16 B per pixel of ONE item, shared by the batch) are not counted.
The fraction printed is bytes / time / 8 TB/s.
Parity: the loss and the gradient against the same restatement in float64 on the device, on the timed inputs.
--quick: B = 1, few iterations.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
C = 3


def make_inputs(B, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.linspace(0, 1, H, device=DEV)[None, None, :, None]
    x = torch.linspace(0, 1, W, device=DEV)[None, None, None, :]

    def field(waves, channels=1):
        out = torch.zeros(B, channels, H, W, device=DEV)
        for _ in range(waves):
            fy, fx, ph = (torch.rand(B, channels, 1, 1, device=DEV, generator=g) * s for s in (9.0, 9.0, 6.283))
            out += torch.sin(fy * y + fx * x + ph) / waves
        return out
    ii = torch.arange(H, device=DEV)[:, None] + torch.arange(W, device=DEV)[None, :]
    depth = 2.5 + 0.25 * field(6) + 0.72 * torch.where(ii % 2 == 0, 1.0, -1.0)[None, None]
    image = (0.5 + 0.3 * field(6, C) + 0.1 * (torch.rand(B, C, H, W, device=DEV, generator=g) - 0.5)).contiguous()
    mask = (torch.rand(B, 1, H, W, device=DEV, generator=g) < 0.8).float()
    weights = (0.6 + 0.4 * field(3)).contiguous()
    return depth.contiguous(), image, mask, weights


def time_loop(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                                # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bufs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "smoothness_bench measures on an MI355X; there is no CPU timing"
    import _smoothness_cases as sc
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.supervision import depth_smoothness
    H, W = 512, 1024
    B = 1 if a.quick else 8
    rounds, iters = (2, 3) if a.quick else (a.rounds, a.iters)
    bufs = [make_inputs(B, H, W, 300 + k) for k in range(a.bufs)]
    n = a.bufs
    npix = B * H * W
    sg = sc.sgrid(H, W).to(DEV)
    sg64 = sg.double()

    def torch_loss(depth, image, mask, weights, grid=sg):
        return sc.loss_of_depth(depth, image, mask != 0, weights, grid)

    def hip_fwd(k):
        with torch.no_grad():
            depth_smoothness(*bufs[k % n], sg)

    def torch_fwd(k):
        with torch.no_grad():
            torch_loss(*bufs[k % n])

    def step(loss_of):
        def run(k):
            depth, image, mask, weights = bufs[k % n]
            d = depth.detach().requires_grad_(True)
            loss_of(d, image, mask, weights).backward()
        return run
    # ---- parity on the first buffer
    depth, image, mask, weights = bufs[0]
    d = depth.detach().requires_grad_(True)
    loss = depth_smoothness(d, image, mask, weights, sg)
    grad, = torch.autograd.grad(loss, d)
    d64 = depth.detach().double().requires_grad_(True)
    l64 = torch_loss(d64, image.double(), mask, weights.double(), sg64)
    grad64, = torch.autograd.grad(l64, d64)
    with torch.no_grad():
        l32 = torch_loss(depth, image, mask, weights)
    parity = dict(loss=float(loss.detach()), loss_err_vs_f64=abs(float(loss.detach()) - float(l64.detach())), torch_f32_loss_err_vs_f64=abs(float(l32) - float(l64.detach())),
                  grad_max_err_rel_largest=float((grad.double() - grad64).abs().max() / grad64.abs().max()))
    del d64, grad64, grad
    legs = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_bwd": step(lambda d, i, m, w: depth_smoothness(d, i, m, w, sg)), "torch_fwd_bwd": step(torch_loss)}
    for fn in legs.values():                                                # warm every leg on every buffer
        for k in range(n):
            fn(k)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(time_loop(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = {"hip_fwd": (12 + 4 * C) * npix, "hip_fwd_bwd": (12 + 4 * C + 16 + 4 * C) * npix}
    row = dict(B=B, C=C, H=H, W=W, rounds=rounds, iters=iters, bufs=n, parity=parity)
    for name, v in times.items():
        row[name + "_us"] = round(med[name], 1)
        row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    for name, nb in nbytes.items():
        row[name + "_compulsory_bytes"] = nb
        row[name + "_floor_us_at_8TBps"] = round(nb / 8e12 * 1e6, 1)
        row[name + "_frac_of_8TBps"] = round(nb / (med[name] * 1e-6) / 8e12, 4)
    row["speedup_fwd"] = round(med["torch_fwd"] / med["hip_fwd"], 2)
    row["speedup_fwd_bwd"] = round(med["torch_fwd_bwd"] / med["hip_fwd_bwd"], 2)
    print(json.dumps(row), flush=True)
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), rows=[row])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
