"""Geometry-terms timing: the fused HIP forward and forward + backward of supervision.geometry.geometry_terms (csrc/omni_normals.hip) against
the torch-eager restatement of the same formulae (tests/_geometry_cases.py: pads, four cross products, five normalisations, two convolutions,
reductions, autograd) on the same GPU in the same run.

    python tools/geometry_bench.py [--rounds 5] [--iters 10] [--out profiles/r12a_geometry.json] [--quick]

Method (as tools/semantic_bench.py): device events over warm loops; the legs ALTERNATE (every round times each leg once, the median over the
rounds is reported with the spread) and every call of a loop takes the next of `--bufs` copies of the inputs.

Shape: B = 8 at 512 x 1024, hole-free smooth ground truth, pred = gt + a smooth perturbation, an 80 % random float mask.
Compulsory bytes: forward = pred + gt + float mask read, 12 B per pixel; backward = the same three read + the gradient written, 16 B per pixel.
The fraction printed is bytes / time / 8 TB/s.
Parity: the losses and the gradient of 0.2 normal_loss + 0.05 grad_loss against the same restatement in float64 on the device, on the timed inputs.
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


def make_inputs(B, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.linspace(0, 1, H, device=DEV)[None, None, :, None]
    x = torch.linspace(0, 1, W, device=DEV)[None, None, None, :]

    def field(waves):
        out = torch.zeros(B, 1, H, W, device=DEV)
        for _ in range(waves):
            fy, fx, ph = (torch.rand(B, 1, 1, 1, device=DEV, generator=g) * s for s in (9.0, 9.0, 6.283))
            out += torch.sin(fy * y + fx * x + ph) / waves
        return out
    gt = 2.5 + 1.5 * field(6)
    pred = gt + 0.2 * field(6)
    mask = (torch.rand(B, 1, H, W, device=DEV, generator=g) < 0.8).float()
    return pred.contiguous(), gt.contiguous(), mask


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
    assert torch.cuda.is_available(), "geometry_bench measures on an MI355X; there is no CPU timing"
    import _geometry_cases as gc
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.supervision import geometry_terms
    H, W = 512, 1024
    B = 1 if a.quick else 8
    rounds, iters = (2, 3) if a.quick else (a.rounds, a.iters)
    bufs = [make_inputs(B, H, W, 200 + k) for k in range(a.bufs)]
    n = a.bufs
    npix = B * H * W

    def hip_fwd(k):
        with torch.no_grad():
            geometry_terms(*bufs[k % n])

    def torch_fwd(k):
        with torch.no_grad():
            gc.terms(*bufs[k % n])

    def step(terms):
        def run(k):
            pred, gt, mask = bufs[k % n]
            p = pred.detach().requires_grad_(True)
            out = terms(p, gt, mask)
            (0.2 * out[0] + 0.05 * out[1]).backward()
        return run
    # ---- parity on the first buffer
    pred, gt, mask = bufs[0]
    p = pred.detach().requires_grad_(True)
    nl, gl = geometry_terms(p, gt, mask)
    grad, = torch.autograd.grad(0.2 * nl + 0.05 * gl, p)
    p64 = pred.detach().double().requires_grad_(True)
    n64, g64, _ = gc.terms(p64, gt.double(), mask.double())
    grad64, = torch.autograd.grad(0.2 * n64 + 0.05 * g64, p64)
    n32, g32, _ = gc.terms(pred, gt, mask)
    parity = dict(normal_loss_err_vs_f64=abs(float(nl.detach()) - float(n64.detach())), grad_loss_err_vs_f64=abs(float(gl.detach()) - float(g64.detach())),
                  torch_f32_normal_loss_err_vs_f64=abs(float(n32) - float(n64.detach())), torch_f32_grad_loss_err_vs_f64=abs(float(g32) - float(g64.detach())),
                  grad_max_err_rel_largest=float((grad.double() - grad64).abs().max() / grad64.abs().max()))
    del p64, grad64, grad
    legs = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_bwd": step(geometry_terms), "torch_fwd_bwd": step(lambda p, g, m: gc.terms(p, g, m)[:2])}
    for fn in legs.values():                                                # warm every leg on every buffer
        for k in range(n):
            fn(k)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(time_loop(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = {"hip_fwd": 12 * npix, "hip_fwd_bwd": (12 + 16) * npix}
    row = dict(B=B, H=H, W=W, rounds=rounds, iters=iters, bufs=n, parity=parity)
    for name, v in times.items():
        row[name + "_us"] = round(med[name], 1)
        row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    for name, nb in nbytes.items():
        row[name + "_compulsory_bytes"] = nb
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
