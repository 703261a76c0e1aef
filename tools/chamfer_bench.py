"""Chamfer timing: the HIP forward and forward + backward of supervision.chamfer.chamfer_distance (csrc/omni_chamfer.hip) against a chunked
torch.cdist(...).min with its autograd on the same GPU in the same run.

    python tools/chamfer_bench.py [--rounds 3] [--iters 2] [--out profiles/r14a_chamfer.json] [--quick]

Method (as tools/smoothness_bench.py): device events over warm loops; the legs ALTERNATE (every round times each leg once, the median over
the rounds is reported with the spread) and every call of a loop takes the next of `--bufs` copies of the inputs.

Shapes: B = 8, D = 3, N = M = 32 768 and 131 072, coordinates uniform in [-3, 3].
Baseline: per item and per chunk of `--chunk` queries, cdist(p1[b, chunk], p2[b]).min(1).values.sum(); for forward + backward each chunk's
backward runs before the next chunk's forward, so at most one [chunk, M] distance matrix is alive (the reference's own form would need
12 N M bytes per item).  torch.cdist evaluates |a|^2 + |b|^2 - 2ab above 25 points, so its distances carry the expansion's error.
Floor: the inner loop of chamfer_nn_kernel issues 9 vector instructions per pair (3 subtractions, a product and two explicit fused
multiply-adds, the comparison and two selects; no packed fp32 in this library), a SIMD issues 32 lanes per cycle: 256 CUs x 4 SIMDs x
32 lanes x 2.4 GHz = 7.86e13 lane-instructions per second.  The fraction printed is 9 B N M / time / 7.86e13.
Parity: loss and gradients against the float64 direct-difference restatement on the device, on one item of the timed inputs.
--quick: B = 1, N = M = 8192 only, few iterations.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
D = 3
OPS_PER_PAIR = 9
LANE_RATE = 256 * 4 * 32 * 2.4e9


def make_inputs(B, N, M, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (6.0 * torch.rand(B, N, D, device=DEV, generator=g) - 3.0).contiguous(), (6.0 * torch.rand(B, M, D, device=DEV, generator=g) - 3.0).contiguous()


def time_loop(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                                # us


def torch_chunks(p1, p2, chunk, backward):
    """-> the loss as a float tensor; with backward=True p1.grad / p2.grad are accumulated chunk by chunk."""
    total = torch.zeros((), device=p1.device)
    for b in range(p1.shape[0]):
        for i0 in range(0, p1.shape[1], chunk):
            part = torch.cdist(p1[b, i0:i0 + chunk], p2[b]).min(dim=1).values.sum()
            if backward:
                part.backward()
            total += part.detach()
    return total


def bench_shape(B, N, M, a, rounds, iters):
    from omnifusion_amd.supervision import chamfer_distance
    bufs = [make_inputs(B, N, M, 400 + k) for k in range(a.bufs)]
    n = a.bufs

    def hip_fwd(k):
        with torch.no_grad():
            chamfer_distance(*bufs[k % n])

    def torch_fwd(k):
        with torch.no_grad():
            torch_chunks(*bufs[k % n], a.chunk, False)

    def hip_step(k):
        p1, p2 = (x.detach().requires_grad_(True) for x in bufs[k % n])
        chamfer_distance(p1, p2).backward()

    def torch_step(k):
        p1, p2 = (x.detach().requires_grad_(True) for x in bufs[k % n])
        torch_chunks(p1, p2, a.chunk, True)
    # ---- parity on the first item of the first buffer, float64 direct differences in chunks
    p1, p2 = (x[:1].detach().requires_grad_(True) for x in bufs[0])
    loss = chamfer_distance(p1, p2)
    loss.backward()
    q1, q2 = (x[:1].detach().double().requires_grad_(True) for x in bufs[0])
    l64 = 0.0
    for i0 in range(0, N, 1024):
        part = torch.linalg.vector_norm(q1[0, i0:i0 + 1024, None] - q2[0, None], dim=2).min(dim=1).values.sum()
        part.backward()
        l64 += float(part.detach())
    with torch.no_grad():
        lcd = float(torch_chunks(bufs[0][0][:1], bufs[0][1][:1], a.chunk, False))
    parity = dict(loss=float(loss.detach()), loss_rel_err_vs_f64=abs(float(loss.detach()) - l64) / abs(l64), torch_cdist_loss_rel_err_vs_f64=abs(lcd - l64) / abs(l64),
                  grad_p1_max_err=float((p1.grad.double() - q1.grad).abs().max()), grad_p2_max_err_rel_largest=float((p2.grad.double() - q2.grad).abs().max() / q2.grad.abs().max()))
    del q1, q2
    legs = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_bwd": hip_step, "torch_fwd_bwd": torch_step}
    for fn in legs.values():                                                # warm every leg on every buffer
        for k in range(n):
            fn(k)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(time_loop(fn, iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    floor_us = OPS_PER_PAIR * B * N * M / LANE_RATE * 1e6
    row = dict(B=B, N=N, M=M, D=D, rounds=rounds, iters=iters, bufs=n, torch_chunk=a.chunk, parity=parity, valu_ops_per_pair=OPS_PER_PAIR,
               valu_floor_us=round(floor_us, 1))
    for name, v in times.items():
        row[name + "_us"] = round(med[name], 1)
        row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    row["hip_fwd_frac_of_valu_floor"] = round(floor_us / med["hip_fwd"], 4)
    row["hip_fwd_bwd_frac_of_valu_floor"] = round(floor_us / med["hip_fwd_bwd"], 4)
    row["speedup_fwd"] = round(med["torch_fwd"] / med["hip_fwd"], 2)
    row["speedup_fwd_bwd"] = round(med["torch_fwd_bwd"] / med["hip_fwd_bwd"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--bufs", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=4096, help="queries per cdist call of the baseline")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "chamfer_bench measures on an MI355X; there is no CPU timing"
    from omnifusion_amd.build import source_hash
    shapes = [(1, 8192, 8192)] if a.quick else [(8, 32768, 32768), (8, 131072, 131072)]
    rounds, iters = (2, 2) if a.quick else (a.rounds, a.iters)
    rows = [bench_shape(B, N, M, a, rounds, iters) for B, N, M in shapes]
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
