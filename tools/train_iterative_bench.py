"""The point-feature operator and one training step of the trainable ITERATIVE spherical_fusion (omnifusion_amd/model/trainable_iterative.py,
DESIGN.md §25) on one MI355X, at 8 panoramas of 512 x 1024, nrows 4 (M = 144 patches of 128 x 128), random weights
make_state_dict(42, 18, True).

    python tools/train_iterative_bench.py [--bs 8] [--iters 5] [--repeats 3] [--out profiles/r22a_train_iterative.json]

In ONE process and one run, each row timed with device events around `iters` back-to-back calls after a warm-up of the same calls; the
median of `repeats` windows with the smallest and the largest beside it, and torch.cuda.max_memory_allocated over one call:
    point_3_16_fwd / point_3_16_fwd_bwd      ops.point_conv(rays [18,3,32,32], w [16,3,1,1], scale=depth [144,1,32,32]); backward w.r.t.
                                             the weight and the scale
    point_16_64_fwd / point_16_64_fwd_bwd    ops.point_conv(x [144,16,32,32] channels-last, w [64,16,1,1]); backward w.r.t. x and the weight
    sum_3_16_* / sum_16_64_*                 the same four from the product-and-sum form of trainable._PointConv — (x[:, None] * w).sum(2) on
                                             rays.repeat(8, 1, 1, 1) * depth and on x — on the same GPU
    iterative_fwd_bwd                        net(rgb, 2, confidence=True) -> sum_k sum(out_k . g_k) -> backward, training mode
    single_fwd_bwd                           the single-pass trainable model's step next to it (tools/train_bench.py's train_fwd_bwd)
    floors                                   the bytes each point_conv call must move (inputs once, outputs once) at 8 TB/s
There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash; DESIGN §25 and the README quote them.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omnifusion_amd import build, ops  # noqa: E402
from omnifusion_amd.model import trainable, trainable_iterative  # noqa: E402
from omnifusion_amd.weights import make_state_dict  # noqa: E402

DEV = "cuda:0"
NROWS, N, P, H, W, FOV = 4, 18, 128, 512, 1024, (80, 80)
HBM = 8e12
cl = lambda t: t.contiguous(memory_format=torch.channels_last)


def timed(fn, iters, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e-3)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def row(fn, iters, repeats):
    r = timed(fn, iters, repeats)
    r["peak_memory_bytes"] = peak(fn)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22a_train_iterative.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_iterative_bench needs an MI355X"
    bs, M, p4 = a.bs, a.bs * N, P // 4
    gen = torch.Generator().manual_seed(0)
    rows = {}

    # the operator alone, against the product-and-sum form
    rays = torch.randn(N, 3, p4, p4, generator=gen).to(DEV)
    depth = torch.rand(M, 1, p4, p4, generator=gen).to(DEV).requires_grad_(True)
    w0 = (torch.randn(16, 3, 1, 1, generator=gen) / 3 ** 0.5).to(DEV).requires_grad_(True)
    x1 = cl(torch.randn(M, 16, p4, p4, generator=gen).to(DEV)).requires_grad_(True)
    w1 = (torch.randn(64, 16, 1, 1, generator=gen) / 4.0).to(DEV).requires_grad_(True)
    g0, g1 = cl(torch.randn(M, 16, p4, p4, generator=gen).to(DEV)), cl(torch.randn(M, 64, p4, p4, generator=gen).to(DEV))
    sum_form = lambda x, w: (x[:, None] * w[None, :, :, :, :]).sum(2)           # trainable._PointConv.forward
    forms = {
        "point_3_16": (lambda: ops.point_conv(rays, w0, scale=depth), [w0, depth], g0),
        "sum_3_16": (lambda: sum_form(rays.repeat(bs, 1, 1, 1) * depth, w0), [w0, depth], g0),
        "point_16_64": (lambda: ops.point_conv(x1, w1), [x1, w1], g1),
        "sum_16_64": (lambda: sum_form(x1, w1), [x1, w1], g1),
    }
    hi = 20 * a.iters
    for name, (fwd, wrt, g) in forms.items():
        with torch.no_grad():
            rows[name + "_fwd"] = row(fwd, hi, a.repeats)
        rows[name + "_fwd_bwd"] = row(lambda: torch.autograd.grad(fwd(), wrt, g), hi, a.repeats)
    rows_px = M * p4 * p4
    floors = {"point_3_16_fwd": (rows_px * 4 + N * 3 * p4 * p4 * 4 + rows_px * 64) / HBM,       # the scale, the rays, y
              "point_16_64_fwd": (rows_px * 64 + rows_px * 256) / HBM}                           # x, y
    del rays, depth, x1, g0, g1

    # the steps
    rgb = torch.rand(bs, 3, H, W, generator=gen).to(DEV)
    gs = [torch.randn(bs, 1, H, W, generator=gen).to(DEV) for _ in range(2)]

    def step_of(net, fn):
        def step():
            for p in net.parameters():
                p.grad = None
            fn(net).backward()
        return step

    it = trainable_iterative.spherical_fusion(NROWS, N, (P, P), FOV)
    it.load_state_dict(make_state_dict(42, N, True))
    it.to(DEV)
    rows["iterative_fwd_bwd"] = row(step_of(it, lambda net: sum((o * g).sum() for o, g in zip(net(rgb, 2, confidence=True), gs))), a.iters, a.repeats)
    del it
    one = trainable.spherical_fusion(NROWS, N, (P, P), FOV)
    one.load_state_dict(make_state_dict(42, N))
    one.to(DEV)
    rows["single_fwd_bwd"] = row(step_of(one, lambda net: (net(rgb, confidence=True) * gs[0]).sum()), a.iters, a.repeats)

    result = {
        "tool": "tools/train_iterative_bench.py", "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(),
        "panoramas": bs, "erp": [H, W], "nrows": NROWS, "patches": M, "iters": a.iters, "repeats": a.repeats,
        "rows": rows, "floors_s": floors,
        "point_over_sum": {k: rows["point_" + k]["median_s"] / rows["sum_" + k]["median_s"]
                           for k in ("3_16_fwd", "3_16_fwd_bwd", "16_64_fwd", "16_64_fwd_bwd")},
        "point_over_floor": {k: rows[k]["median_s"] / v for k, v in floors.items()},
        "iterative_over_single": rows["iterative_fwd_bwd"]["median_s"] / rows["single_fwd_bwd"]["median_s"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
