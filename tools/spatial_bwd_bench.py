"""The stem convolution, the 3x3/2 max-pool and the 2x bilinear up-sampling in training mode (csrc/omni_stem_conv.hip, omni_maxpool_bwd.hip,
omni_upsample_bwd.hip) at their shapes in the benched network, B = 8 panoramas x 18 patches of 128 x 128 (M = 144).

    python tools/spatial_bwd_bench.py [--m 144] [--iters 50] [--repeats 5] [--only stem,pool,up3] [--out profiles/r20a_spatial_bwd.json]

Per operator, in ONE process and one run, each timed with device events around `iters` back-to-back calls after a warm-up of the same
calls; the median of `repeats` windows with the smallest and the largest window beside it:
    ours_fwd       the ops.* call on channels-last tensors (the stem's x planar), as a model calls it
    ours_fwd_bwd   the same and torch.autograd.grad (stem: w.r.t. the weight; pool, up-sampling: w.r.t. x)
    lib_bwd        the backward entry point alone, on buffers allocated once
    torch_fwd      the torch-eager operator on channels-last tensors, same GPU (F.conv2d / F.max_pool2d / F.interpolate)
    torch_fwd_bwd  the same and torch.autograd.grad w.r.t. the same tensor
    *_graph        fwd + bwd of either side captured in a torch.cuda.graph and replayed: the device's time without the host's
    stem only:     torch_conv2d_weight (torch.nn.grad.conv2d_weight alone) beside lib_bwd, and stem_sh_f16x3_fwd, the inference stem
                   (omni_stem_sh_f16x3: folded normalisation and ReLU, split-half output) at the same M and patch size
    floor          the bytes the backward must move at 8 TB/s (pool: x, g, dx; up-sampling: g, dx; stem: x and g once)
The two sides are compared at the sizes that are timed (largest difference over the largest reference magnitude).
There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash; DESIGN §22 and the README quote them.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnifusion_amd import _lib, build, ops  # noqa: E402

PATCH = 128
# (name, H, W, C) of the operator's input
POOL = ("pool", 64, 64, 64)
UPS = [("up0", 4, 4, 512), ("up1", 8, 8, 128), ("up2", 16, 16, 64), ("up3", 32, 32, 64), ("up4", 64, 64, 32)]     # in front of de_conv0_0 .. de_conv4_0
HBM = 8e12                                   # bytes per second

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
cl = lambda t: t.contiguous(memory_format=torch.channels_last)


def timed(fn, iters, repeats):
    """(median, min, max) over `repeats` windows of the mean time of `iters` calls, seconds"""
    for _ in range(3):
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
    return statistics.median(out), min(out), max(out)


def captured(fn):
    """fn captured in a graph after a warm-up on a side stream -> (the graph, fn's outputs: kept alive with it)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph, keep


def measure(variants, graphs, a):
    t = {key: timed(fn, a.iters, a.repeats) for key, fn in variants.items()}
    for key, fn in graphs.items():
        graph, keep = captured(fn)
        t[key] = timed(graph.replay, a.iters, a.repeats)
        del graph, keep
    return t


def rel(p, q):
    return ((p - q).abs().max() / q.abs().max()).item()


def ok(rc):
    assert rc == 0, _lib.load().omni_last_error()


def bench_stem(M, a, lib, S):
    dev = "cuda"
    H = W = PATCH
    Ho = Wo = PATCH // 2
    x = torch.randn(M, 3, H, W, device=dev)
    xc = cl(x)
    w = (torch.randn(64, 3, 7, 7, device=dev) / 147 ** 0.5).requires_grad_(True)
    wc = cl(w.detach()).requires_grad_(True)
    g = cl(torch.randn(M, 64, Ho, Wo, device=dev))
    ours = lambda: ops.stem_conv2d(x, w)
    eager = lambda: F.conv2d(xc, wc, None, stride=2, padding=3)
    ours_fb = lambda: torch.autograd.grad(ours(), (w,), g)
    eager_fb = lambda: torch.autograd.grad(eager(), (wc,), g)
    nbytes = lib.omni_stem_conv_bwd_workspace_bytes(M, H, W)
    ws, dw, db = torch.empty(nbytes // 4, device=dev), torch.empty(147, 64, device=dev), torch.empty(64, device=dev)
    gn = g.permute(0, 2, 3, 1)
    assert gn.is_contiguous()
    wk = w.detach().permute(2, 3, 1, 0).contiguous()
    y = torch.empty(M, Ho, Wo, 64, device=dev)
    lib_fwd = lambda: ok(lib.omni_stem_conv_fwd_f32(P(x), P(wk), None, P(y), M, H, W, S()))
    lib_bwd = lambda: ok(lib.omni_stem_conv_bwd_weight_f32(P(gn), P(x), P(dw), P(db), M, H, W, P(ws), nbytes, S()))
    torch_wgrad = lambda: torch.nn.grad.conv2d_weight(xc, (64, 3, 7, 7), g, stride=2, padding=3)
    # the inference stem on the matrix cores, with the engine's packed weights (tools/stembench.py)
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    net = spherical_fusion(4, 18, (PATCH, PATCH), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    with torch.no_grad():
        net(torch.rand((1, 3, 512, 1024), device=dev))                          # packs the weights
    ew = net._eng.w
    sh_out = torch.empty((M, Ho, Wo, 64), device=dev)
    stem_sh = lambda: _lib.check(lib.omni_stem_sh_f16x3(P(x), P(ew["stem.w16"]), P(ew["stem.b"]), P(sh_out), M, PATCH, S()), "stem")
    t = measure({"ours_fwd": ours, "ours_fwd_bwd": ours_fb, "lib_fwd": lib_fwd, "lib_bwd": lib_bwd, "torch_fwd": eager, "torch_fwd_bwd": eager_fb,
                 "torch_conv2d_weight": torch_wgrad, "stem_sh_f16x3_fwd": stem_sh},
                {"ours_fwd_bwd_graph": ours_fb, "torch_fwd_bwd_graph": eager_fb}, a)
    diff = {"y": rel(ours().detach(), eager().detach()), "dw": rel(ours_fb()[0], eager_fb()[0])}
    rows = M * Ho * Wo
    flop = 2.0 * rows * 147 * 64
    floor = (x.numel() + g.numel()) * 4 / HBM
    return {"op": "stem", "M": M, "H": H, "W": W, "C": 3, "rows": rows, "bwd_flop": flop, "bwd_floor_us": round(floor * 1e6, 2),
            "lib_bwd_tflops": round(flop / t["lib_bwd"][0] / 1e12, 2), "workspace_MiB": round(nbytes / 2 ** 20, 2)}, t, diff


def bench_x_op(name, M, H, W, C, a, lib, S):
    dev = "cuda"
    pool = name == "pool"
    x = cl(torch.randn(M, C, H, W, device=dev))
    if pool:
        x = cl(F.relu(x))                                                       # the pool's input is a ReLU output
    x.requires_grad_(True)
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (2 * H, 2 * W)
    g = cl(torch.randn(M, C, Ho, Wo, device=dev))
    ours = (lambda: ops.max_pool2d(x)) if pool else (lambda: ops.upsample_bilinear2x(x))
    eager = (lambda: F.max_pool2d(x, 3, 2, 1)) if pool else (lambda: F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False))
    ours_fb = lambda: torch.autograd.grad(ours(), (x,), g)
    eager_fb = lambda: torch.autograd.grad(eager(), (x,), g)
    xn, gn = x.detach().permute(0, 2, 3, 1), g.permute(0, 2, 3, 1)
    assert xn.is_contiguous() and gn.is_contiguous()
    dx = torch.empty_like(xn)
    if pool:
        lib_bwd = lambda: ok(lib.omni_maxpool3x3s2_bwd_f32(P(gn), P(xn), P(dx), M, H, W, C, S()))
        moved = (2 * x.numel() + g.numel()) * 4
    else:
        lib_bwd = lambda: ok(lib.omni_upsample_bilinear2x_bwd_f32(P(gn), P(dx), M, H, W, C, S()))
        moved = (x.numel() + g.numel()) * 4
    t = measure({"ours_fwd": ours, "ours_fwd_bwd": ours_fb, "lib_bwd": lib_bwd, "torch_fwd": eager, "torch_fwd_bwd": eager_fb},
                {"ours_fwd_bwd_graph": ours_fb, "torch_fwd_bwd_graph": eager_fb}, a)
    diff = {"y": rel(ours().detach(), eager().detach()), "dx": rel(ours_fb()[0], eager_fb()[0])}
    return {"op": name, "M": M, "H": H, "W": W, "C": C, "x_MiB": round(x.numel() * 4 / 2 ** 20, 2), "bwd_floor_us": round(moved / HBM * 1e6, 2)}, t, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=144)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join("profiles", "r20a_spatial_bwd.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_bwd_bench needs an MI355X: nothing is measured without one")
    lib = _lib.load()
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    only = set(a.only.split(",")) if a.only else None
    rows_out = []
    for name, H, W, C in [("stem", PATCH, PATCH, 3), POOL] + UPS:
        if only and name not in only:
            continue
        row, t, diff = bench_stem(a.m, a, lib, S) if name == "stem" else bench_x_op(name, a.m, H, W, C, a, lib, S)
        row["us"] = {k: round(v[0] * 1e6, 2) for k, v in t.items()}
        row["us_min_max"] = {k: [round(v[1] * 1e6, 2), round(v[2] * 1e6, 2)] for k, v in t.items()}
        row["fwd_over_torch"] = round(t["ours_fwd"][0] / t["torch_fwd"][0], 3)
        row["fwd_bwd_over_torch"] = round(t["ours_fwd_bwd"][0] / t["torch_fwd_bwd"][0], 3)
        row["graph_fwd_bwd_over_torch"] = round(t["ours_fwd_bwd_graph"][0] / t["torch_fwd_bwd_graph"][0], 3)
        row["lib_bwd_over_floor"] = round(t["lib_bwd"][0] * 1e6 / row["bwd_floor_us"], 2)
        if name == "stem":
            row["lib_bwd_over_torch_conv2d_weight"] = round(t["lib_bwd"][0] / t["torch_conv2d_weight"][0], 3)
            row["lib_bwd_over_stem_sh_f16x3_fwd"] = round(t["lib_bwd"][0] / t["stem_sh_f16x3_fwd"][0], 2)
        row["vs_torch_rel_max"] = diff
        rows_out.append(row)
        u = row["us"]
        print("%-5s [%d,%d,%d,%d] | fwd %8.1f us (%5.2fx torch %8.1f) | fwd+bwd %8.1f us (%5.2fx torch %8.1f) | lib bwd %8.1f us (%6.2fx floor) | "
              "graph fwd+bwd %8.1f (%5.2fx torch %8.1f) | rel. diff to torch %s"
              % (name, a.m, C, H, W, u["ours_fwd"], row["fwd_over_torch"], u["torch_fwd"], u["ours_fwd_bwd"], row["fwd_bwd_over_torch"],
                 u["torch_fwd_bwd"], u["lib_bwd"], row["lib_bwd_over_floor"], u["ours_fwd_bwd_graph"], row["graph_fwd_bwd_over_torch"],
                 u["torch_fwd_bwd_graph"], {k: "%.1e" % v for k, v in diff.items()}), flush=True)
        if name == "stem":
            print("      stem: lib fwd %.1f us | weight gradient %.1f us = %.2f TFLOP/s fp32, %.2fx torch conv2d_weight (%.1f us), %.2fx "
                  "omni_stem_sh_f16x3's forward (%.1f us)" % (u["lib_fwd"], u["lib_bwd"], row["lib_bwd_tflops"], row["lib_bwd_over_torch_conv2d_weight"],
                                                              u["torch_conv2d_weight"], row["lib_bwd_over_stem_sh_f16x3_fwd"], u["stem_sh_f16x3_fwd"]),
                  flush=True)
    out = {"tool": "tools/spatial_bwd_bench.py", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "M": a.m,
           "iters": a.iters, "repeats": a.repeats,
           "timing": "device events around `iters` calls, median (and min, max) of the `repeats` windows, warm-up of 3 calls per variant",
           "hbm_bytes_per_s": HBM, "rows": rows_out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
