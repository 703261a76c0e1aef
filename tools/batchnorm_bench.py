"""Training-mode batch normalisation with a fused residual and ReLU (csrc/omni_batchnorm.hip) at the output shapes of the
network's convolutions, B = 8 panoramas x 18 patches (M = 144).

    python tools/batchnorm_bench.py [--m 144] [--iters 20] [--repeats 3] [--only 0,3] [--out profiles/r18a_batchnorm.json]

Per layer (the output shapes of tools/convbench.py), in ONE process and one run, each timed with device events around `iters` back-to-back
calls after a warm-up of the same calls, the median of `repeats` windows:
    fused_fwd      ops.batch_norm(x, w, b, rm, rv, res=res, training=True, act="relu") on channels-last tensors, as a model calls it
    fused_fwd_bwd  the same and torch.autograd.grad w.r.t. x, w, b and res
    lib_fwd        omni_batchnorm_fwd_f32 alone, on buffers allocated once (stats + finish + apply)
    lib_bwd        omni_batchnorm_bwd_f32 alone, every gradient asked for (reduce + finish + apply)
    torch_fwd      F.relu(F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5) + res), eager, channels-last, same GPU
    torch_fwd_bwd  the same and torch.autograd.grad w.r.t. the same four tensors
    *_graph        fwd + bwd of either side captured in a torch.cuda.graph and replayed: the device's time without the host's (at the small
                   shapes both sides are bound by the host: a Python autograd.Function here, the dispatcher there)
    floor          the bytes each pass must move (fwd 16 B per element: x twice, res, y; bwd 28 B: g, y, x, dZ written; dZ, x, dx) at 8 TB/s
The two sides are compared at the sizes that are timed; a pre-activation within an ulp of 0 can fall on either side of the ReLU (the two
forwards differ in the last bit), so the elements whose masks differ are counted and dx / dres are compared on the others.
There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash; DESIGN §20 and the README quote them.
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

# (name, H, W, C1, C2, Cout, k, stride, pad) — tools/convbench.py
CFGS = [("layer1", 32, 32, 64, 0, 64, 3, 1, 1), ("layer2_0a", 32, 32, 64, 0, 128, 3, 2, 1), ("layer2", 16, 16, 128, 0, 128, 3, 1, 1),
        ("layer3_0a", 16, 16, 128, 0, 256, 3, 2, 1), ("layer3", 8, 8, 256, 0, 256, 3, 1, 1), ("layer4_0a", 8, 8, 256, 0, 512, 3, 2, 1),
        ("layer4", 4, 4, 512, 0, 512, 3, 1, 1), ("de0_0", 8, 8, 512, 0, 256, 3, 1, 1), ("de0_1", 8, 8, 256, 256, 128, 3, 1, 1),
        ("de1_0", 16, 16, 128, 0, 128, 3, 1, 1), ("de1_1", 16, 16, 128, 128, 64, 3, 1, 1), ("de2_0", 32, 32, 64, 0, 64, 3, 1, 1),
        ("de2_1", 32, 32, 64, 64, 64, 3, 1, 1), ("de3_0", 64, 64, 64, 0, 64, 3, 1, 1), ("de3_1", 64, 64, 64, 64, 32, 3, 1, 1),
        ("de4_0", 128, 128, 32, 0, 32, 3, 1, 1)]
HBM = 8e12                                   # bytes per second
FWD_BYTES, BWD_BYTES = 16, 28                # per element (module docstring)

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn, iters, repeats):
    """median over `repeats` windows of the mean time of `iters` calls, seconds"""
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
    return statistics.median(out)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=144)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join("profiles", "r18a_batchnorm.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batchnorm_bench needs an MI355X: nothing is measured without one")
    lib = _lib.load()
    dev = "cuda"
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfgs = [CFGS[int(i)] for i in a.only.split(",")] if a.only else CFGS
    M = a.m
    rows_out = []
    for name, H, W, C1, C2, C, k, s, pad in cfgs:
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        rows = M * Ho * Wo
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        x, res, g = (cl(torch.randn(M, C, Ho, Wo, device=dev)) for _ in range(3))
        x.requires_grad_(True)
        res.requires_grad_(True)
        w = (1 + 0.1 * torch.randn(C, device=dev)).requires_grad_(True)
        b = (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        leaves = (x, w, b, res)

        fused = lambda: ops.batch_norm(x, w, b, rm, rv, res=res, training=True, momentum=0.1, eps=1e-5, act="relu")
        eager = lambda: F.relu(F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5) + res)
        fused_fb = lambda: torch.autograd.grad(fused(), leaves, g)
        eager_fb = lambda: torch.autograd.grad(eager(), leaves, g)

        # the library alone, on buffers allocated once
        nbytes = lib.omni_batchnorm_workspace_bytes(rows, C)
        assert nbytes > 0, (rows, C)
        ws = torch.empty(nbytes // 4, device=dev)
        xn, resn, gn = (t.detach().permute(0, 2, 3, 1) for t in (x, res, g))
        assert xn.is_contiguous() and resn.is_contiguous() and gn.is_contiguous()
        y, dx, dres = torch.empty_like(xn), torch.empty_like(xn), torch.empty_like(xn)
        saved, dgamma, dbeta = torch.empty(2, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        wd, bd = w.detach(), b.detach()

        def ok(rc):
            assert rc == 0, lib.omni_last_error()

        lib_fwd = lambda: ok(lib.omni_batchnorm_fwd_f32(P(xn), P(resn), P(wd), P(bd), P(rm), P(rv), P(y), P(saved), rows, C, 1, 0.1, 1e-5, 1,
                                                        P(ws), nbytes, S()))
        lib_bwd = lambda: ok(lib.omni_batchnorm_bwd_f32(P(gn), P(xn), P(y), P(wd), P(saved), P(dx), P(dres), P(dgamma), P(dbeta), rows, C, 1, 1,
                                                        P(ws), nbytes, S()))
        lib_fwd()
        t = {"fused_fwd": timed(fused, a.iters, a.repeats), "fused_fwd_bwd": timed(fused_fb, a.iters, a.repeats),
             "lib_fwd": timed(lib_fwd, a.iters, a.repeats), "lib_bwd": timed(lib_bwd, a.iters, a.repeats),
             "torch_fwd": timed(eager, a.iters, a.repeats), "torch_fwd_bwd": timed(eager_fb, a.iters, a.repeats)}
        for key, fn in (("fused_fwd_bwd_graph", fused_fb), ("torch_fwd_bwd_graph", eager_fb)):
            graph, keep = captured(fn)
            t[key] = timed(graph.replay, a.iters, a.repeats)
            del graph, keep
        # same results? (the two sides at the sizes that are timed)
        yf, ye = fused().detach(), eager().detach()
        gf, ge = fused_fb(), eager_fb()
        rel = lambda p, q: ((p - q).abs().max() / q.abs().max()).item()
        agree = (yf > 0) == (ye > 0)
        diff = {"y": rel(yf, ye), "dx": rel(gf[0] * agree, ge[0] * agree), "dgamma": rel(gf[1], ge[1]), "dbeta": rel(gf[2], ge[2]),
                "dres": rel(gf[3] * agree, ge[3] * agree), "relu_masks_that_differ": int((~agree).sum().item())}
        n = rows * C
        floor_f, floor_b = n * FWD_BYTES / HBM, n * BWD_BYTES / HBM
        row = {"layer": name, "M": M, "H": Ho, "W": Wo, "C": C, "rows": rows, "MiB": round(n * 4 / 2 ** 20, 2),
               "us": {key: round(v * 1e6, 2) for key, v in t.items()},
               "floor_us": {"fwd": round(floor_f * 1e6, 2), "bwd": round(floor_b * 1e6, 2)},
               "fwd_over_torch": round(t["fused_fwd"] / t["torch_fwd"], 3), "fwd_bwd_over_torch": round(t["fused_fwd_bwd"] / t["torch_fwd_bwd"], 3),
               "graph_fwd_bwd_over_torch": round(t["fused_fwd_bwd_graph"] / t["torch_fwd_bwd_graph"], 3),
               "lib_fwd_over_floor": round(t["lib_fwd"] / floor_f, 2), "lib_bwd_over_floor": round(t["lib_bwd"] / floor_b, 2),
               "vs_torch_rel_max": diff}
        rows_out.append(row)
        print("%-10s %7.1f MiB | fwd %8.1f us (%5.2fx torch %8.1f) | fwd+bwd %8.1f us (%5.2fx torch %8.1f) | lib fwd %7.1f (%5.2fx floor) bwd %7.1f "
              "(%5.2fx floor) | graph fwd+bwd %7.1f (%5.2fx torch %7.1f) | rel. diff to torch y %.1e dx %.1e dgamma %.1e, %d masks differ"
              % (name, row["MiB"], t["fused_fwd"] * 1e6, row["fwd_over_torch"], t["torch_fwd"] * 1e6, t["fused_fwd_bwd"] * 1e6,
                 row["fwd_bwd_over_torch"], t["torch_fwd_bwd"] * 1e6, t["lib_fwd"] * 1e6, row["lib_fwd_over_floor"], t["lib_bwd"] * 1e6,
                 row["lib_bwd_over_floor"], t["fused_fwd_bwd_graph"] * 1e6, row["graph_fwd_bwd_over_torch"], t["torch_fwd_bwd_graph"] * 1e6, diff["y"], diff["dx"],
                 diff["dgamma"], diff["relu_masks_that_differ"]), flush=True)
    out = {"tool": "tools/batchnorm_bench.py", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "M": M,
           "iters": a.iters, "repeats": a.repeats, "timing": "device events, median of the windows, warm-up of 3 calls per shape",
           "bytes_per_element": {"fwd": FWD_BYTES, "bwd": BWD_BYTES}, "hbm_bytes_per_s": HBM, "rows": rows_out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
