"""Data and weight gradient of the convolution (csrc/omni_conv_bwd.hip) at the network's layer shapes, B = 8 panoramas x 18 patches (M = 144).

    python tools/conv_bwd_bench.py [--m 144] [--iters 20] [--repeats 3] [--only 0,3] [--precision f16x3|f16x1|both]
                                   [--out profiles/r17a_conv_bwd.json]

Per layer (the shapes of tools/convbench.py), in ONE process and one run, each timed with device events around `iters` back-to-back calls after
a warm-up of the same calls, the median of `repeats` windows:
    fwd     omni_conv2d_nhwc_f16x3_ws (the forward the gradients belong to; the library's split-K plan)
    dgrad   omni_conv2d_bwd_data_f16x3 (includes the per-call weight repack)        t_dgrad / t_fwd
    wgrad   omni_conv2d_bwd_weight_f16x3 (partial sums + the ordered second pass)     t_wgrad / t_fwd
    torch   torch.nn.grad.conv2d_input / conv2d_weight, fp32, channels-last, same GPU  t_dgrad / t_torch_dgrad, t_wgrad / t_torch_wgrad
The gradient epilogue (one element-wise pass) is timed on its own.
--precision f16x1 times the single-product entry points in the same way.  --precision both times the two modes INTERLEAVED:
per kernel (fwd, dgrad, wgrad) the windows alternate f16x3, f16x1, f16x3, ... in one process, and a row holds per mode the median, the
smallest and the largest window, the ratio f16x1 / f16x3 of the medians and the run's own spread (largest - smallest window over the
median, the larger of the two modes); torch is not timed then.  There is no GPU -> the tool fails; it never falls back.
Writes the rows with the library's source hash; the README quotes the ratios from that file.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnifusion_amd import _lib, build  # noqa: E402

# (name, H, W, C1, C2, Cout, k, stride, pad) — tools/convbench.py
CFGS = [("layer1", 32, 32, 64, 0, 64, 3, 1, 1), ("layer2_0a", 32, 32, 64, 0, 128, 3, 2, 1), ("layer2", 16, 16, 128, 0, 128, 3, 1, 1),
        ("layer3_0a", 16, 16, 128, 0, 256, 3, 2, 1), ("layer3", 8, 8, 256, 0, 256, 3, 1, 1), ("layer4_0a", 8, 8, 256, 0, 512, 3, 2, 1),
        ("layer4", 4, 4, 512, 0, 512, 3, 1, 1), ("de0_0", 8, 8, 512, 0, 256, 3, 1, 1), ("de0_1", 8, 8, 256, 256, 128, 3, 1, 1),
        ("de1_0", 16, 16, 128, 0, 128, 3, 1, 1), ("de1_1", 16, 16, 128, 128, 64, 3, 1, 1), ("de2_0", 32, 32, 64, 0, 64, 3, 1, 1),
        ("de2_1", 32, 32, 64, 64, 64, 3, 1, 1), ("de3_0", 64, 64, 64, 0, 64, 3, 1, 1), ("de3_1", 64, 64, 64, 64, 32, 3, 1, 1),
        ("de4_0", 128, 128, 32, 0, 32, 3, 1, 1)]

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


def timed_interleaved(fns, iters, repeats):
    """[{median, min, max} per function], seconds: the windows of the functions alternate, so that clock and thermal drift reach all alike"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / iters * 1e-3)
    return [{"median": statistics.median(v), "min": min(v), "max": max(v)} for v in out]


def entry_points(lib, precision):
    sfx = "_" + precision
    return (getattr(lib, "omni_conv2d_split_weights" + sfx), getattr(lib, "omni_conv2d_nhwc" + sfx + "_ws"),
            getattr(lib, "omni_conv2d_bwd_data" + sfx), getattr(lib, "omni_conv2d_bwd_weight" + sfx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=144)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--precision", default="f16x3", choices=("f16x3", "f16x1", "both"))
    ap.add_argument("--out", default=os.path.join("profiles", "r17a_conv_bwd.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_bwd_bench needs an MI355X: nothing is measured without one")
    lib = _lib.load()
    dev = "cuda"
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfgs = [CFGS[int(i)] for i in a.only.split(",")] if a.only else CFGS
    M = a.m
    rows_out = []
    for name, H, W, C1, C2, Cout, k, s, pad in cfgs:
        Cin, K = C1 + C2, (C1 + C2) * k * k
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        shape = (M, H, W, C1, C2, Cout, k, k, s, pad)
        x1 = torch.randn(M, H, W, C1, device=dev)
        x2 = torch.randn(M, H, W, C2, device=dev) if C2 else None
        w = (torch.randn(Cout, K) / np.sqrt(K)).to(dev)
        b = torch.randn(Cout, device=dev)
        g = torch.randn(M, Ho, Wo, Cout, device=dev) * 1e-6                       # the magnitude of a loss averaged over 5e5 pixels
        out, dz = torch.empty(M, Ho, Wo, Cout, device=dev), torch.empty(M, Ho, Wo, Cout, device=dev)
        w16 = torch.empty(Cout * K * 2, dtype=torch.float16, device=dev)
        sk = lib.omni_conv2d_splitk_plan(M * Ho * Wo, Cout, K // 32)
        fws = torch.empty(max(1, sk * M * Ho * Wo * Cout), device=dev)
        nbytes = lib.omni_conv2d_bwd_workspace_bytes(*shape)
        assert nbytes > 0, shape
        ws = torch.empty(nbytes // 4, device=dev)
        scale, dbias = torch.empty(2, device=dev), torch.empty(Cout, device=dev)
        dx1 = torch.empty_like(x1)
        dx2 = torch.empty_like(x2) if C2 else None
        dw = torch.empty_like(w)

        def ok(rc):
            assert rc == 0, lib.omni_last_error()

        def calls(precision, w16):
            split, conv, bdata, bweight = entry_points(lib, precision)
            ok(split(P(w), P(w16), Cout, K, S()))
            return {"fwd": lambda: ok(conv(P(x1), P(x2), P(w16), P(b), None, P(out), M, H, W, C1, C2, Cout, k, k, s, pad, 1, sk, P(fws),
                                           ctypes.c_size_t(fws.numel() * 4), S())),
                    "dgrad": lambda: ok(bdata(P(dz), P(w), P(scale), P(dx1), P(dx2), *shape, P(ws), nbytes, S())),
                    "wgrad": lambda: ok(bweight(P(dz), P(x1), P(x2), P(scale), P(dw), *shape, P(ws), nbytes, S()))}

        epi = lambda: ok(lib.omni_conv2d_bwd_epilogue_f32(P(g), P(out), P(dz), P(dbias), P(scale), M * Ho * Wo, Cout, 1, P(ws), nbytes, S()))
        if a.precision == "both":
            c3, c1 = calls("f16x3", w16), calls("f16x1", torch.empty(Cout * K, dtype=torch.float16, device=dev))
            c3["fwd"]()
            epi()
            row = {"layer": name, "M": M, "H": H, "W": W, "C1": C1, "C2": C2, "Cout": Cout, "k": k, "stride": s, "pad": pad, "splitk_fwd": sk,
                   "us": {}, "f16x1_over_f16x3": {}, "spread": {}}
            for key in ("fwd", "dgrad", "wgrad"):
                t3, t1 = timed_interleaved([c3[key], c1[key]], a.iters, a.repeats)
                row["us"][key] = {m: {q: round(v * 1e6, 2) for q, v in t.items()} for m, t in (("f16x3", t3), ("f16x1", t1))}
                row["f16x1_over_f16x3"][key] = round(t1["median"] / t3["median"], 3)
                row["spread"][key] = round(max((t["max"] - t["min"]) / t["median"] for t in (t3, t1)), 3)
            rows_out.append(row)
            print("%-10s " % name + " | ".join("%s %8.1f -> %8.1f us (x%.3f, spread %.3f)" % (
                key, row["us"][key]["f16x3"]["median"], row["us"][key]["f16x1"]["median"], row["f16x1_over_f16x3"][key], row["spread"][key])
                for key in ("fwd", "dgrad", "wgrad")), flush=True)
            continue
        c = calls(a.precision, w16)
        fwd, dgrad, wgrad = c["fwd"], c["dgrad"], c["wgrad"]
        fwd()
        epi()
        # torch, fp32, channels-last views of the same storage
        xin = (x1 if x2 is None else torch.cat([x1, x2], 3)).permute(0, 3, 1, 2)
        wt = w.view(Cout, k, k, Cin).permute(0, 3, 1, 2)
        dzt = dz.permute(0, 3, 1, 2)
        prev = torch.backends.cudnn.allow_tf32
        torch.backends.cudnn.allow_tf32 = False
        t_dgrad = lambda: torch.nn.grad.conv2d_input(xin.shape, wt, dzt, stride=s, padding=pad)
        t_wgrad = lambda: torch.nn.grad.conv2d_weight(xin, wt.shape, dzt, stride=s, padding=pad)
        t = {"fwd": timed(fwd, a.iters, a.repeats), "epilogue": timed(epi, a.iters, a.repeats), "dgrad": timed(dgrad, a.iters, a.repeats),
             "wgrad": timed(wgrad, a.iters, a.repeats), "torch_dgrad": timed(t_dgrad, a.iters, a.repeats),
             "torch_wgrad": timed(t_wgrad, a.iters, a.repeats)}
        torch.backends.cudnn.allow_tf32 = prev
        # same results? (the two sides at the sizes that are timed)
        rd = t_dgrad()
        ours = dx1 if x2 is None else torch.cat([dx1, dx2], 3)
        ed = ((ours.permute(0, 3, 1, 2) - rd).abs().max() / rd.abs().max()).item()
        rw = t_wgrad()
        ew = ((dw.view(Cout, k, k, Cin).permute(0, 3, 1, 2) - rw).abs().max() / rw.abs().max()).item()
        row = {"layer": name, "M": M, "H": H, "W": W, "C1": C1, "C2": C2, "Cout": Cout, "k": k, "stride": s, "pad": pad, "splitk_fwd": sk,
               "us": {key: round(v * 1e6, 2) for key, v in t.items()},
               "dgrad_over_fwd": round(t["dgrad"] / t["fwd"], 3), "wgrad_over_fwd": round(t["wgrad"] / t["fwd"], 3),
               "dgrad_over_torch": round(t["dgrad"] / t["torch_dgrad"], 3), "wgrad_over_torch": round(t["wgrad"] / t["torch_wgrad"], 3),
               "dgrad_vs_torch_rel_max": ed, "wgrad_vs_torch_rel_max": ew}
        rows_out.append(row)
        print("%-10s fwd %8.1f us | dgrad %8.1f (%5.2fx fwd, %5.2fx torch) | wgrad %8.1f (%5.2fx fwd, %5.2fx torch) | epilogue %7.1f | rel. diff to torch %.1e %.1e"
              % (name, t["fwd"] * 1e6, t["dgrad"] * 1e6, row["dgrad_over_fwd"], row["dgrad_over_torch"], t["wgrad"] * 1e6, row["wgrad_over_fwd"],
                 row["wgrad_over_torch"], t["epilogue"] * 1e6, ed, ew), flush=True)
    res = {"tool": "tools/conv_bwd_bench.py", "precision": a.precision, "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "M": M,
           "iters": a.iters, "repeats": a.repeats, "timing": "device events, median of the windows, warm-up of 3 calls per shape" +
           ("; the windows of the two modes alternate" if a.precision == "both" else ""),
           "grad_out_scale": 1e-6, "rows": rows_out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
