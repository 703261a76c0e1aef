"""The transformer's training operators (csrc/omni_transformer_bwd.hip) at the model's shapes: bs in {1, 8} panoramas of
N = 18 patches (18 and 144 token rows) and bs = 8 with N = 46.

    python tools/transformer_bwd_bench.py [--iters 20] [--repeats 3] [--out profiles/r19a_transformer_bwd.json]

Per shape and operator, in ONE process and one run, each timed with device events around `iters` back-to-back calls after a warm-up of the
same calls, the median of `repeats` windows:
    layer_norm   ops.layer_norm on [rows, 512] with weight and bias        against F.layer_norm
    gelu         ops.gelu on [rows, 2048]                                   against F.gelu
    attention    ops.attention on q [rows, 512], kv [rows, 1024]            against softmax(q k^T / sqrt(128)) v in torch, 4 heads
    block        one ops.TransformerBlock step (forward + every gradient)  against the same block from torch's own operators
each as  *_fwd  (the forward alone),  *_fwd_bwd  (forward and torch.autograd.grad w.r.t. every differentiable input), and
*_fwd_bwd_graph  (the same captured in a torch.cuda.graph and replayed: the device's time without the host's — at these sizes a Python
autograd.Function costs more on the host than its kernels on the device).
These operators move a few hundred KiB each and are bound by launches, so no floor is quoted; the table says where the eager torch chain
wins.  There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnifusion_amd import build, ops  # noqa: E402

SHAPES = [(1, 18), (8, 18), (8, 46)]         # (bs, N)


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


def torch_attention(q, kv, bs, N):
    sp = lambda t: t.reshape(bs, N, 4, 128).permute(0, 2, 1, 3)
    p = torch.softmax(sp(q) @ sp(kv[:, :512]).transpose(-2, -1) * 128 ** -0.5, -1)
    return (p @ sp(kv[:, 512:])).permute(0, 2, 1, 3).reshape(bs * N, 512)


def torch_block(blk, x, bs, N):
    """ops.TransformerBlock.forward from torch's own operators on the same parameters"""
    y = F.layer_norm(x, (512,), blk.norm1.weight, blk.norm1.bias, 1e-5)
    a = torch_attention(F.linear(y, blk.attn.q.weight), F.linear(y, blk.attn.kv.weight), bs, N)
    x = x + F.linear(a, blk.attn.proj.weight, blk.attn.proj.bias)
    h = F.gelu(F.linear(F.layer_norm(x, (512,), blk.norm2.weight, blk.norm2.bias, 1e-5), blk.mlp.fc1.weight, blk.mlp.fc1.bias))
    return x + F.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r19a_transformer_bwd.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer_bwd_bench needs an MI355X: nothing is measured without one")
    dev = "cuda"
    torch.manual_seed(0)
    rows_out = []
    for bs, N in SHAPES:
        rows = bs * N
        leaf = lambda *s: torch.randn(*s, device=dev).requires_grad_(True)
        x, w, b, g = leaf(rows, 512), leaf(512), leaf(512), torch.randn(rows, 512, device=dev)
        h, gh = leaf(rows, 2048), torch.randn(rows, 2048, device=dev)
        q, kv = leaf(rows, 512), leaf(rows, 1024)
        blk = ops.TransformerBlock(512, 4).to(dev)
        params = list(blk.parameters())
        pairs = {
            "layer_norm": (lambda: ops.layer_norm(x, w, b, 1e-5), lambda: F.layer_norm(x, (512,), w, b, 1e-5), (x, w, b), g),
            "gelu": (lambda: ops.gelu(h), lambda: F.gelu(h), (h,), gh),
            "attention": (lambda: ops.attention(q, kv, bs), lambda: torch_attention(q, kv, bs, N), (q, kv), g),
            "block": (lambda: blk(x, bs), lambda: torch_block(blk, x, bs, N), [x] + params, g),
        }
        for name, (ours, theirs, leaves, grad) in pairs.items():
            ours_fb = lambda: torch.autograd.grad(ours(), leaves, grad)
            theirs_fb = lambda: torch.autograd.grad(theirs(), leaves, grad)
            t = {"ops_fwd": timed(ours, a.iters, a.repeats), "ops_fwd_bwd": timed(ours_fb, a.iters, a.repeats),
                 "torch_fwd": timed(theirs, a.iters, a.repeats), "torch_fwd_bwd": timed(theirs_fb, a.iters, a.repeats)}
            for key, fn in (("ops_fwd_bwd_graph", ours_fb), ("torch_fwd_bwd_graph", theirs_fb)):
                graph, keep = captured(fn)
                t[key] = timed(graph.replay, a.iters, a.repeats)
                del graph, keep
            rel = lambda p, r: ((p - r).abs().max() / r.abs().max().clamp_min(1e-30)).item()
            yo, yt = ours().detach(), theirs().detach()
            go, gt = ours_fb(), theirs_fb()
            diff = {"y": rel(yo, yt), "grads_max": max(rel(p, r) for p, r in zip(go, gt))}
            row = {"op": name, "bs": bs, "N": N, "rows": rows, "us": {k: round(v * 1e6, 2) for k, v in t.items()},
                   "fwd_over_torch": round(t["ops_fwd"] / t["torch_fwd"], 3), "fwd_bwd_over_torch": round(t["ops_fwd_bwd"] / t["torch_fwd_bwd"], 3),
                   "graph_fwd_bwd_over_torch": round(t["ops_fwd_bwd_graph"] / t["torch_fwd_bwd_graph"], 3), "vs_torch_rel_max": diff}
            rows_out.append(row)
            print("bs %d N %2d %-10s | fwd %7.1f us (%5.2fx torch %7.1f) | fwd+bwd %7.1f us (%5.2fx torch %7.1f) | graph fwd+bwd %7.1f us "
                  "(%5.2fx torch %7.1f) | rel. diff to torch y %.1e grads %.1e"
                  % (bs, N, name, t["ops_fwd"] * 1e6, row["fwd_over_torch"], t["torch_fwd"] * 1e6, t["ops_fwd_bwd"] * 1e6, row["fwd_bwd_over_torch"],
                     t["torch_fwd_bwd"] * 1e6, t["ops_fwd_bwd_graph"] * 1e6, row["graph_fwd_bwd_over_torch"], t["torch_fwd_bwd_graph"] * 1e6,
                     diff["y"], diff["grads_max"]), flush=True)
    out = {"tool": "tools/transformer_bwd_bench.py", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "repeats": a.repeats, "timing": "device events, median of the windows, warm-up of 3 calls per operator",
           "rows": rows_out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
