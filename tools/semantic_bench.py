"""Segmentation supervision timing: the fused HIP step (cross-entropy + argmax + confusion matrix, csrc/omni_semantic.hip), its backward
and the confusion matrix alone against torch-eager on the same GPU in the same run: F.cross_entropy + argmax(1) + torch.bincount, forward and
autograd backward.

    python tools/semantic_bench.py [--rounds 5] [--iters 10] [--out profiles/r11a_semantic.json] [--quick]

Method (as tools/dibr_bench.py): device events over warm loops; the legs are INTERLEAVED (every round times each leg once, the median over
the rounds is reported with the spread) and every call of a loop takes the next of `--bufs` copies of the inputs, so that no call finds its
logits in the 256-MB memory-side cache.  The backward alone is timed directly: the HIP gradient kernel through its autograd node, torch's
through torch.autograd.grad on a retained graph.

Shapes: C = 13 at 512 x 1024, B = 8 and B = 1; labels in constant rectangles (a real label map), logits biased towards the label, 5 %
ignored; and B = 8 with i.i.d. labels and logits (every lane of a wave in another bin: the worst case of the histogram).

Compulsory bytes: step = logits + int64 target read, int64 pred + float32 lse written (72 B per pixel at C = 13); backward = logits +
target + lse read, gradient written; confusion matrix = two int64 maps read.  The fraction printed is bytes / time / 8 TB/s.
Parity: |loss - torch float64 loss|, max |grad - torch float64 grad| x count, and pred / matrix equality with torch's, on the timed inputs.
--quick: B = 1 only, few iterations (for a rocprofv3 --kernel-trace --stats run).
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

DEV = "cuda:0"


def make_inputs(B, C, H, W, kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "rectangles":
        cells = torch.randint(0, C, (B, H // 32 + 1, W // 32 + 1), device=DEV, generator=g)
        target = cells.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
        bias = 3.0
    else:
        target = torch.randint(0, C, (B, H, W), device=DEV, generator=g)
        bias = 0.0
    logits = torch.rand(B, C, H, W, device=DEV, generator=g) * 6.0 - 3.0
    logits.scatter_add_(1, target[:, None], torch.full((B, 1, H, W), bias, device=DEV))
    target[torch.rand(B, H, W, device=DEV, generator=g) < 0.05] = -1
    return logits, target


def torch_step(x, t, C):
    loss = F.cross_entropy(x, t, ignore_index=-1)
    pred = x.argmax(1)
    ok = t >= 0
    conf = torch.bincount(pred[ok] * C + t[ok], minlength=C * C).reshape(C, C)
    return loss, pred, conf


def torch_confusion(pred, t, C):
    ok = t >= 0
    return torch.bincount(pred[ok] * C + t[ok], minlength=C * C).reshape(C, C)


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
    assert torch.cuda.is_available(), "semantic_bench measures on an MI355X; there is no CPU timing"
    from omnifusion_amd import iou
    from omnifusion_amd.build import source_hash
    from omnifusion_amd.supervision import segmentation_step
    from omnifusion_amd.supervision.semantic import valid_count
    C, H, W = 13, 512, 1024
    cases = [(1, "rectangles")] if a.quick else [(8, "rectangles"), (1, "rectangles"), (8, "iid")]
    rounds, iters = (2, 3) if a.quick else (a.rounds, a.iters)
    rows = []
    for B, kind in cases:
        bufs = [make_inputs(B, C, H, W, kind, 100 + k) for k in range(a.bufs)]
        xs = [x.requires_grad_(True) for x, _ in bufs]
        ts = [t for _, t in bufs]
        npix = B * H * W
        # ---- parity on the first buffer
        x0, t0 = xs[0], ts[0]
        loss, pred, conf = segmentation_step(x0, t0)
        grad, = torch.autograd.grad(loss, x0)
        x64 = x0.detach().double().requires_grad_(True)
        l64, p_t, c_t = torch_step(x64, t0, C)
        g64, = torch.autograd.grad(l64, x64)
        l32, _, _ = torch_step(x0.detach(), t0, C)
        count = int(valid_count(loss))
        parity = dict(loss_err_vs_f64=abs(float(loss) - float(l64)), torch_f32_loss_err_vs_f64=abs(float(l32) - float(l64)),
                      grad_x_count_max_err_vs_f64=float(((grad.double() - g64) * count).abs().max()),
                      pred_equal=bool(torch.equal(pred, p_t)), confusion_equal=bool(torch.equal(conf, c_t)),
                      confusion_alone_equal=bool(torch.equal(iou.confusion_matrix(pred, t0), c_t)), valid_pixels=count)
        del x64, g64, grad
        # ---- the legs; graphs for the backward-only legs are built once per buffer and retained
        hip_loss = [segmentation_step(x, t)[0] for x, t in zip(xs, ts)]
        tor_loss = [F.cross_entropy(x, t, ignore_index=-1) for x, t in zip(xs, ts)]
        preds = [x.detach().argmax(1) for x in xs]
        acc = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        n = a.bufs

        def no_grad(fn):
            def run(k):
                with torch.no_grad():
                    fn(k)
            return run
        legs = {
            "hip_step": no_grad(lambda k: segmentation_step(xs[k % n], ts[k % n], confusion=acc)),
            "torch_step": no_grad(lambda k: torch_step(xs[k % n], ts[k % n], C)),
            "hip_bwd": lambda k: torch.autograd.grad(hip_loss[k % n], xs[k % n], retain_graph=True),
            "torch_bwd": lambda k: torch.autograd.grad(tor_loss[k % n], xs[k % n], retain_graph=True),
            "hip_confusion": no_grad(lambda k: iou.confusion_matrix(preds[k % n], ts[k % n], C, acc)),
            "torch_confusion": no_grad(lambda k: torch_confusion(preds[k % n], ts[k % n], C)),
        }
        for fn in legs.values():                                            # warm every leg on every buffer
            for k in range(n):
                fn(k)
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                times[name].append(time_loop(fn, iters))
        nbytes = {"hip_step": npix * (4 * C + 8 + 8 + 4), "hip_bwd": npix * (4 * C + 8 + 4 + 4 * C), "hip_confusion": npix * 16}
        row = dict(B=B, C=C, H=H, W=W, labels=kind, rounds=rounds, iters=iters, bufs=n, parity=parity)
        for name, v in times.items():
            row[name + "_us"] = round(statistics.median(v), 1)
            row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
        for name, nb in nbytes.items():
            row[name + "_compulsory_bytes"] = nb
            row[name + "_frac_of_8TBps"] = round(nb / (statistics.median(times[name]) * 1e-6) / 8e12, 4)
        for k in ("step", "bwd", "confusion"):
            row["speedup_" + k] = round(statistics.median(times["torch_" + k]) / statistics.median(times["hip_" + k]), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del bufs, xs, ts, hip_loss, tor_loss, preds
        torch.cuda.empty_cache()
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
