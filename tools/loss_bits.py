"""The bits of the losses and metrics: forward and backward of every operator that sums over a block, with fixed seeds, as a JSON file.

    python tools/loss_bits.py OUT.json

Per case: every scalar result as the hex bit pattern of its float32 and a SHA-256 of the bytes of every tensor result (gradients, label maps,
the confusion matrix).  Nothing in the file depends on the run, so two builds that add in the same order write byte-identical files — which
is what a change to the reductions (csrc/omni_reduce.h, the finals of the loss units) is checked with: run it on both builds, compare the files.

Operators: calculate_berhu_loss, calculate_l1_loss ([B,1,H,W] and [B,C,H,W] masks), the photometric loss (gaussian 7 and box 5),
geometry_terms (both terms), the semantic step with its confusion matrix, the depth metrics.  Shapes: 2 x 1 x 40 x 72; 3 x 3 x 90 x 150 (ragged
against every tile size in use); for BerHu and L1 also 2 x 1 x 300 x 257: 77 100 elements per item, more than the 256 blocks of 256 threads an item
gets, so the grid-stride loop wraps with a ragged tail.  Masks are binary at about 60 %.  geometry_terms takes one channel and the semantic step
13 classes, whatever the shape's C.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
SHAPES = [(2, 1, 40, 72), (3, 3, 90, 150)]
CAP_SHAPE = (2, 1, 300, 257)
CLASSES = 13


def bits(t):
    """hex bit patterns of the float32 values of a small tensor"""
    a = t.detach().to(torch.float32).cpu().numpy().reshape(-1).view(np.uint32)
    return [f"0x{int(v):08x}" for v in a]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rand(rng, shape, lo=0.0, hi=1.0):
    return torch.from_numpy((lo + (hi - lo) * rng.random(shape)).astype(np.float32)).to(DEV)


def mask_of(rng, shape):
    return torch.from_numpy((rng.random(shape) < 0.6).astype(np.float32)).to(DEV)


def with_grad(loss_of, pred):
    p = pred.clone().requires_grad_(True)
    loss = loss_of(p)
    total = loss if isinstance(loss, torch.Tensor) else sum(loss)
    grad, = torch.autograd.grad(total, p)
    losses = [loss] if isinstance(loss, torch.Tensor) else list(loss)
    return {"loss": [b for x in losses for b in bits(x)], "grad_sha256": sha(grad)}


def cases():
    from omnifusion_amd.eval import compute_eval_metrics
    from omnifusion_amd.supervision import geometry_terms
    from omnifusion_amd.supervision.direct import calculate_berhu_loss, calculate_l1_loss
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    from omnifusion_amd.supervision.semantic import last_n_bad, segmentation_step
    out = {}
    for si, (B, C, H, W) in enumerate(SHAPES + [CAP_SHAPE]):
        tag = f"{B}x{C}x{H}x{W}"
        rng = np.random.default_rng(4100 + si)
        pred, gt = rand(rng, (B, C, H, W), 0.5, 4.0), rand(rng, (B, C, H, W), 0.5, 4.0)
        full, one, wts = mask_of(rng, (B, C, H, W)), mask_of(rng, (B, 1, H, W)), rand(rng, (B, C, H, W), 0.5, 1.5)
        out[f"berhu {tag}"] = with_grad(lambda p: calculate_berhu_loss(p, gt, full, wts), pred)
        out[f"l1 mask1 {tag}"] = with_grad(lambda p: calculate_l1_loss(p, gt, one), pred)
        out[f"l1 maskC {tag}"] = with_grad(lambda p: calculate_l1_loss(p, gt, full), pred)
        if (B, C, H, W) == CAP_SHAPE:
            continue
        img_p, img_g = rand(rng, (B, C, H, W)), rand(rng, (B, C, H, W))
        for mode, window in (("gaussian", 7), ("box", 5)):
            params = PhotometricLossParameters(window=window, ssim_mode=mode)
            out[f"photometric {mode}{window} {tag}"] = with_grad(lambda p: calculate_loss(p, img_g, params, one, wts[:, :1]), img_p)
        depth_g = rand(rng, (B, 1, H, W), 1.0, 4.0)
        depth_p = depth_g + rand(rng, (B, 1, H, W), -0.2, 0.2)
        out[f"geometry_terms {B}x1x{H}x{W}"] = with_grad(lambda p: geometry_terms(p, depth_g, one), depth_p)
        logits = rand(rng, (B, CLASSES, H, W), -3.0, 3.0).requires_grad_(True)
        target = torch.from_numpy(rng.integers(-1, CLASSES, (B, H, W))).to(DEV)              # -1: ignored, about one pixel in 14
        loss, ids, confusion = segmentation_step(logits, target, ignore_index=-1)
        grad, = torch.autograd.grad(loss, logits)
        out[f"semantic {B}x{CLASSES}x{H}x{W}"] = {"loss": bits(loss), "grad_sha256": sha(grad), "pred_sha256": sha(ids), "confusion_sha256": sha(confusion),
                                                  "n_bad": int(last_n_bad(loss))}
        scaled = depth_p.clone()
        metrics = compute_eval_metrics(scaled, depth_g, one)
        out[f"depth_metrics {B}x1x{H}x{W}"] = {"metrics": bits(metrics), "scaled_sha256": sha(scaled)}
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    result = cases()
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(result)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
