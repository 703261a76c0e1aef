"""Seeded inputs of the segmentation fixtures G18a-d (tools/gen_golden_semantic.py): logits [B, C, H, W] float32 and a label map [B, H, W]
int64.  The tests regenerate the same inputs; only the references' results and input checksums are stored in tests/golden/.

  a  B = 2, C = 13, 17 x 40   680 pixels per item — no multiple of a wave or a block; about 10 % of the labels are -1; i.i.d. labels
  b  B = 3, C = 13, 33 x 65   odd width (one pixel per lane), several blocks and a tail; labels in constant rectangles and logits biased
                              towards the label: most lanes of a wave hit one bin of the matrix
  c  B = 1, C = 2,  8 x 16    the fewest classes
  d  B = 1, C = 64, 5 x 7     the most classes, fewer pixels than one wave

Logits are uniform in [-3, 3) plus `bias` on the label's plane: |x| < 8, where a float32 softmax keeps every term.  a and b hold all 13
classes (the reference's `evaluate` fails on an absent class)."""
import numpy as np

from _util import rng_uniform

NAMES = ("G18a", "G18b", "G18c", "G18d")
SHAPES = {"G18a": (2, 13, 17, 40), "G18b": (3, 13, 33, 65), "G18c": (1, 2, 8, 16), "G18d": (1, 64, 5, 7)}
IGNORE_INDEX = -1


def _labels(name):
    B, C, H, W = SHAPES[name]
    k = NAMES.index(name)
    s = 1800 + 10 * k
    if name == "G18b":
        # constant rectangles of 11 x 13 pixels, classes in a seeded order that starts with every class once
        ry, rx = -(-H // 11), -(-W // 13)
        cells = np.floor(rng_uniform(s + 1, (B, ry, rx)) * C).astype(np.int64)
        cells.reshape(-1)[:C] = np.arange(C)
        lab = np.repeat(np.repeat(cells, 11, axis=1), 13, axis=2)[:, :H, :W]
        return np.ascontiguousarray(lab)
    lab = np.floor(rng_uniform(s + 1, (B, H, W)) * C).astype(np.int64)
    if name == "G18a":
        lab[rng_uniform(s + 2, (B, H, W)) < 0.1] = IGNORE_INDEX
    n = min(C, H * W)
    lab.reshape(-1)[:n] = np.arange(n)                                # every class occurs
    return lab


def case(name):
    """-> dict(logits float32 [B,C,H,W], target int64 [B,H,W], ignore_index, n_classes)."""
    B, C, H, W = SHAPES[name]
    k = NAMES.index(name)
    s = 1800 + 10 * k
    target = _labels(name)
    bias = 4.0 if name == "G18b" else 1.5
    logits = (rng_uniform(s + 3, (B, C, H, W)) * 6.0 - 3.0).astype(np.float32)
    onehot = (np.arange(C)[None, :, None, None] == target[:, None]).astype(np.float32)
    logits = (logits + np.float32(bias) * onehot).astype(np.float32)
    return dict(logits=logits, target=target, ignore_index=IGNORE_INDEX, n_classes=C)


def checksums(c):
    return {"sum_logits": np.float64(c["logits"].astype(np.float64).sum()), "sum_target": np.int64(c["target"].sum()),
            "sum_target_sq": np.int64((c["target"] * c["target"]).sum())}


def reference_cross_entropy(c, dtype, scale=1.0):
    """torch's own F.cross_entropy on the CPU in `dtype` -> (loss float, gradient w.r.t. the logits as numpy `dtype`, valid count)."""
    import torch
    x = (torch.from_numpy(c["logits"]).to(dtype) * scale).requires_grad_(True)
    t = torch.from_numpy(c["target"])
    loss = torch.nn.functional.cross_entropy(x, t, ignore_index=c["ignore_index"])
    loss.backward()
    return float(loss.detach()), x.grad.numpy(), int((c["target"] != c["ignore_index"]).sum())


def loss_gate(g):
    """max(4 x the reference's own float32 error, 1 ulp of the loss)"""
    return max(4.0 * float(g["ref32_loss_err"]), float(np.spacing(np.float32(g["loss"]))))


def grad_gate(g):
    """on gradient x count (entries softmax - onehot, |.| <= 1): max(4 x the reference's own float32 error, 8 x 2^-23)"""
    return max(4.0 * float(g["ref32_grad_max"]), 8.0 * 2.0 ** -23)
