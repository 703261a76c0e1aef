"""The supervision of the reference's segmentation script (train_erp_sem.py:203-210): cross-entropy, the label map and the confusion matrix.

    loss = cross_entropy(equi_outputs, sem, ignore_index=-1)             # = F.cross_entropy(...), 0-d tensor on the device, differentiable
    loss, pred_ids, confusion = segmentation_step(equi_outputs, sem)     # + equi_outputs.argmax(1) and iou.confusion_matrix(pred, sem)

Everything numeric runs in libomnifusion_hip.so (csrc/omni_semantic.hip): ONE pass over the logits gives all three results, the backward is one
element-wise pass from the per-pixel log-sum-exp the forward saved, and nothing is copied to the host.

Layout: logits are converted, not refused — a non-contiguous view is made contiguous and a half / bfloat16 / float64 tensor is cast to float32
(autograd sees both conversions); an int32 / int16 / uint8 target is widened to int64.  A floating-point or boolean target, a shape mismatch,
C outside [2, 64] and CPU tensors raise ValueError.

Pixel rules: `target == ignore_index` is outside the loss; a negative target is outside the matrix (the reference's `gt_ids >= 0`);
a target that is neither ignored nor in [0, C) — torch raises a device-side assert for it — is dropped from both and counted: pass
`n_bad=` (a 1-element int64 device tensor) to accumulate the count, or read `last_n_bad(loss)` of a result.
"""
import torch

from .. import _lib
from .._lib import ptr as _p

MAX_CLASSES = 64
_INT_TARGETS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _check(logits, target, n_classes=None):
    for t, name in ((logits, "logits"), (target, "target")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if logits.dim() < 2 or not logits.is_floating_point():
        raise ValueError(f"logits must be a floating-point tensor [B, C, ...], got {logits.dtype} {tuple(logits.shape)}")
    if target.dtype not in _INT_TARGETS:
        raise ValueError(f"target must hold integer class indices (it is widened to int64), got {target.dtype}")
    C = logits.shape[1]
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"2 <= C <= {MAX_CLASSES} classes are supported, got C = {C}")
    if tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError(f"target {tuple(target.shape)} does not match logits {tuple(logits.shape)}: expected [B, ...] of the same batch and image size")
    if logits.numel() == 0:
        raise ValueError("empty batch")
    K = C if n_classes is None else int(n_classes)
    if not C <= K <= MAX_CLASSES:
        raise ValueError(f"n_classes must lie in [C, {MAX_CLASSES}] = [{C}, {MAX_CLASSES}], got {K}")
    for t, name in ((logits, "logits"), (target, "target")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if target.device != logits.device:
        raise ValueError("logits and target must live on the same device")
    return C, K


def _check_counter(t, name, shape, device):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous int64 tensor {shape} on {device} (it is accumulated in place)")


class _SemanticStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, K, confusion, want_pred):
        lib = _lib.load()
        B, C = logits.shape[0], logits.shape[1]
        HW = logits.numel() // (B * C)
        ws = torch.empty(lib.omni_semantic_workspace_bytes(B * HW), dtype=torch.uint8, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        pred = torch.empty(target.shape, dtype=torch.int64, device=logits.device) if want_pred else None
        with torch.cuda.device(logits.device):
            _lib.check(lib.omni_semantic_step_f32(_p(logits), _p(target), B, C, HW, ignore_index, K, _p(ws), _p(loss), _p(pred), _p(confusion),
                                                  _lib.stream_of(logits)), "semantic_step")
        ctx.save_for_backward(logits, target, ws)
        ctx.ignore_index = ignore_index
        head = ws[:16].view(torch.int64)                     # [count of valid pixels, n_bad], on the device
        if pred is None:
            pred = torch.empty(0, dtype=torch.int64, device=logits.device)
        ctx.mark_non_differentiable(pred, head)
        return loss, pred, head

    @staticmethod
    def backward(ctx, grad_out, _gp, _gh):
        logits, target, ws = ctx.saved_tensors
        lib = _lib.load()
        B, C = logits.shape[0], logits.shape[1]
        HW = logits.numel() // (B * C)
        g = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            _lib.check(lib.omni_semantic_grad_f32(_p(logits), _p(target), B, C, HW, ctx.ignore_index, _p(ws), _p(g), _p(grad),
                                                  _lib.stream_of(logits)), "semantic_grad")
        return grad, None, None, None, None, None


def _run(logits, target, ignore_index, K, confusion, want_pred, n_bad):
    x = logits.contiguous().to(torch.float32)
    t = target.contiguous().to(torch.int64)
    loss, pred, head = _SemanticStep.apply(x, t, int(ignore_index), K, confusion, want_pred)
    if n_bad is not None:
        n_bad += head[1]
    loss._omni_semantic_head = head
    return loss, pred


def last_n_bad(loss):
    """The int64 device scalar n_bad of the call that returned `loss`: the pixels dropped because their target is neither ignored nor a class index."""
    return loss._omni_semantic_head[1]


def valid_count(loss):
    """The int64 device scalar count of the pixels the mean of `loss` runs over."""
    return loss._omni_semantic_head[0]


def cross_entropy(logits, target, ignore_index=-1, n_bad=None):
    """F.cross_entropy(logits, target, ignore_index=ignore_index) with mean reduction for logits [B, C, H, W] and target [B, H, W]: a 0-d float32
    tensor on the device, differentiable w.r.t. `logits`.  All pixels ignored: NaN with a zero gradient, as in torch."""
    _check(logits, target)
    _check_counter(n_bad, "n_bad", (1,), logits.device)
    return _run(logits, target, ignore_index, 0, None, False, n_bad)[0]


def segmentation_step(logits, target, ignore_index=-1, confusion=None, n_classes=None, n_bad=None):
    """-> (loss, pred_ids, confusion) from one pass over `logits`: the cross-entropy above, logits.argmax(1) as int64 [B, H, W] (torch's rules:
    the first index of the maximum, a NaN counts as the maximum) and the int64 [K, K] matrix of iou.confusion_matrix(pred_ids, target), rows =
    predictions, K = n_classes or C.  `confusion=` is accumulated in place and returned; None starts from zeros."""
    C, K = _check(logits, target, n_classes)
    _check_counter(confusion, "confusion", (K, K), logits.device)
    _check_counter(n_bad, "n_bad", (1,), logits.device)
    if confusion is None:
        confusion = torch.zeros(K, K, dtype=torch.int64, device=logits.device)
    loss, pred = _run(logits, target, ignore_index, K, confusion, True, n_bad)
    return loss, pred, confusion
