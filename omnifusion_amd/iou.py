"""Segmentation scores on the device — host-side mirror of the reference's iou.py (used at train_erp_sem.py:278).

    confusion = confusion_matrix(pred_ids, gt_ids)       # int64 [13, 13] on the device; rows = predictions, columns = ground truth
    mean_iou = evaluate(pred_ids, gt_ids)                # same return value and the same printed table as the reference

    meters = SegmentationMetrics()
    meters.update(equi_outputs, sem)                     # logits [B, C, H, W] (argmax in the same pass) or an int64 label map
    print(meters.mean_iou())

The histogram runs in libomnifusion_hip.so (csrc/omni_semantic.hip); `get_iou` / `evaluate` copy only the K*K integers to the host and redo
the reference's Python float arithmetic in its order (`mean_iou += iou / 13` per class), so that — the counts being exact — the mean and the
printed text are IDENTICAL to the reference's, not merely close.

Divergences: a pair whose gt is >= K or whose prediction is outside [0, K) is dropped and counted in `n_bad` (the reference's
`pred*13 + gt` spills into the next row or makes `reshape` fail); for a class absent from both maps the reference's `get_iou` returns a bare
float('nan') and its `evaluate` then dies with TypeError on `[0]` — here `get_iou` returns (nan, 0, 0) and `evaluate` a NaN mean.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p

# the reference's constants (iou.py:12-16), as it ships them
VALID_CLASS_IDS = np.array([0, 1])
CLASS_LABELS = ['beam', 'board', 'bookcase', 'ceiling', 'chair', 'clutter', 'column', 'door', 'floor', 'sofa', 'table', 'wall', 'window']
UNKNOWN_ID = -100
N_CLASSES = len(CLASS_LABELS)


def printout(flog, data):
    flog.write(data + '\n')


def _label_map(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold integer class indices, got {t.dtype}")
    return t.contiguous().to(torch.int64)


def confusion_matrix(pred_ids, gt_ids, n_classes=N_CLASSES, confusion=None, n_bad=None):
    """int64 [K, K] device tensor: confusion[p, g] = number of pixels with prediction p and label g, over the pixels with gt >= 0
    (iou.py:21-24).  `confusion=` is accumulated in place; `n_bad=` (1-element int64 device tensor) accumulates the dropped pairs."""
    pred, gt = _label_map(pred_ids, "pred_ids"), _label_map(gt_ids, "gt_ids")
    if pred.shape != gt.shape:
        raise ValueError(f"pred_ids {tuple(pred.shape)} and gt_ids {tuple(gt.shape)} must have the same shape")
    K = int(n_classes)
    if not 1 <= K <= 64:
        raise ValueError(f"1 <= n_classes <= 64 supported, got {K}")
    if confusion is None:
        confusion = torch.zeros(K, K, dtype=torch.int64, device=pred.device)
    for t, name, shape in ((confusion, "confusion", (K, K)), (n_bad, "n_bad", (1,))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous()
                              or t.device != pred.device):
            raise ValueError(f"{name} must be a contiguous int64 tensor {shape} on {pred.device} (it is accumulated in place)")
    lib = _lib.load()
    with torch.cuda.device(pred.device):
        _lib.check(lib.omni_confusion_matrix_i64(_p(pred), _p(gt), pred.numel(), K, _p(confusion), _p(n_bad), _lib.stream_of(pred)),
                   "confusion_matrix")
    return confusion


def _host(confusion):
    """the K*K counts as Python-int rows (the only device->host copy of this module)"""
    if isinstance(confusion, torch.Tensor):
        confusion = confusion.detach().cpu().numpy()
    return np.asarray(confusion).astype(np.int64)


def get_iou(label_id, confusion):
    """(iou, tp, tp + fp + fn) of one class, iou.py:26-37; (nan, 0, 0) for a class absent from both maps."""
    c = _host(confusion)
    tp = int(c[label_id, label_id])
    fp = int(c[label_id, :].sum()) - tp
    fn = int(c[:, label_id].sum()) - tp
    denom = tp + fp + fn
    if denom == 0:
        return (float('nan'), 0, 0)
    return (float(tp) / denom, tp, denom)


def evaluate_confusion(confusion, n_points, flog=None):
    """The host half of `evaluate`: the table and the mean of iou.py:39-57 from a finished 13 x 13 matrix."""
    c = _host(confusion)
    if c.shape != (N_CLASSES, N_CLASSES):
        raise ValueError(f"evaluate scores the {N_CLASSES} classes of CLASS_LABELS: confusion must be {N_CLASSES} x {N_CLASSES}, got {c.shape}")
    print('evaluating', n_points, 'points...')
    class_ious = {}
    mean_iou = 0
    for i in range(N_CLASSES):
        label_name = CLASS_LABELS[i]
        class_ious[label_name] = get_iou(i, c)
        mean_iou += class_ious[label_name][0] / 13

    print('classes          IoU')
    print('----------------------------')
    for i in range(N_CLASSES):
        label_name = CLASS_LABELS[i]
        line = '{0:<14s}: {1:>5.3f}   ({2:>6d}/{3:<6d})'.format(label_name, class_ious[label_name][0], class_ious[label_name][1], class_ious[label_name][2])
        if flog is not None:
            printout(flog, line)
        print(line)
    print('mean IOU: %f' % mean_iou)
    return mean_iou


def evaluate(pred_ids, gt_ids, flog=None):
    """iou.py:39-57 for device label maps: prints the reference's table and returns its mean IoU."""
    return evaluate_confusion(confusion_matrix(pred_ids, gt_ids), gt_ids.numel(), flog)


class SegmentationMetrics:
    """The confusion matrix of an evaluation loop, kept on the device (the counterpart of eval.DepthMetrics): nothing is copied to the host
    until a score is asked for."""

    def __init__(self, n_classes=N_CLASSES, ignore_index=-1):
        self.n_classes = int(n_classes)
        self.ignore_index = ignore_index
        self.confusion = None
        self.n_bad = None

    def _init(self, device):
        if self.confusion is None:
            self.confusion = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int64, device=device)
            self.n_bad = torch.zeros(1, dtype=torch.int64, device=device)

    def update(self, logits_or_pred, gt):
        """logits [B, C, H, W] (floating point; the argmax is taken in the same pass, C <= n_classes) or a label map shaped like `gt`.
        -> the label map that was scored."""
        if not isinstance(logits_or_pred, torch.Tensor) or not logits_or_pred.is_cuda:
            raise ValueError("logits_or_pred must be a tensor on an MI355X device; there is no CPU path")
        self._init(logits_or_pred.device)
        if logits_or_pred.is_floating_point():
            from .supervision.semantic import segmentation_step
            with torch.no_grad():
                _, pred, _ = segmentation_step(logits_or_pred, gt, self.ignore_index, self.confusion, self.n_classes, self.n_bad)
            return pred
        confusion_matrix(logits_or_pred, gt, self.n_classes, self.confusion, self.n_bad)
        return logits_or_pred

    def class_ious(self):
        """[(iou, tp, tp + fp + fn)] per class."""
        if self.confusion is None:
            return [(float('nan'), 0, 0)] * self.n_classes
        c = _host(self.confusion)
        return [get_iou(i, c) for i in range(self.n_classes)]

    def mean_iou(self, skip_absent=False):
        """Sum of iou / n_classes in class order (the reference's arithmetic: NaN as soon as one class is absent from both maps);
        skip_absent=True: the mean over the classes that occur."""
        return _mean(self.class_ious(), self.n_classes, skip_absent)

    def averages_all_ranks(self, skip_absent=False):
        """Mean IoU over the matrices of every rank of an image-sharded run (omnifusion_amd/dist.py): the integer matrix is all-reduced once,
        at the end — not on the data path.  Every rank must call it, also one that scored nothing."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if self.confusion is None:
                # a rank without data still enters the collective, with zeros (raising here would leave the others waiting in all_reduce)
                dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() and dist.get_backend() == "nccl" else torch.device("cpu")
                self.confusion = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int64, device=dev)
                self.n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
            t = torch.cat([self.confusion.reshape(-1), self.n_bad])
            if dist.get_backend() != "nccl":
                t = t.cpu()
            dist.all_reduce(t)
            c = _host(t[:-1].reshape(self.n_classes, self.n_classes))
            return _mean([get_iou(i, c) for i in range(self.n_classes)], self.n_classes, skip_absent)
        if self.confusion is None:
            raise RuntimeError("no batch has been scored")
        return self.mean_iou(skip_absent)


def _mean(ious, n_classes, skip_absent):
    if skip_absent:
        seen = [v[0] for v in ious if v[2] > 0]
        return sum(seen) / len(seen) if seen else float('nan')
    mean_iou = 0
    for v in ious:
        mean_iou += v[0] / n_classes
    return mean_iou
