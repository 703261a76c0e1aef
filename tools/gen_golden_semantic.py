"""G18a-d: torch's own F.cross_entropy (CPU, float64 and float32) and the reference's own iou.py for the seeded inputs of
tests/_semantic_cases.py.  Needs the reference checkout (its iou.py is imported, never copied); writes arrays and text only.

    python tools/gen_golden_semantic.py

Each fixture holds the input checksums, the float64 loss and gradient, the reference's own float32-against-float64 errors (`ref32_loss_err`;
`ref32_grad_max` on gradient x valid count, whose entries are softmax - onehot), logits.argmax(1), the confusion matrix of iou.confusion_matrix
(K = C), and — for the 13-class cases a and b — the 13 (iou, tp, denom) triples of iou.get_iou, `mean_iou` and the text iou.evaluate prints.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_iou():
    from oracle import ref_loader
    spec = importlib.util.spec_from_file_location("reference_iou", os.path.join(ref_loader.REFERENCE_ROOT, "iou.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def confusion_of(pred, gt, K):
    """iou.py:21-24 for K classes (the reference hard-codes 13), in numpy: the cases' labels are all in range"""
    ok = gt >= 0
    return np.bincount(pred[ok] * K + gt[ok], minlength=K * K).reshape(K, K).astype(np.int64)


def build(name):
    import torch
    import _semantic_cases as sc
    c = sc.case(name)
    K = c["n_classes"]
    l64, g64, count = sc.reference_cross_entropy(c, torch.float64)
    l32, g32, _ = sc.reference_cross_entropy(c, torch.float32)
    pred = torch.from_numpy(c["logits"]).argmax(1).numpy()
    assert (pred == torch.from_numpy(c["logits"]).double().argmax(1).numpy()).all()
    gt = c["target"]
    assert gt.max() < K and pred.max() < K
    conf = confusion_of(pred.reshape(-1), gt.reshape(-1), K)
    out = dict(loss=np.float64(l64), grad=g64, count=np.int64(count), ref32_loss_err=np.float64(abs(l32 - l64)),
               ref32_grad_max=np.float64(np.abs(g32.astype(np.float64) * count - g64 * count).max()), pred=pred.astype(np.int64), confusion=conf)
    if K == 13:
        ref = reference_iou()
        assert (ref.confusion_matrix(pred.reshape(-1), gt.reshape(-1)).astype(np.int64) == conf).all()
        triples = [ref.get_iou(i, conf.astype(np.ulonglong)) for i in range(13)]
        assert all(isinstance(t, tuple) for t in triples), f"{name}: a class is absent from both maps: pick other seeds"
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            mean = ref.evaluate(pred, gt)
        out.update(iou=np.array([t[0] for t in triples], np.float64), tp=np.array([t[1] for t in triples], np.int64),
                   denom=np.array([t[2] for t in triples], np.int64), mean_iou=np.float64(mean), evaluate_text=np.array(buf.getvalue()))
    out.update(sc.checksums(c))
    return c, out


def main():
    import _semantic_cases as sc
    for name in sc.NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_semantic.npz")
        np.savez_compressed(path, **out)
        print(name, c["logits"].shape, f"loss {float(out['loss']):.8f} ref32 loss err {float(out['ref32_loss_err']):.1e} ref32 grad max "
              f"{float(out['ref32_grad_max']):.1e} count {int(out['count'])} trace {int(np.trace(out['confusion']))} "
              f"mean_iou {float(out.get('mean_iou', np.nan)):.6f} {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
