"""GPU: the fused segmentation step, its backward and the confusion matrix (csrc/omni_semantic.hip) against the G18a-d fixtures (torch's own
float64 F.cross_entropy and the reference's iou.py, tools/gen_golden_semantic.py), and the properties the fixtures cannot show: contention,
ties and NaN, range, nothing valid, out-of-range labels, exactness, determinism and layout.

Gates (tests/_semantic_cases.py): loss max(4 x ref32_loss_err, 1 ulp of the loss); gradient x count max(4 x ref32_grad_max, 8 x 2^-23) on
entries of magnitude <= 1.  The factor 4: the summation order and the device's expf / logf differ from torch's, each within a few ulp; four
times the reference's own float32 noise covers that without hiding a wrong term.  Every parity test prints its measured errors beside the gates."""
import numpy as np
import pytest
import torch

import _semantic_cases as sc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_RESULTS = {}


def run(name):
    """One step + backward per case, shared by the tests and left unchanged -> dict of host arrays."""
    if name not in _RESULTS:
        from omnifusion_amd.supervision import segmentation_step
        from omnifusion_amd.supervision.semantic import last_n_bad, valid_count
        c = sc.case(name)
        x = t(c["logits"]).requires_grad_(True)
        loss, pred, conf = segmentation_step(x, t(c["target"]), ignore_index=c["ignore_index"])
        loss.backward()
        _RESULTS[name] = dict(loss=loss.detach().cpu().numpy(), pred=pred.cpu().numpy(), confusion=conf.cpu().numpy(), grad=x.grad.cpu().numpy(),
                              count=int(valid_count(loss)), n_bad=int(last_n_bad(loss)), pred_dev=pred, case=c)
    return _RESULTS[name]


@pytest.mark.parametrize("name", sc.NAMES)
def test_parity_with_the_fixtures(name, capsys):
    from omnifusion_amd import iou
    g, r = golden(name + "_semantic"), run(name)
    assert r["pred"].dtype == np.int64 and (r["pred"] == g["pred"]).all()
    assert r["confusion"].dtype == np.int64 and (r["confusion"] == g["confusion"]).all()
    assert r["count"] == int(g["count"]) and r["n_bad"] == 0
    assert r["loss"].dtype == np.float32 and r["loss"].shape == ()
    le = abs(float(r["loss"]) - float(g["loss"]))
    ge = float(np.abs(r["grad"].astype(np.float64) * r["count"] - g["grad"] * r["count"]).max())
    print(f"{name}: loss err {le:.3e} (gate {sc.loss_gate(g):.3e})  grad x count err {ge:.3e} (gate {sc.grad_gate(g):.3e})")
    assert le <= sc.loss_gate(g), (name, le)
    assert ge <= sc.grad_gate(g), (name, ge)
    if name in ("G18a", "G18b"):
        capsys.readouterr()
        mean = iou.evaluate(r["pred_dev"], t(r["case"]["target"]))
        assert mean == float(g["mean_iou"])
        assert capsys.readouterr().out == str(g["evaluate_text"])
        assert iou.get_iou(3, iou.confusion_matrix(r["pred_dev"], t(r["case"]["target"]))) == (float(g["iou"][3]), int(g["tp"][3]), int(g["denom"][3]))


def test_cross_entropy_alone_equals_the_step():
    from omnifusion_amd.supervision import cross_entropy
    r = run("G18a")
    x = t(r["case"]["logits"]).requires_grad_(True)
    loss = cross_entropy(x, t(r["case"]["target"]))
    (3.0 * loss).backward()
    assert loss.detach().cpu().numpy().tobytes() == r["loss"].tobytes()
    assert np.abs(x.grad.cpu().numpy() - 3.0 * r["grad"]).max() <= 3.0 * 2.0 ** -21 / r["count"]           # grad_out reaches the kernel (three float32 roundings of entries <= 3 / count)


def test_worst_case_contention():
    """every lane of every wave hits ONE bin"""
    from omnifusion_amd import iou
    from omnifusion_amd.supervision import segmentation_step
    x = torch.zeros(1, 13, 64, 128, device=DEV)
    x[:, 11] = 5.0
    gt = torch.full((1, 64, 128), 11, dtype=torch.int64, device=DEV)
    _, pred, conf = segmentation_step(x, gt)
    want = np.zeros((13, 13), np.int64)
    want[11, 11] = 8192
    assert (pred == 11).all() and (conf.cpu().numpy() == want).all()
    assert (iou.confusion_matrix(pred, gt).cpu().numpy() == want).all()


def test_ties_and_nan():
    from omnifusion_amd.supervision import segmentation_step
    c = sc.case("G18a")
    gt = t(c["target"])
    loss, pred, _ = segmentation_step(torch.full((2, 13, 17, 40), 0.25, device=DEV), gt)
    assert (pred == 0).all() and abs(float(loss) - np.log(13.0)) < 1e-6
    x = c["logits"].copy()
    assert c["target"][1, 9, 21] >= 0 and run("G18a")["pred"][1, 9, 21] != 5
    x[1, 5, 9, 21] = np.nan
    xg = t(x).requires_grad_(True)
    loss, pred, _ = segmentation_step(xg, gt)
    loss.backward()
    pred = pred.cpu().numpy()
    assert pred[1, 9, 21] == 5 and np.isnan(float(loss))
    want = run("G18a")["pred"].copy()
    want[1, 9, 21] = 5
    assert (pred == want).all()
    g = xg.grad.cpu().numpy()
    assert np.isnan(g[1, :, 9, 21]).all() and np.isfinite(np.delete(g.reshape(2, 13, -1), 9 * 40 + 21, axis=2)[1]).all() and np.isfinite(g[0]).all()
    # a NaN in a LATER plane than the running maximum, and one in plane 0
    x = c["logits"].copy()
    x[0, 12, 3, 3] = np.nan
    x[0, 0, 4, 4] = np.nan
    pred = segmentation_step(t(x), gt)[1].cpu().numpy()
    assert pred[0, 3, 3] == 12 and pred[0, 4, 4] == 0
    assert (pred == torch.from_numpy(x).argmax(1).numpy()).all()


def test_range():
    """logits x 1e4: the loss stays finite and inside the same relative gate against torch's float64"""
    from omnifusion_amd.supervision import cross_entropy
    c, g = sc.case("G18a"), golden("G18a_semantic")
    x = (c["logits"] * np.float32(1e4)).astype(np.float32)
    want, _, _ = sc.reference_cross_entropy(dict(c, logits=x), torch.float64)
    got = float(cross_entropy(t(x), t(c["target"])))
    rel = sc.loss_gate(g) / float(g["loss"])
    print(f"range: loss {got:.6e} want {want:.6e} rel err {abs(got - want) / want:.3e} (gate {rel:.3e})")
    assert np.isfinite(got) and abs(got - want) <= rel * want


def test_nothing_valid():
    from omnifusion_amd.supervision import segmentation_step
    c = sc.case("G18c")
    tgt = np.full_like(c["target"], -1)
    want, wgrad, _ = sc.reference_cross_entropy(dict(c, target=tgt), torch.float32)
    x = t(c["logits"]).requires_grad_(True)
    loss, _, conf = segmentation_step(x, t(tgt))
    loss.backward()
    assert np.isnan(want) and not wgrad.any()                                   # what torch returns: NaN and zeros
    assert np.isnan(float(loss)) and (x.grad.cpu().numpy() == wgrad).all() and not conf.cpu().numpy().any()


def test_out_of_range_labels_are_dropped_and_counted():
    from omnifusion_amd import iou
    from omnifusion_amd.supervision import segmentation_step
    from omnifusion_amd.supervision.semantic import last_n_bad
    c, r = sc.case("G18a"), run("G18a")
    bad, clean = c["target"].copy(), c["target"].copy()
    spots = [(0, 0, 5), (0, 16, 39), (1, 7, 7), (1, 8, 30), (1, 16, 0)]
    for k, s in enumerate(spots):
        assert c["target"][s] >= 0
        bad[s] = 13 if k % 2 == 0 else -100
        clean[s] = -1
    x = t(c["logits"])
    n_bad = torch.zeros(1, dtype=torch.int64, device=DEV)
    xb = x.clone().requires_grad_(True)
    loss_b, _, conf_b = segmentation_step(xb, t(bad), n_bad=n_bad)
    loss_b.backward()
    xc = x.clone().requires_grad_(True)
    loss_c, _, conf_c = segmentation_step(xc, t(clean))
    loss_c.backward()
    assert int(n_bad) == len(spots) == int(last_n_bad(loss_b)) and int(last_n_bad(loss_c)) == 0
    assert loss_b.detach().cpu().numpy().tobytes() == loss_c.detach().cpu().numpy().tobytes() and torch.equal(conf_b, conf_c) and torch.equal(xb.grad, xc.grad)
    assert int(conf_b.sum()) == int((c["target"] >= 0).sum()) - len(spots)
    # confusion_matrix: a prediction of 13 and of -1 and a label of 13 are dropped and counted; a label of -100 is skipped (gt_ids >= 0)
    pred = r["pred"].copy()
    pred[spots[0]], pred[spots[1]] = 13, -1
    gt = c["target"].copy()
    gt[spots[2]], gt[spots[3]] = 13, -100
    n_bad.zero_()
    conf = iou.confusion_matrix(t(pred), t(gt), n_bad=n_bad)
    for s in spots[:4]:
        gt[s] = -1
    pred[spots[0]], pred[spots[1]] = 0, 0
    assert int(n_bad) == 3 and torch.equal(conf, iou.confusion_matrix(t(pred), t(gt)))


def test_exactness_and_determinism():
    from omnifusion_amd import iou
    from omnifusion_amd.supervision import segmentation_step
    c, r = sc.case("G18b"), run("G18b")
    x, gt = t(c["logits"]), t(c["target"])
    items = [segmentation_step(x[b:b + 1], gt[b:b + 1])[2] for b in range(x.shape[0])]
    assert (sum(items).cpu().numpy() == r["confusion"]).all()                   # the matrix of a batch = the sum over its items
    acc = torch.zeros(13, 13, dtype=torch.int64, device=DEV)
    for _ in range(2):
        out = segmentation_step(x, gt, confusion=acc)[2]
        assert out is acc
    assert (acc.cpu().numpy() == 2 * r["confusion"]).all()                      # confusion= accumulates over two calls
    for _ in range(2):                                                          # identical bits from run to run, step and backward
        xg = x.clone().requires_grad_(True)
        loss, pred, conf = segmentation_step(xg, gt)
        loss.backward()
        assert loss.detach().cpu().numpy().tobytes() == r["loss"].tobytes() and xg.grad.cpu().numpy().tobytes() == r["grad"].tobytes()
        assert (pred.cpu().numpy() == r["pred"]).all() and (conf.cpu().numpy() == r["confusion"]).all()
    assert (iou.confusion_matrix(r["pred_dev"], gt).cpu().numpy() == r["confusion"]).all()     # the histogram alone = the fused step's
    m = iou.SegmentationMetrics()
    m.update(x, gt)
    m.update(r["pred_dev"], gt)
    assert (m.confusion.cpu().numpy() == 2 * r["confusion"]).all() and int(m.n_bad) == 0
    g = golden("G18b_semantic")
    assert m.mean_iou() == float(g["mean_iou"]) == m.averages_all_ranks()       # doubling every count leaves each ratio's float unchanged
    assert [v[0] for v in m.class_ious()] == [float(v) for v in g["iou"]]


def test_layout_is_converted():
    """a non-contiguous logits view and an int32 target are converted (supervision/semantic.py docstring), never read through a wrong stride;
    a wider class range (n_classes) pads the matrix"""
    from omnifusion_amd.supervision import segmentation_step
    c, r = sc.case("G18a"), run("G18a")
    nhwc = t(c["logits"].transpose(0, 2, 3, 1))                                 # [B, H, W, C] storage
    view = nhwc.permute(0, 3, 1, 2).requires_grad_(True)                        # [B, C, H, W] view with NHWC strides
    assert not view.is_contiguous()
    loss, pred, conf = segmentation_step(view, t(c["target"].astype(np.int32)), n_classes=16)
    loss.backward()
    assert loss.detach().cpu().numpy().tobytes() == r["loss"].tobytes() and (pred.cpu().numpy() == r["pred"]).all()
    assert conf.shape == (16, 16) and (conf.cpu().numpy()[:13, :13] == r["confusion"]).all() and int(conf.sum()) == int(r["confusion"].sum())
    assert view.grad.shape == view.shape and view.grad.cpu().numpy().tobytes() == r["grad"].tobytes()
    half = segmentation_step(t(c["logits"]).half(), t(c["target"]))[0]          # cast to float32, not refused
    assert abs(float(half) - float(r["loss"])) < 2e-3
