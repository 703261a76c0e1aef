"""CPU: the host side of the segmentation path (omnifusion_amd/supervision/semantic.py, omnifusion_amd/iou.py, csrc/omni_semantic.hip) — names,
argument checks before any launch, the C boundary, the G18 fixtures against their seeded recipes (and, where the reference checkout is present,
against the reference itself), and the host half of get_iou / evaluate: exact equality with what the reference returned and printed."""
import ctypes
import io

import numpy as np
import pytest
import torch

import _semantic_cases as sc
from _util import golden

NEW_SYMBOLS = ("omni_semantic_workspace_bytes", "omni_semantic_step_f32", "omni_semantic_grad_f32", "omni_confusion_matrix_i64")


def test_modules_and_names():
    from omnifusion_amd import iou, supervision
    from omnifusion_amd.supervision import semantic
    assert supervision.cross_entropy is semantic.cross_entropy and supervision.segmentation_step is semantic.segmentation_step
    for name in ("VALID_CLASS_IDS", "CLASS_LABELS", "UNKNOWN_ID", "N_CLASSES", "confusion_matrix", "get_iou", "evaluate", "SegmentationMetrics"):
        assert hasattr(iou, name), name
    assert iou.N_CLASSES == 13 == len(iou.CLASS_LABELS) and iou.UNKNOWN_ID == -100
    m = iou.SegmentationMetrics()
    for name in ("update", "confusion", "class_ious", "mean_iou", "averages_all_ranks"):
        assert hasattr(m, name), name


def test_new_symbols_exported_and_listed():
    from omnifusion_amd import _lib, build
    build.build()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_semantic_workspace_bytes(1000) - L.omni_semantic_workspace_bytes(0) == 4000          # + one float of lse per pixel
    assert L.omni_semantic_workspace_bytes(0) >= 16


def test_c_boundary_refuses_before_a_launch():
    """Shapes the kernels do not cover return OMNI_ERR_INVALID / OMNI_ERR_UNSUPPORTED from the argument checks: no device is touched."""
    from omnifusion_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    step = lambda B, C, HW, K=0, logits=p: L.omni_semantic_step_f32(logits, p, B, C, HW, -1, K, p, p, None, None, None)
    assert step(1, 1, 4) == _lib.OMNI_ERR_UNSUPPORTED and b"2 <= C <= 64" in L.omni_last_error()
    assert step(1, 65, 4) == _lib.OMNI_ERR_UNSUPPORTED
    assert step(0, 13, 4) == _lib.OMNI_ERR_INVALID and step(1, 13, 0) == _lib.OMNI_ERR_INVALID
    assert step(1, 13, 4, logits=None) == _lib.OMNI_ERR_INVALID
    assert step(1, 13, 4, K=12) == _lib.OMNI_ERR_INVALID and step(1, 13, 4, K=65) == _lib.OMNI_ERR_INVALID
    assert L.omni_semantic_grad_f32(p, p, 1, 65, 4, -1, p, p, p, None) == _lib.OMNI_ERR_UNSUPPORTED
    assert L.omni_semantic_grad_f32(p, p, 1, 13, 4, -1, p, p, None, None) == _lib.OMNI_ERR_INVALID
    assert L.omni_confusion_matrix_i64(p, p, 4, 65, p, None, None) == _lib.OMNI_ERR_UNSUPPORTED
    assert L.omni_confusion_matrix_i64(p, p, 4, 0, p, None, None) == _lib.OMNI_ERR_UNSUPPORTED
    assert L.omni_confusion_matrix_i64(p, None, 4, 13, p, None, None) == _lib.OMNI_ERR_INVALID


def test_bad_arguments_raise_value_error():
    from omnifusion_amd import iou
    from omnifusion_amd.supervision import cross_entropy, segmentation_step
    x, t = torch.zeros(1, 13, 4, 8), torch.zeros(1, 4, 8, dtype=torch.int64)
    for fn in (cross_entropy, segmentation_step):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(x, t)
        with pytest.raises(ValueError, match="2 <= C <= 64"):
            fn(torch.zeros(1, 1, 4, 8), t)
        with pytest.raises(ValueError, match="2 <= C <= 64"):
            fn(torch.zeros(1, 65, 4, 8), t)
        with pytest.raises(ValueError, match="integer class indices"):
            fn(x, t.float())
        with pytest.raises(ValueError, match="does not match"):
            fn(x, torch.zeros(1, 4, 9, dtype=torch.int64))
        with pytest.raises(ValueError, match="does not match"):
            fn(x, torch.zeros(2, 4, 8, dtype=torch.int64))
        with pytest.raises(ValueError, match="floating-point"):
            fn(x.long(), t)
    with pytest.raises(ValueError, match="n_classes"):
        segmentation_step(x, t, n_classes=12)
    with pytest.raises(ValueError, match="no CPU path"):
        iou.confusion_matrix(t, t)
    with pytest.raises(ValueError, match="no CPU path"):
        iou.evaluate(t, t)
    with pytest.raises(ValueError, match="no CPU path"):
        iou.SegmentationMetrics().update(x, t)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_checksums_match_the_recipes(name):
    c, g = sc.case(name), golden(name + "_semantic")
    assert c["logits"].shape == sc.SHAPES[name] and c["logits"].dtype == np.float32 and c["target"].dtype == np.int64
    for k, v in sc.checksums(c).items():
        assert v == g[k], (name, k)
    B, C, H, W = sc.SHAPES[name]
    assert g["grad"].shape == (B, C, H, W) and g["grad"].dtype == np.float64 and g["pred"].shape == (B, H, W) and g["confusion"].shape == (C, C)
    assert int(g["count"]) == int((c["target"] != -1).sum()) and int(g["confusion"].sum()) == int((c["target"] >= 0).sum())
    if C == 13:
        assert set(np.unique(c["target"])) >= set(range(13))                  # the evaluate fixtures need every class
    if name == "G18a":
        assert 0.05 < (c["target"] == -1).mean() < 0.15


def test_case_a_reproduces_the_fixture_from_the_reference():
    from oracle import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("reference checkout not present")
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import gen_golden_semantic as gen
    _, out = gen.build("G18a")
    g = golden("G18a_semantic")
    assert sorted(out) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(out[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("name", ("G18a", "G18b"))
def test_host_half_of_get_iou_and_evaluate_is_exact(name, capsys):
    from omnifusion_amd import iou
    g = golden(name + "_semantic")
    conf = g["confusion"]
    for i in range(13):
        v = iou.get_iou(i, conf)
        assert v == (float(g["iou"][i]), int(g["tp"][i]), int(g["denom"][i])), (name, i)
    flog = io.StringIO()
    mean = iou.evaluate_confusion(conf, int(g["pred"].size), flog)
    assert mean == float(g["mean_iou"])                                        # the same float, not a close one
    text = capsys.readouterr().out
    assert text == str(g["evaluate_text"])
    assert flog.getvalue() == "".join(line + "\n" for line in text.splitlines()[3:16])
    assert iou.evaluate_confusion(torch.from_numpy(conf), int(g["pred"].size)) == mean          # a tensor is copied to the host first


def test_absent_class_gives_nan_not_type_error(capsys):
    from omnifusion_amd import iou
    conf = np.zeros((13, 13), np.int64)
    conf[0, 0], conf[1, 0] = 3, 1
    assert iou.get_iou(0, conf) == (0.75, 3, 4)
    v = iou.get_iou(5, conf)
    assert np.isnan(v[0]) and v[1:] == (0, 0)
    assert np.isnan(iou.evaluate_confusion(conf, 4))
    assert "clutter       :   nan   (     0/0     )" in capsys.readouterr().out
    m = iou.SegmentationMetrics()
    m.confusion = torch.from_numpy(conf)
    assert np.isnan(m.mean_iou()) and m.mean_iou(skip_absent=True) == (0.75 + 0.0) / 2
    with pytest.raises(ValueError, match="13 x 13"):
        iou.evaluate_confusion(np.zeros((2, 2), np.int64), 4)
