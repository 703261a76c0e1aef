"""CPU: the autograd-capable restatement of tests/_freeview_bwd_cases.py is pinned against _freeview_cases' float64 forward (bit for
bit) and against the reference's own float64 autograd (goldens G17a-d, tools/gen_golden_freeview_bwd.py).  The GPU tests then use it
where no golden exists: views_to_erp and the non-finite sets."""
import numpy as np
import pytest
import torch

import _freeview_bwd_cases as bc
import _freeview_cases as fc

REL = 1e-6               # of the largest gradient of the tensor (the goldens are float64 results rounded to float32: 6e-8)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


@pytest.mark.parametrize("name", bc.NAMES)
def test_restatement_forward_equals_the_forward_restatement(name):
    c = bc.case(name)
    args = (c["hfov"], c["wfov"], c["theta"], c["phi"])
    assert torch.equal(bc.equi2pers(_t(c["erp"]), *args, c["h"], c["w"]), fc.equi2pers(c["erp"], *args, c["h"], c["w"]))
    want, wmask = fc.pers2equi(c["pers"], *args, c["H"], c["W"])
    for select in (False, True):
        got, mask = bc.pers2equi(_t(c["pers"]), *args, c["H"], c["W"], select=select)
        assert torch.equal(got, want) and torch.equal(mask, wmask)
    views = _t(c["pers"])[None]
    merged, count = bc.views_to_erp(views, *args, c["H"], c["W"])
    wm, wc = fc.merge(want, wmask)
    assert torch.equal(merged[0], wm) and torch.equal(count, wc)


@pytest.mark.parametrize("name", bc.NAMES)
def test_restatement_gradients_equal_the_reference_autograd(name):
    c, g = bc.case(name), bc.load(name)
    g_e2p, g_p2e = bc.upstream(name)
    args = (c["hfov"], c["wfov"], c["theta"], c["phi"])
    erp = _t(c["erp"]).requires_grad_(True)
    (bc.equi2pers(erp, *args, c["h"], c["w"]) * _t(g_e2p)).sum().backward()
    top = np.abs(g["grad_erp"]).max()
    assert np.abs(erp.grad.numpy() - g["grad_erp"]).max() <= REL * top
    for select in (False, True):
        pers = _t(c["pers"]).requires_grad_(True)
        (bc.pers2equi(pers, *args, c["H"], c["W"], select=select)[0] * _t(g_p2e)).sum().backward()
        top = np.abs(g["grad_pers"]).max()
        assert np.abs(pers.grad.numpy() - g["grad_pers"]).max() <= REL * top
    # the reference's own float32 autograd stays inside the gate everywhere: the device is allowed no outlier either
    assert int(g["ref32_erp_outliers"]) == 0 and int(g["ref32_pers_outliers"]) == 0
    assert float(g["ref32_erp_rel"]) < bc.GATE and float(g["ref32_pers_rel"]) < bc.GATE


def test_mask_divergence_of_the_restatement():
    """DESIGN §7 d11 on the CPU: an inf upstream value OUTSIDE the mask reaches pixel (0, 0) of the view as NaN through the reference's
    `sample * mask`, and reaches nothing through `where(mask, sample, 0)`."""
    c = bc.case("G17a")
    args = (c["hfov"], c["wfov"], c["theta"], c["phi"])
    _, g_p2e = bc.upstream("G17a")
    _, mask = bc.p2e_grid(*args, c["h"], c["w"], c["H"], c["W"])
    r, s = (int(v[0]) for v in np.nonzero(mask[0, 0].numpy() == 0))
    g_p2e[0, 1, r, s] = np.inf
    for select, finite in ((False, False), (True, True)):
        pers = _t(c["pers"]).requires_grad_(True)
        (bc.pers2equi(pers, *args, c["H"], c["W"], select=select)[0] * _t(g_p2e)).sum().backward()
        bad = ~torch.isfinite(pers.grad)
        assert bool(bad.any()) != finite
        if not finite:
            where = bad.nonzero().tolist()                                   # the dummy coordinate's corners: pixel (0, 0) and its zero-weight neighbours
            assert [0, 1, 0, 0] in where and all(v == 0 and p == 1 and i <= 1 and j <= 1 for v, p, i, j in where)
