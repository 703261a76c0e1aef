"""G17a-d free-view backward goldens: the reference's own autograd through its equi2pers (equi_pers/equi2pers_torch.py:37) and pers2equi
(equi_pers/pers2equi_torch.py:37) on the CPU for the cases of tests/_freeview_cases.py, with the seeded upstream gradients of
tests/_freeview_bwd_cases.upstream: loss = (out * G).sum().  Stored per case: the float64 run's gradients rounded to float32
(d/d equi_img, d/d pers_img) and the deviation of the reference's own float32 autograd from them — max |d| relative to the largest
float64 gradient of the tensor, and the number of elements over the gate (1e-4 of that largest gradient): the outlier count the device
is allowed.  Needs the reference checkout; writes arrays only.

    python tools/gen_golden_freeview_bwd.py

The float64 run is made as in tools/gen_golden_freeview.py (its `precision` and `reference_modules`): nothing of the reference is
edited or copied.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run_reference(mods, c, g_e2p, g_p2e, dtype):
    import torch
    from gen_golden_freeview import precision
    e2p, p2e = mods
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    with precision(mods, dtype):
        erp, pers = t(c["erp"]).requires_grad_(True), t(c["pers"]).requires_grad_(True)
        out = e2p.equi2pers(erp, c["hfov"], c["wfov"], t(c["theta"]), t(c["phi"]), c["h"], c["w"])
        (out * t(g_e2p)).sum().backward()
        out, _ = p2e.pers2equi(pers, c["hfov"], c["wfov"], t(c["theta"]), t(c["phi"]), c["H"], c["W"])
        (out * t(g_p2e)).sum().backward()
    assert erp.grad.dtype == dtype and pers.grad.dtype == dtype
    return erp.grad.numpy(), pers.grad.numpy()


def build(mods, name):
    import torch
    import _freeview_bwd_cases as bc
    c = bc.case(name)
    g_e2p, g_p2e = bc.upstream(name)
    erp64, pers64 = run_reference(mods, c, g_e2p, g_p2e, torch.float64)
    erp32, pers32 = run_reference(mods, c, g_e2p, g_p2e, torch.float32)
    assert np.isfinite(erp64).all() and np.isfinite(pers64).all()
    out = dict(grad_erp=erp64.astype(np.float32), grad_pers=pers64.astype(np.float32))
    for key, a64, a32 in (("erp", erp64, erp32), ("pers", pers64, pers32)):
        top = np.abs(a64).max()
        d = np.abs(a32.astype(np.float64) - a64)
        out[f"ref32_{key}_rel"] = np.float64(d.max() / top)
        out[f"ref32_{key}_outliers"] = np.int64((d > bc.GATE * top).sum())
    return out


def main():
    import _freeview_bwd_cases as bc
    from gen_golden_freeview import reference_modules
    mods = reference_modules()
    for name in bc.NAMES:
        out = build(mods, name)
        path = os.path.join(ROOT, "tests", "golden", name + "_freeview_bwd.npz")
        np.savez_compressed(path, **out)
        print(name, "grad_erp", out["grad_erp"].shape, "grad_pers", out["grad_pers"].shape,
              "| ref fp32 vs fp64 autograd: erp rel %.2e (%d over the gate), pers rel %.2e (%d over the gate)" %
              (out["ref32_erp_rel"], out["ref32_erp_outliers"], out["ref32_pers_rel"], out["ref32_pers_outliers"]),
              f"| {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
