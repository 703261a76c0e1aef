"""G19a-e: the reference's own geometry terms — depth2normal_gpu, imgrad_yx and calculate_l1_loss combined as train_erp_depth.py:271-274
spells them — and their gradients w.r.t. the prediction by autograd on the CPU in float64, for the seeded inputs of tests/_geometry_cases.py.
G19e runs the same formula on the eroded mask (erode_mask=True of supervision.geometry).  The generator also asserts what the GPU gates rest
on: the reference's own float32 gradients are within 1e-4 of the float64 ones at EVERY element (relative to the largest gradient), its float32
losses within a quarter of the loss gate, and no masked |gt' - pred'| of the Sobel maps is below 1e-6 (the kink of |.| is never reached).
Needs the reference checkout; writes arrays only.

    python tools/gen_golden_geometry.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOSS_GATE = 2e-6                                       # x max(1, |loss|): the gate of tests/test_geometry_gpu.py


def build(name):
    import torch
    import _geometry_cases as gc
    c = gc.case(name)
    r64, r32 = gc.run_reference(c, torch.float64), gc.run_reference(c, torch.float32)
    out = dict(normal_loss=np.float64(r64["normal_loss"]), grad_loss=np.float64(r64["grad_loss"]), normals=r64["normals"].astype(np.float32),
               grad_normal=r64["grad_normal"].astype(np.float32), grad_grad=r64["grad_grad"].astype(np.float32))
    for k in ("normals", "grad_normal", "grad_grad"):
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), f"{name}: non-finite {k}: pick other seeds"
    for k in ("normal_loss", "grad_loss"):
        err = abs(r32[k] - r64[k])
        assert np.isfinite(r64[k]) and err <= 0.25 * LOSS_GATE * max(1.0, abs(r64[k])), f"{name}: the reference's own float32 {k} is off by {err:.2e}: pick other seeds"
        out["ref32_" + k + "_err"] = np.float64(err)
    out["ref32_normals_err"] = np.float64(np.abs(r32["normals"].astype(np.float64) - r64["normals"]).max())
    for k in ("grad_normal", "grad_grad"):
        e = gc.rel_error(r32[k], r64[k]).max()
        assert e <= 1e-4, f"{name}: the reference's own float32 {k} is off by {e:.2e} of the largest gradient: pick other seeds"
        out["ref32_" + k + "_max"] = np.float64(e)
    min_d = gc.run_restatement(c, torch.float64)["min_dsobel"]
    assert min_d > 1e-6, f"{name}: a masked |gt' - pred'| is {min_d:.2e}: the kink of |.| is reached, pick other seeds"
    out["min_dsobel"] = np.float64(min_d)
    if name == "G19a":
        res, fd, dot = gc.directional_residual(lambda p: gc.reference_loss32(c, p), r32["grad_normal"].astype(np.float64) + r32["grad_grad"], c["pred"],
                                               gc.direction(name), gc.DIRECTION_H)
        assert np.isfinite(res)
        out["ref32_direction_residual"] = np.float64(res)
    out.update({"sum_" + k: v for k, v in gc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_geometry_cases").NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_geometry.npz")
        np.savez_compressed(path, **out)
        print(name, c["pred"].shape, f"erode {c['erode']} normal_loss {float(out['normal_loss']):.8f} grad_loss {float(out['grad_loss']):.8f} ref32 loss err "
              f"{float(out['ref32_normal_loss_err']):.1e} / {float(out['ref32_grad_loss_err']):.1e} normals {float(out['ref32_normals_err']):.1e} grad max rel "
              f"{float(out['ref32_grad_normal_max']):.1e} / {float(out['ref32_grad_grad_max']):.1e} min |dsobel| {float(out['min_dsobel']):.1e} "
              + (f"direction residual {float(out['ref32_direction_residual']):.2e} " if "ref32_direction_residual" in out else "")
              + f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
