"""G20a-e: the reference's own guided smoothness term — coords_3d, dV_dxyz, dI_duv and guided_smoothness_loss combined as
supervision.smoothness.depth_smoothness combines them — and its gradient w.r.t. the depth by autograd on the CPU in float64, for the seeded
inputs of tests/_smoothness_cases.py.  Stored per case: the loss, the dV_dxyz and dI_duv maps, d loss / d depth, and the error of the
reference's own FLOAT32 run against that float64 run (the GPU gates are max(1e-5, 4 x that error)).  The generator also asserts what the
gates rest on: every value is finite, no interior vertex difference that matters is within 1e-4 of 0 (the kink of |.| is reached only where
replicate padding puts it), and the float64 restatement of the test module reproduces the reference to round-off.  G20a also stores the
residual of the directional-derivative check on the reference's float32 and float64 runs.
Needs the reference checkout; writes arrays only.

    python tools/gen_golden_smoothness.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(name):
    import torch
    import _smoothness_cases as sc
    c = sc.case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r64, r32 = sc.run_reference(c, torch.float64), sc.run_reference(c, torch.float32)
    rest = sc.run_restatement(c, torch.float64)
    for k in ("dV_dxyz", "dI_duv", "grad"):
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), f"{name}: non-finite {k}: pick other seeds"
        assert np.abs(rest[k] - r64[k]).max() <= 1e-12 * max(1.0, np.abs(r64[k]).max()), f"{name}: the restatement's {k} is not the reference's"
    assert np.isfinite(r64["loss"]) and abs(rest["loss"] - r64["loss"]) <= 1e-12
    out = dict(loss=np.float64(r64["loss"]), dV_dxyz=r64["dV_dxyz"].astype(np.float32), dI_duv=r64["dI_duv"].astype(np.float32), grad=r64["grad"].astype(np.float32))
    out["ref32_loss_err"] = np.float64(abs(r32["loss"] - r64["loss"]))
    for k in ("dV_dxyz", "dI_duv"):
        out["ref32_" + k + "_err"] = np.float64(np.abs(r32[k].astype(np.float64) - r64[k]).max())
    out["ref32_grad_max"] = np.float64(sc.rel_error(r32["grad"], r64["grad"]).max())
    margin = sc.kink_margin(c)
    assert margin > sc.KINK_MARGIN, f"{name}: an interior vertex difference is {margin:.2e}: the kink of |.| is too close, pick other seeds"
    out["kink_margin"] = np.float64(margin)
    if name == "G20a":
        for tag, dtype, r in (("ref32", torch.float32, r32), ("ref64", torch.float64, r64)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res, fd, dot = sc.directional_residual(lambda p: sc.run_reference(dict(c, depth=p), dtype)["loss"], r["grad"].astype(np.float64), c["depth"],
                                                       sc.direction(name), sc.DIRECTION_H)
            assert np.isfinite(res)
            out[tag + "_direction_residual"] = np.float64(res)
    out.update({"sum_" + k: v for k, v in sc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_smoothness_cases").NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_smoothness.npz")
        np.savez_compressed(path, **out)
        print(name, c["depth"].shape, f"weights {c['weights'] is not None} loss {float(out['loss']):.8f} ref32 err: loss {float(out['ref32_loss_err']):.1e} "
              f"dV_dxyz {float(out['ref32_dV_dxyz_err']):.1e} dI_duv {float(out['ref32_dI_duv_err']):.1e} grad max rel {float(out['ref32_grad_max']):.1e} "
              f"kink margin {float(out['kink_margin']):.1e} "
              + (f"direction residual f32 {float(out['ref32_direction_residual']):.2e} f64 {float(out['ref64_direction_residual']):.2e} " if "ref32_direction_residual" in out else "")
              + f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
