"""G22a-g: the reference's own plane-fit normals (equi_pers/depth2normal.py), the normal loss of train_erp_depth.py:271 over them, and their
gradients by autograd on the CPU in float64, for the seeded inputs of tests/_planefit_cases.py.  Stored per case: the normals of pred, the
loss, d loss / d pred, the gradient of sum(normals * U) for the seeded upstream U, and the error of the reference's own FLOAT32 run against
that float64 run for each of them (the GPU gates are max(floor, 4 x that error)); G22g (the forward map alone) stores the float64 determinants
too.  The generator also asserts what the gates rest on: every value is finite, the float64 restatement of the test module reproduces the
reference to 1e-12, no determinant of G22f lies within 10 % of the threshold 1e-5 (no branch can flip there), at most 1 % of G22g's
determinants lie within 1 % of it and the reference's float32 run takes the float64 run's branch at every pixel outside that band.  G22a also
stores the residual of the directional-derivative check on the reference's float32 and float64 runs.
Needs the reference checkout; writes arrays only.

    python tools/gen_golden_planefit.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(name):
    import torch
    import _planefit_cases as pc
    c = pc.case(name)
    r64, r32 = pc.run_reference(c, torch.float64, name), pc.run_reference(c, torch.float32, name)
    rest = pc.run_restatement(c, torch.float64, name=name)
    arrays = [k for k in ("normals", "grad_map", "grad_loss") if k in r64]
    for k in arrays + [k for k in ("det", "det_gt") if k in r64]:
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), f"{name}: non-finite {k}: pick other seeds"
        assert np.abs(rest[k] - r64[k]).max() <= 1e-12 * max(1.0, np.abs(r64[k]).max()), f"{name}: the restatement's {k} is not the reference's"
    out = {k: r64[k].astype(np.float32) for k in arrays}
    out["ref32_normals_err"] = np.float64(np.abs(r32["normals"].astype(np.float64) - r64["normals"]).max())
    for k in arrays[1:]:
        out["ref32_" + k + "_max"] = np.float64(pc.rel_error(r32[k], r64[k]).max())
    if "loss" in r64:
        assert np.isfinite(r64["loss"]) and abs(rest["loss"] - r64["loss"]) <= 1e-12
        out["loss"] = np.float64(r64["loss"])
        out["ref32_loss_err"] = np.float64(abs(r32["loss"] - r64["loss"]))
    dets = np.stack([r64[k] for k in ("det", "det_gt") if k in r64])
    out["fallback_pixels"] = np.int64((dets < pc.DET_MIN).sum())
    if name == "G22f":
        assert 0 < out["fallback_pixels"] < dets.size and not pc.band(dets, pc.F_BAND).any(), f"{name}: a determinant within 10 % of 1e-5, or one branch only"
    if name == "G22g":
        near = pc.band(r64["det"], pc.G_BAND)
        assert 0 < near.sum() <= 0.01 * near.size, f"{name}: {int(near.sum())} of {near.size} determinants within 1 % of 1e-5"
        flips = ((r32["det"] >= pc.DET_MIN) != (r64["det"] >= pc.DET_MIN)) & ~near
        assert not flips.any(), f"{name}: the reference's float32 run flips {int(flips.sum())} branches outside the band"
        assert min((r64["det"] >= pc.DET_MIN).mean(), (r64["det"] < pc.DET_MIN).mean()) > 0.25, f"{name}: the determinants do not straddle 1e-5"
        out["det"] = r64["det"].astype(np.float64)
        out["band_pixels"] = np.int64(near.sum())
    if name == "G22a":
        for tag, dtype, r in (("ref32", torch.float32, r32), ("ref64", torch.float64, r64)):
            res, fd, dot = pc.directional_residual(lambda p: pc.run_reference(dict(c, pred=p), dtype)["loss"], r["grad_loss"].astype(np.float64), c["pred"],
                                                   pc.direction(name), pc.DIRECTION_H)
            assert np.isfinite(res)
            out[tag + "_direction_residual"] = np.float64(res)
    out.update({"sum_" + k: v for k, v in pc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_planefit_cases").NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_planefit.npz")
        np.savez_compressed(path, **out)
        f = lambda k: f"{float(out[k]):.1e}" if k in out else "-"
        print(name, c["pred"].shape, f"loss {f('loss')} fallback {int(out['fallback_pixels'])} ref32 err: normals {f('ref32_normals_err')} loss {f('ref32_loss_err')} "
              f"grad_map {f('ref32_grad_map_max')} grad_loss {f('ref32_grad_loss_max')} direction residual f32 {f('ref32_direction_residual')} "
              f"f64 {f('ref64_direction_residual')} band {int(out['band_pixels']) if 'band_pixels' in out else '-'} {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
