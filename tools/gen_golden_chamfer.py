"""G21a-e: the reference's own chamfer_distance_with_batch (util.py:201-257) and its gradients w.r.t. both clouds by autograd on the CPU in
float64, for the seeded inputs of tests/_chamfer_cases.py; with masks (G21e) the reference is called item by item on the valid points.  The
per-point distances and argmins come from the same formula (the restatement of the test module, asserted here to reproduce the reference's
loss and gradients to round-off).  Stored per case: loss, dist, idx, grad_p1, grad_p2, and the errors of the reference's own FLOAT32 run
against that float64 run — ref32_loss_err, ref32_dist_err, ref32_grad_max (the GPU gates are multiples of them).  The generator also asserts
what the exact index comparison rests on: in float64 every valid query's nearest and second-nearest valid targets are at least 1e-5 apart
(the planted exact duplicates of G21e have distance 0 to distinct originals), and no index flips in the float32 run.  G21a also stores the
residual of the directional-derivative check on the reference's float32 and float64 runs.
Needs the reference checkout; writes arrays only.

    python tools/gen_golden_chamfer.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(name):
    import torch
    import _chamfer_cases as cc
    c = cc.case(name)
    r64, r32 = cc.run_reference(c, torch.float64), cc.run_reference(c, torch.float32)
    s64, s32 = cc.run_restatement(c, torch.float64), cc.run_restatement(c, torch.float32)
    assert np.isfinite(r64["loss"]) and abs(s64["loss"] - r64["loss"]) <= 1e-12 * max(1.0, abs(r64["loss"])), f"{name}: the restatement's loss is not the reference's"
    for k in ("grad_p1", "grad_p2"):
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all()
        assert np.abs(s64[k] - r64[k]).max() <= 1e-12, f"{name}: the restatement's {k} is not the reference's"
    gap = cc.gaps(c)
    assert gap >= cc.MIN_GAP, f"{name}: a query's two nearest targets are {gap:.2e} apart: pick another seed"
    assert np.array_equal(s32["idx"], s64["idx"]), f"{name}: an index flips in float32: pick another seed"
    for b, i, j in c["dup"]:
        assert s64["idx"][b, i] == j and s64["dist"][b, i] == 0.0 and not s64["grad_p1"][b, i].any()
    out = dict(loss=np.float64(r64["loss"]), dist=s64["dist"], idx=s64["idx"], grad_p1=r64["grad_p1"], grad_p2=r64["grad_p2"], min_gap=np.float64(gap))
    out["ref32_loss_err"] = np.float64(abs(r32["loss"] - r64["loss"]))
    out["ref32_dist_err"] = np.float64(np.abs(s32["dist"] - s64["dist"]).max())
    out["ref32_grad_max"] = np.float64(max(cc.rel_error(r32[k], r64[k]).max() if np.abs(r64[k]).max() > 0 else 0.0 for k in ("grad_p1", "grad_p2")))
    if name == "G21a":
        v1, v2 = cc.direction(name)
        n1 = c["p1"].size
        x, v = np.concatenate([c["p1"].ravel(), c["p2"].ravel()]), np.concatenate([v1.ravel(), v2.ravel()])
        for tag, dtype, r in (("ref32", torch.float32, r32), ("ref64", torch.float64, r64)):
            loss_of = lambda y: cc.run_reference(c, dtype, p1=y[:n1].reshape(c["p1"].shape), p2=y[n1:].reshape(c["p2"].shape))["loss"]
            grad = np.concatenate([r["grad_p1"].ravel(), r["grad_p2"].ravel()]).astype(np.float64)
            res, fd, dot = cc.directional_residual(loss_of, grad, x, v, cc.DIRECTION_H)
            assert np.isfinite(res)
            out[tag + "_direction_residual"] = np.float64(res)
    out.update({"sum_" + k: v for k, v in cc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_chamfer_cases").NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_chamfer.npz")
        np.savez_compressed(path, **out)
        print(name, c["p1"].shape, c["p2"].shape, f"loss {float(out['loss']):.8f} min gap {float(out['min_gap']):.1e} ref32 err: loss {float(out['ref32_loss_err']):.1e} "
              f"dist {float(out['ref32_dist_err']):.1e} grad max rel {float(out['ref32_grad_max']):.1e} "
              + (f"direction residual f32 {float(out['ref32_direction_residual']):.2e} f64 {float(out['ref64_direction_residual']):.2e} " if "ref32_direction_residual" in out else "")
              + f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
