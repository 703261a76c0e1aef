"""G16a-c: the reference's own photometric loss (supervision/photometric.py:34-51, supervision/ssim.py) and its gradient w.r.t. the
prediction by autograd on the CPU in float64, for the seeded inputs of tests/_vs_cases.py.  The generator also checks what the GPU
parity gate relies on: the reference's own float32 gradient is within 1e-4 of the float64 one at EVERY element (relative to the largest
gradient), and (1 - ssim) / 2 stays strictly inside (0, 1) — the clamp, the only step of this loss besides |.|, is never reached.
Needs the reference checkout; writes arrays only.

    python tools/gen_golden_photometric.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(name):
    import torch
    import _vs_cases as vc
    c = vc.photo_case(name)
    res = {}
    for dtype in (torch.float64, torch.float32):
        loss, p, hmin, hmax = vc.reference_photo(c, dtype)
        loss.backward()
        res[dtype] = (float(loss.detach()), p.grad.numpy(), hmin, hmax)
    l64, g64, hmin, hmax = res[torch.float64]
    l32, g32 = res[torch.float32][:2]
    e = vc.rel_error(g32, g64)
    assert np.isfinite(g64).all()
    assert 1e-5 < hmin and hmax < 1.0 - 1e-5, f"{name}: the clamp is reached ({hmin}, {hmax}): pick other seeds"
    assert e.max() <= 1e-4, f"{name}: the reference's own float32 gradient is off by {e.max():.2e}: pick other seeds"
    out = dict(loss=np.float64(l64), grad=g64.astype(np.float32), ref32_loss_err=np.float64(abs(l32 - l64)), ref32_grad_max=np.float64(e.max()),
               dssim_min=np.float64(hmin), dssim_max=np.float64(hmax))
    out.update({"sum_" + k: v for k, v in vc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_vs_cases").PHOTO_NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_photometric.npz")
        np.savez_compressed(path, **out)
        print(name, c["mode"], c["window"], c["mask"].shape, f"loss {float(out['loss']):.8f} ref32 loss err {float(out['ref32_loss_err']):.1e} "
              f"ref32 grad max rel {float(out['ref32_grad_max']):.1e} d_ssim in [{float(out['dssim_min']):.3f}, {float(out['dssim_max']):.3f}] "
              f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
