"""G15a-e: the gradients of the reference's own render (supervision/splatting.py:73-80) and DIBR (util.py:384-413) by its autograd on
the CPU, for the G14a-e inputs and the upstream gradient of tests/_vs_cases.py.  Stored per input tensor: the float64 run's gradient
(rounded to float32 for storage; NaN where the reference returns NaN), and the deviation of the reference's own float32 run from it in
the parity gate's measure (share of elements over 1e-4, worst element).  Needs the reference checkout; writes arrays only.

    python tools/gen_golden_dibr_bwd.py
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
    c = vc.dibr_case(name)
    g64 = vc.reference_dibr_grads(c, torch.float64)
    g32 = vc.reference_dibr_grads(c, torch.float32)
    out = {}
    for k in vc.dibr_grad_names(c):
        e = vc.rel_error(g32[k], g64[k])
        out["grad_" + k] = g64[k].astype(np.float32)
        out["ref32_share_" + k] = np.float64((e > 1e-4).mean())
        out["ref32_max_" + k] = np.float64(e.max())
        out["nonfinite_" + k] = np.int64((~np.isfinite(g64[k])).sum())
    out.update({"sum_" + k: v for k, v in vc.checksums(c).items()})
    return c, out


def main():
    for name in __import__("_vs_cases").DIBR_NAMES:
        c, out = build(name)
        path = os.path.join(ROOT, "tests", "golden", name + "_dibr_bwd.npz")
        np.savez_compressed(path, **out)
        stats = {k: (float(out["ref32_share_" + k]), float(out["ref32_max_" + k]), int(out["nonfinite_" + k]))
                 for k in ("img", "depth", "coords") if "grad_" + k in out}
        print(name, c["kind"], c["img"].shape, "ref fp32 vs fp64 (share > 1e-4, max, non-finite):", stats, f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
