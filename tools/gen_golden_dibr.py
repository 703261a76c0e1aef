"""G14a-e: the reference's own DIBR (util.py:384-413) and forward splat (supervision/splatting.py:73-80) on the CPU, for the seeded
inputs of tests/_dibr_cases.py.  Needs the reference checkout (oracle/ref_loader.py); writes outputs and float64 input checksums only.

    python tools/gen_golden_dibr.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _dibr_cases as dc
    for name in dc.NAMES:
        c = dc.case(name)
        recon, mask = dc.run_reference(c)
        out = dict(recon=recon.astype(np.float32))
        if mask is not None:
            out["mask"] = mask.astype(np.uint8)
        out.update({"sum_" + k: v for k, v in dc.checksums(c).items()})
        path = os.path.join(ROOT, "tests", "golden", name + "_dibr.npz")
        np.savez_compressed(path, **out)
        print(name, c["kind"], c["img"].shape, "finite", bool(np.isfinite(recon).all()), f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
