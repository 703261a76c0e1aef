"""G16a-d free-view goldens: the reference's own equi2pers (equi_pers/equi2pers_torch.py:37) and pers2equi (equi_pers/pers2equi_torch.py:37)
on the CPU for the cases of tests/_freeview_cases.py.  Stored per case: the inputs, the float64 run's results rounded to float32, the
float64 run's mask, and the deviation of the reference's own float32 run from it (max |d| of both directions where the masks agree, and
the number of mask elements that differ).  Needs the reference checkout; writes arrays only.

    python tools/gen_golden_freeview.py

The reference hard-codes torch.float32 for its axis vectors, so its float64 run is made by handing its two modules a `torch` whose
float32 IS float64 and a float64 default dtype (nothing of the reference is edited or copied).  For cases a, b and d the float32 run's
mask must stay within FLIP_CAP of the float64 one (asserted): angles that sit on a frustum edge would be moved by a fraction of a degree
and recorded in the case table (none had to be).
"""
import contextlib
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_modules():
    from oracle import ref_loader
    ref_loader._install_stubs()
    for name in ("matplotlib", "matplotlib.pyplot"):                  # imported at module level, used under __main__ only
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if "matplotlib" in sys.modules and "matplotlib.pyplot" in sys.modules:
        setattr(sys.modules["matplotlib"], "pyplot", sys.modules["matplotlib.pyplot"])
    if ref_loader.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    return importlib.import_module("equi_pers.equi2pers_torch"), importlib.import_module("equi_pers.pers2equi_torch")


class _Torch64:
    """`torch` as the reference's modules see it during the float64 run."""

    def __init__(self, torch):
        self._torch = torch
        self.float32 = torch.float64

    def __getattr__(self, name):
        return getattr(self._torch, name)


@contextlib.contextmanager
def precision(mods, dtype):
    import torch
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    for m in mods:
        m.torch = _Torch64(torch) if dtype == torch.float64 else torch
    try:
        yield
    finally:
        torch.set_default_dtype(old)
        for m in mods:
            m.torch = torch


def run_reference(mods, c, dtype):
    import torch
    e2p, p2e = mods
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    with precision(mods, dtype), torch.no_grad():
        pers = e2p.equi2pers(t(c["erp"]), c["hfov"], c["wfov"], t(c["theta"]), t(c["phi"]), c["h"], c["w"])
        erp, mask = p2e.pers2equi(t(c["pers"]), c["hfov"], c["wfov"], t(c["theta"]), t(c["phi"]), c["H"], c["W"])
    assert pers.dtype == dtype and erp.dtype == dtype, (pers.dtype, erp.dtype)
    return pers.numpy(), erp.numpy(), mask.numpy()


def build(mods, name):
    import torch
    import _freeview_cases as fc
    c = fc.case(name)
    pers64, erp64, mask64 = run_reference(mods, c, torch.float64)
    pers32, erp32, mask32 = run_reference(mods, c, torch.float32)
    assert np.isfinite(pers64).all() and np.isfinite(erp64).all()
    flips = int((mask32 != mask64).sum())
    agree = np.broadcast_to(mask32 == mask64, erp64.shape)
    stray = int(((mask32 != mask64) & ~fc.flip_allowed(c["theta"], c["phi"], c["hfov"], c["wfov"], c["H"], c["W"])).sum())
    out = dict(erp=c["erp"], pers=c["pers"], theta=c["theta"], phi=c["phi"], hfov=np.float64(c["hfov"]), wfov=np.float64(c["wfov"]),
               e2p=pers64.astype(np.float32), p2e=erp64.astype(np.float32), mask=mask64.astype(np.uint8),
               mask_dtype=np.array(str(mask64.dtype)), mask_shape=np.array(mask64.shape, np.int64),
               ref32_e2p_max=np.float64(np.abs(pers32 - pers64).max()), ref32_p2e_max=np.float64(np.abs(erp32 - erp64)[agree].max()),
               ref32_mask_flips=np.int64(flips), ref32_mask_flips_stray=np.int64(stray))
    if name != "G16c":
        assert flips <= fc.FLIP_CAP * mask64.size, f"{name}: the reference's own float32 mask differs from its float64 mask in {flips} of {mask64.size} elements"
    return out


def main():
    import _freeview_cases as fc
    mods = reference_modules()
    for name in fc.NAMES:
        out = build(mods, name)
        path = os.path.join(ROOT, "tests", "golden", name + "_freeview.npz")
        np.savez_compressed(path, **out)
        print(name, "e2p", out["e2p"].shape, "p2e", out["p2e"].shape, "mask", str(out["mask_dtype"]), tuple(int(v) for v in out["mask_shape"]), "covered", int(out["mask"].sum()),
              "| ref fp32 vs fp64: e2p max %.2e, p2e max %.2e, mask flips %d (outside the allowed band: %d)" %
              (out["ref32_e2p_max"], out["ref32_p2e_max"], out["ref32_mask_flips"], out["ref32_mask_flips_stray"]), f"| {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
