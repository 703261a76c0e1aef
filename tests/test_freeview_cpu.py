"""Free-view sampling without a GPU: the goldens G16a-d against the torch restatement of tests/_freeview_cases.py, the host side of the C
ABI (rotation tables, argument validation) and the refusal of the Python mirrors to run anywhere but on the device."""
import ctypes

import numpy as np
import pytest
import torch

import _freeview_cases as fc
from omnifusion_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", fc.NAMES)
def test_restatement_agrees_with_goldens(name):
    """The float64 restatement reproduces what the reference itself computed in float64 (stored rounded to float32: 6e-8), masks exactly;
    its float32 run stays within a few times the reference's own float32 deviation."""
    c, g = fc.case(name), fc.load(name)
    for k in ("erp", "pers", "theta", "phi"):
        assert np.array_equal(c[k], g[k]), f"{name}: seeded input {k} differs from the stored one"
    assert str(g["mask_dtype"]) == "int64" and tuple(g["mask_shape"]) == (len(c["theta"]), 1, c["H"], c["W"])
    e2p = fc.equi2pers(c["erp"], c["hfov"], c["wfov"], c["theta"], c["phi"], c["h"], c["w"]).numpy()
    erp, mask = fc.pers2equi(c["pers"], c["hfov"], c["wfov"], c["theta"], c["phi"], c["H"], c["W"])
    assert e2p.shape == g["e2p"].shape and erp.shape == g["p2e"].shape
    assert np.abs(e2p - g["e2p"]).max() <= 1e-6
    assert np.array_equal(mask.numpy(), g["mask"])
    assert np.abs(erp.numpy() - g["p2e"]).max() <= 1e-6
    e32 = fc.equi2pers(c["erp"], c["hfov"], c["wfov"], c["theta"], c["phi"], c["h"], c["w"], torch.float32).numpy()
    assert np.abs(e32 - g["e2p"]).max() <= 1e-4
    assert float(g["ref32_e2p_max"]) <= 1e-4 and float(g["ref32_p2e_max"]) <= 1e-4
    if name != "G16c":
        assert int(g["ref32_mask_flips"]) <= fc.FLIP_CAP * g["mask"].size
    assert int(g["ref32_mask_flips_stray"]) == 0


def _rotations(lib, theta, phi):
    theta, phi = np.ascontiguousarray(theta, np.float32), np.ascontiguousarray(phi, np.float32)
    n = len(theta)
    fwd, inv = np.zeros((n, 3, 3), np.float32), np.zeros((n, 2, 3, 3), np.float32)
    assert lib.omni_freeview_rotations(theta.ctypes.data, phi.ctypes.data, n, fwd.ctypes.data, inv.ctypes.data) == _lib.OMNI_OK
    return fwd, inv


@pytest.mark.parametrize("name", fc.NAMES)
def test_rotation_tables(lib, name):
    """omni_freeview_rotations against the reference's matrices (its quaternion form in float64, restated) to 1e-6, and R_inv . R_fwd = I."""
    c = fc.case(name)
    fwd, inv = _rotations(lib, c["theta"], c["phi"])
    R1, R2 = fc.view_rotations(c["theta"], c["phi"], torch.float64)
    assert np.abs(fwd - torch.matmul(R2, R1).numpy()).max() <= 1e-6
    assert np.abs(inv[:, 0] - torch.inverse(R2).numpy()).max() <= 1e-6
    assert np.abs(inv[:, 1] - torch.inverse(R1).numpy()).max() <= 1e-6
    prod = np.einsum("vij,vjk,vkl->vil", inv[:, 1].astype(np.float64), inv[:, 0].astype(np.float64), fwd.astype(np.float64))
    assert np.abs(prod - np.eye(3)).max() <= 1e-6


def test_cubemap_views_are_the_six_faces(lib):
    from omnifusion_amd.equi_pers import cubemap_views
    theta, phi = cubemap_views()
    assert tuple(theta.tolist()) == fc.CUBE_THETA and tuple(phi.tolist()) == fc.CUBE_PHI
    fwd, _ = _rotations(lib, theta.numpy(), phi.numpy())
    axes = fwd[:, :, 0]                                              # where each view's optical axis (1, 0, 0) points
    want = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    assert np.abs(axes - want).max() <= 1e-6


def test_argument_validation_needs_no_device(lib):
    """Bad arguments are refused before anything is launched: the pointers below are never dereferenced."""
    p = ctypes.c_void_p(4096)
    e2p = lambda B=1, C=1, H=8, W=16, N=1, h=4, w=4, hf=90.0, wf=90.0, layout=_lib.LAYOUT_BNCHW, erp=p, pers=p, rot=p: \
        lib.omni_freeview_equi2pers_f32(erp, pers, rot, B, C, H, W, N, h, w, hf, wf, layout, None)
    p2e = lambda N=1, C=1, h=4, w=4, H=8, W=16, hf=90.0, wf=90.0, mask=p: lib.omni_freeview_pers2equi_f32(p, p, mask, p, N, C, h, w, H, W, hf, wf, None)
    mrg = lambda B=1, N=1, C=1, h=4, w=4, H=8, W=16, hf=90.0, wf=90.0, count=p: lib.omni_freeview_merge_f32(p, p, count, p, B, N, C, h, w, H, W, hf, wf, None)
    for call in (e2p, p2e, mrg):
        for bad in (dict(N=0), dict(N=-3), dict(h=1), dict(w=1), dict(hf=0.0), dict(hf=180.0), dict(wf=-10.0), dict(wf=200.0), dict(hf=float("nan")), dict(C=0)):
            assert call(**bad) == _lib.OMNI_ERR_INVALID, bad
            assert lib.omni_last_error()
    assert e2p(erp=None) == e2p(pers=None) == e2p(rot=None) == _lib.OMNI_ERR_INVALID
    assert e2p(layout=_lib.LAYOUT_BCHWN) == e2p(layout=7) == e2p(B=0) == _lib.OMNI_ERR_INVALID
    assert p2e(mask=None) == mrg(count=None) == mrg(B=0) == mrg(N=256) == _lib.OMNI_ERR_INVALID
    assert b"null" in lib.omni_last_error() or b"255" in lib.omni_last_error()
    one = np.zeros(1, np.float32)
    out = np.zeros(18, np.float32)
    assert lib.omni_freeview_rotations(None, one.ctypes.data, 1, out.ctypes.data, None) == _lib.OMNI_ERR_INVALID
    assert lib.omni_freeview_rotations(one.ctypes.data, one.ctypes.data, 0, out.ctypes.data, None) == _lib.OMNI_ERR_INVALID
    assert lib.omni_freeview_rotations(one.ctypes.data, one.ctypes.data, 1, None, None) == _lib.OMNI_ERR_INVALID
    nan = np.array([np.nan], np.float32)
    assert lib.omni_freeview_rotations(nan.ctypes.data, one.ctypes.data, 1, out.ctypes.data, None) == _lib.OMNI_ERR_INVALID


def test_mirrors_have_no_cpu_path():
    from omnifusion_amd import util
    from omnifusion_amd.equi_pers import views_to_erp
    from omnifusion_amd.equi_pers.equi2pers_torch import equi2pers, equi2pers_planar
    from omnifusion_amd.equi_pers.pers2equi_torch import pers2equi
    theta, phi = torch.tensor([10.0, 20.0]), torch.tensor([0.0, 5.0])
    with pytest.raises(ValueError, match="no CPU path"):
        equi2pers(torch.zeros(1, 3, 8, 16), 80, 80, theta, phi, 4, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        equi2pers_planar(torch.zeros(1, 3, 8, 16), 80, 80, theta, phi, 4, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        pers2equi(torch.zeros(2, 3, 4, 4), 80, 80, theta, phi, 8, 16)
    with pytest.raises(ValueError, match="no CPU path"):
        views_to_erp(torch.zeros(1, 2, 3, 4, 4), 80, 80, theta, phi, 8, 16)
    with pytest.raises(ValueError, match="no CPU path"):
        util.transform_equi(torch.zeros(1, 3, 8, 16), theta, phi, 4, 4, 2, 80, 80)
    with pytest.raises(ValueError, match="no CPU path"):
        util.transform_pers(torch.zeros(2, 3, 4, 4), theta, phi, 8, 16, 80, 80)


def test_mirrors_fail_without_the_library(tmp_path):
    """No library, no result: the loader raises, the mirrors do not compute anything themselves."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import omnifusion_amd._lib as L\n"
            "L.LIB_PATH = %r\n"
            "from omnifusion_amd.equi_pers import _freeview\n"
            "try:\n    _freeview.rotations([0.0], [0.0])\nexcept ImportError as e:\n    print('RAISED', type(e).__name__)\n") % (root, str(tmp_path / "nope.so"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "RAISED OmniLibraryMissing" in out.stdout, out.stdout + out.stderr
