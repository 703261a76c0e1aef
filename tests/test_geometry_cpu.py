"""CPU: the boundary of the geometry terms (supervision.geometry, util.depth2normal_gpu / imgrad / imgrad_yx, direct.calculate_l1_loss) — names,
exported symbols, argument checks that return before a device is touched, the Python errors — and the float64 restatement of
tests/_geometry_cases.py against the committed fixtures G19a-e and, where the checkout is present, against the reference itself."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import _geometry_cases as gc
from _util import golden
from oracle import ref_loader

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
NEW_SYMBOLS = ("omni_depth_normals_f32", "omni_sobel_f32", "omni_l1_workspace_bytes", "omni_l1_loss_f32", "omni_l1_grad_f32",
               "omni_geometry_terms_workspace_bytes", "omni_geometry_terms_f32", "omni_geometry_terms_grad_f32")


def test_names_and_reexports():
    import omnifusion_amd.supervision as S
    from omnifusion_amd import util
    from omnifusion_amd.supervision import direct, geometry
    assert S.geometry is geometry
    for name in ("geometry_terms", "normal_loss", "gradient_loss"):
        assert getattr(S, name) is getattr(geometry, name)
    for name in ("depth2normal_gpu", "imgrad", "imgrad_yx"):
        assert callable(getattr(util, name))
    assert callable(direct.calculate_l1_loss)


def test_symbols_exported():
    from omnifusion_amd import _lib
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_workspace_query():
    from omnifusion_amd import _lib
    L = _lib.load()
    for H, W in [(2, 2), (17, 67), (512, 1024)]:
        sizes = [L.omni_geometry_terms_workspace_bytes(B, H, W) for B in (1, 2, 3, 8, 64)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes                   # monotone in B
        tiles = ((H + 15) // 16) * ((W + 63) // 64)
        assert sizes[0] >= 24 * tiles + 12                                          # three double partials per tile, three floats of sums
    assert L.omni_geometry_terms_workspace_bytes(0, 8, 8) == 0 and L.omni_geometry_terms_workspace_bytes(1, 1, 8) == 0
    l1 = [L.omni_l1_workspace_bytes(B) for B in (1, 2, 8)]
    assert l1[0] < l1[1] < l1[2]


def test_c_boundary_rejects_before_touching_a_device():
    """Null pointers and B < 1: OMNI_ERR_INVALID; H or W < 2: OMNI_ERR_UNSUPPORTED.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    assert L.omni_depth_normals_f32(z, p, 1, 8, 8, p, z) == INV and L.omni_depth_normals_f32(p, p, 1, 8, 8, z, z) == INV
    assert L.omni_depth_normals_f32(p, p, 0, 8, 8, p, z) == INV
    assert L.omni_depth_normals_f32(p, p, 1, 1, 8, p, z) == UNS and L.omni_depth_normals_f32(p, p, 1, 8, 1, p, z) == UNS
    assert b"H, W >= 2" in L.omni_last_error()
    assert L.omni_sobel_f32(z, 1, 1, 8, 8, p, p, z) == INV and L.omni_sobel_f32(p, 0, 1, 8, 8, p, p, z) == INV
    assert L.omni_sobel_f32(p, 1, 0, 8, 8, p, p, z) == INV and L.omni_sobel_f32(p, 1, 1, 1, 8, p, p, z) == UNS
    assert L.omni_l1_loss_f32(p, p, z, 1, 1, 64, 1, p, p, z) == INV and L.omni_l1_loss_f32(p, p, p, 0, 1, 64, 1, p, p, z) == INV
    assert L.omni_l1_loss_f32(p, p, p, 1, 2, 64, 3, p, p, z) == INV                  # mask channels: 1 or C
    assert L.omni_l1_grad_f32(p, p, p, 1, 1, 64, 1, p, z, p, z) == INV and L.omni_l1_grad_f32(p, p, p, -1, 1, 64, 1, p, p, p, z) == INV
    assert L.omni_geometry_terms_f32(p, p, p, p, 1, 8, 8, 3, 0, z, p, z) == INV and L.omni_geometry_terms_f32(p, z, p, p, 1, 8, 8, 3, 0, p, p, z) == INV
    assert L.omni_geometry_terms_f32(p, p, p, p, 0, 8, 8, 3, 0, p, p, z) == INV and L.omni_geometry_terms_f32(p, p, p, p, 1, 8, 8, 0, 0, p, p, z) == INV
    assert L.omni_geometry_terms_f32(p, p, p, p, 1, 1, 8, 3, 0, p, p, z) == UNS and L.omni_geometry_terms_f32(p, p, p, p, 1, 8, 1, 3, 0, p, p, z) == UNS
    assert L.omni_geometry_terms_grad_f32(p, p, p, p, 1, 8, 8, 0, p, z, z, p, z) == INV    # no upstream gradient
    assert L.omni_geometry_terms_grad_f32(p, p, p, p, 1, 8, 8, 0, p, p, p, z, z) == INV
    assert L.omni_geometry_terms_grad_f32(p, p, p, p, 0, 8, 8, 0, p, p, p, p, z) == INV
    assert L.omni_geometry_terms_grad_f32(p, p, p, p, 1, 8, 1, 0, p, p, p, p, z) == UNS


def test_python_errors():
    from omnifusion_amd.supervision import geometry_terms, gradient_loss, normal_loss
    from omnifusion_amd.supervision.direct import calculate_l1_loss
    from omnifusion_amd.util import depth2normal_gpu, imgrad, imgrad_yx
    d, m = torch.rand(1, 1, 8, 16) + 1, torch.ones(1, 1, 8, 16)
    for fn in (depth2normal_gpu, imgrad, imgrad_yx):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(d)
        with pytest.raises(ValueError, match="forward only"):
            fn(d.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="single-channel"):
        imgrad_yx(torch.rand(1, 3, 8, 16))
    for fn in (geometry_terms, normal_loss, gradient_loss):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(d, d, m)
        with pytest.raises(ValueError, match="must not require grad"):
            fn(d, d.clone().requires_grad_(True), m)
        with pytest.raises(ValueError, match="must not require grad"):
            fn(d, d, m.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no CPU path"):
        calculate_l1_loss(d, d, m)


def test_ray_tables_are_the_rays_of_the_restatement():
    """The four separable tables the kernels read reproduce the full [3,H,W] ray grid bit for bit."""
    from omnifusion_amd.spherical.grid import ray_table_values
    for H, W in [(2, 2), (17, 67), (64, 128)]:
        t = ray_table_values(H, W)
        assert t.dtype == np.float32 and t.shape == (2 * H + 2 * W,)
        sv, cv, su, cu = t[:H], t[H:2 * H], t[2 * H:2 * H + W], t[2 * H + W:]
        grid = np.stack([cv[:, None] * su[None, :], cv[:, None] * cu[None, :], np.broadcast_to(sv[:, None], (H, W))])
        assert np.array_equal(grid, gc.rays(H, W))


@pytest.mark.parametrize("name", gc.NAMES)
def test_restatement_reproduces_golden(name):
    """float64 restatement against the fixture: losses to 1e-9; the arrays are stored as float32, so they agree to that rounding."""
    c, g = gc.case(name), golden(name + "_geometry")
    for k, v in gc.checksums(c).items():
        assert float(g["sum_" + k]) == float(v), f"{name}: the seeded input {k} is not the one the fixture was made from"
    r = gc.run_restatement(c, torch.float64)
    assert abs(r["normal_loss"] - float(g["normal_loss"])) <= 1e-9 and abs(r["grad_loss"] - float(g["grad_loss"])) <= 1e-9
    for k in ("normals", "grad_normal", "grad_grad"):
        want = g[k].astype(np.float64)
        assert np.abs(r[k] - want).max() <= 1e-9 + 6e-8 * np.abs(want).max(), k
    assert r["min_dsobel"] > 1e-6


@needs_reference
@pytest.mark.parametrize("name", ["G19a", "G19b", "G19e"])
def test_restatement_equals_reference_in_float32(name):
    c = gc.case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = gc.run_reference(c, torch.float32)
    r = gc.run_restatement(c, torch.float32)
    assert abs(r["normal_loss"] - ref["normal_loss"]) <= 2e-7 and abs(r["grad_loss"] - ref["grad_loss"]) <= 2e-7
    assert np.abs(r["normals"] - ref["normals"]).max() <= 1e-6
    for k in ("grad_normal", "grad_grad"):
        assert gc.rel_error(r[k], ref[k]).max() <= 1e-5, k


@needs_reference
def test_reference_crosses_over_the_batch_axis_at_b3():
    """at B = 3 the reference's `torch.cross` without `dim` runs over the batch axis; the product and the restatement never do."""
    c = gc.b3_case()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = gc.run_reference(c, torch.float64)
    r = gc.run_restatement(c, torch.float64)
    assert np.abs(r["normals"] - ref["normals"]).max() > 0.5
    assert np.abs(np.linalg.norm(r["normals"], axis=1) - 1).max() < 1e-12
