"""CPU: the boundary of the plane-fit normals (equi_pers.depth2normal, supervision.geometry.planefit_normal_loss) — names, exported symbols, the
workspace query, argument checks that return before a device is touched, the Python errors — and the float64 restatement of
tests/_planefit_cases.py against the committed fixtures G22a-g, against its own hand-written backward and, where the checkout is present,
against the reference itself."""
import ctypes

import numpy as np
import pytest
import torch

import _planefit_cases as pc
from _util import golden
from oracle import ref_loader

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
NEW_SYMBOLS = ("omni_planefit_workspace_bytes", "omni_planefit_normals_f32", "omni_planefit_normals_grad_f32", "omni_planefit_loss_f32",
               "omni_planefit_loss_grad_f32")


def test_names_and_reexports():
    import omnifusion_amd.supervision as S
    from omnifusion_amd.equi_pers import depth2normal as module
    from omnifusion_amd.supervision import geometry
    assert callable(module.depth2normal)
    assert S.planefit_normal_loss is geometry.planefit_normal_loss
    for name in ("geometry_terms", "normal_loss", "gradient_loss"):                    # the neighbours stay where they were
        assert getattr(S, name) is getattr(geometry, name)


def test_symbols_exported():
    from omnifusion_amd import _lib
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name


def test_workspace_query():
    from omnifusion_amd import _lib
    L = _lib.load()
    for H, W in [(1, 1), (2, 2), (17, 67), (512, 1024)]:
        sizes = [L.omni_planefit_workspace_bytes(B, H, W) for B in (1, 2, 3, 8, 64)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes                   # monotone in B
        tiles = ((H + 15) // 16) * ((W + 63) // 64)
        assert sizes[0] >= 48 * H * W + 16 * tiles + 8                              # the [6,H,W] double map, two double partials per tile, two sums
    for bad in [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, -3), (65536, 8, 8), (1, 65536, 32768)]:
        assert L.omni_planefit_workspace_bytes(*bad) == 0, bad


def test_c_boundary_rejects_before_touching_a_device():
    """Null pointers, B < 1, H or W < 1 and a misaligned workspace: OMNI_ERR_INVALID.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, odd, z = ctypes.c_void_p(4096), ctypes.c_void_p(4104), None
    INV = _lib.OMNI_ERR_INVALID
    fwd, bwd, loss, lgrad = L.omni_planefit_normals_f32, L.omni_planefit_normals_grad_f32, L.omni_planefit_loss_f32, L.omni_planefit_loss_grad_f32
    assert fwd(z, p, 1, 8, 8, p, z) == INV and fwd(p, z, 1, 8, 8, p, z) == INV and fwd(p, p, 1, 8, 8, z, z) == INV
    assert fwd(p, p, 0, 8, 8, p, z) == INV and fwd(p, p, 1, 0, 8, p, z) == INV and fwd(p, p, 1, 8, 0, p, z) == INV
    for k in range(5):
        args = [p] * 3 + [1, 8, 8] + [p] * 2
        args[k if k < 3 else k + 3] = z
        assert bwd(*args, z) == INV, k
    assert bwd(p, p, p, 0, 8, 8, p, p, z) == INV and bwd(p, p, p, 1, 8, -1, p, p, z) == INV
    assert bwd(p, p, p, 1, 8, 8, odd, p, z) == INV and b"aligned" in L.omni_last_error()
    for k in range(6):
        args = [p] * 4 + [1, 8, 8, 0] + [p] * 2
        args[k if k < 4 else k + 4] = z
        assert loss(*args, z) == INV, k
    assert loss(p, p, p, p, 0, 8, 8, 0, p, p, z) == INV and loss(p, p, p, p, 1, 0, 8, 0, p, p, z) == INV
    assert loss(p, p, p, p, 1, 8, 8, 1, odd, p, z) == INV and b"aligned" in L.omni_last_error()
    for k in range(7):
        args = [p] * 4 + [1, 8, 8, 0] + [p] * 3
        args[k if k < 4 else k + 4] = z
        assert lgrad(*args, z) == INV, k
    assert lgrad(p, p, p, p, -2, 8, 8, 0, p, p, p, z) == INV
    assert lgrad(p, p, p, p, 1, 8, 8, 0, odd, p, p, z) == INV and b"aligned" in L.omni_last_error()


def test_python_errors():
    from omnifusion_amd.equi_pers.depth2normal import depth2normal
    from omnifusion_amd.supervision import planefit_normal_loss
    d, m = torch.rand(1, 1, 8, 16) + 1, torch.ones(1, 1, 8, 16)
    with pytest.raises(ValueError, match="must be a tensor"):
        depth2normal(d.numpy())
    with pytest.raises(ValueError, match="must be a tensor on an MI355X device; there is no CPU path"):
        depth2normal(d)
    with pytest.raises(ValueError, match="no CPU path"):                              # no requires-grad rejection: the map is differentiable
        depth2normal(d.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no CPU path"):
        planefit_normal_loss(d, d, m)
    with pytest.raises(ValueError, match="must not require grad"):
        planefit_normal_loss(d, d.clone().requires_grad_(True), m)
    with pytest.raises(ValueError, match="must not require grad"):
        planefit_normal_loss(d, d, m.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="must be a tensor"):
        planefit_normal_loss(d, None, m)


@pytest.mark.parametrize("name", pc.NAMES)
def test_restatement_reproduces_golden(name):
    """float64 restatement against the fixture: the loss to 1e-9; the arrays are stored as float32, so they agree to that rounding."""
    c, g = pc.case(name), golden(name + "_planefit")
    for k, v in pc.checksums(c).items():
        assert float(g["sum_" + k]) == float(v), f"{name}: the seeded input {k} is not the one the fixture was made from"
    r = pc.run_restatement(c, torch.float64, name=name)
    for k in ("normals", "grad_map", "grad_loss"):
        assert (k in g.files) == (k in r), k
        if k in r:
            want = g[k].astype(np.float64)
            assert np.abs(r[k] - want).max() <= 1e-9 + 6e-8 * np.abs(want).max(), k
    if name == "G22g":
        assert np.abs(r["det"] - g["det"]).max() <= 1e-12 * np.abs(g["det"]).max()
        assert int(pc.band(r["det"], pc.G_BAND).sum()) == int(g["band_pixels"]) <= 0.01 * r["det"].size
    else:
        assert abs(r["loss"] - float(g["loss"])) <= 1e-9
        assert int((r["det"] < pc.DET_MIN).sum() + (r["det_gt"] < pc.DET_MIN).sum()) == int(g["fallback_pixels"])
    if name == "G22b":
        assert int(g["fallback_pixels"]) == 8                                         # every window is its centre
        rays = pc.rays(2, 2)[None].astype(np.float64)
        assert np.abs(r["normals"] - rays / np.linalg.norm(rays, axis=1, keepdims=True)).max() <= 1e-15      # the normal is the ray


@pytest.mark.parametrize("name", ["G22a", "G22b", "G22f"])
def test_hand_written_backward_is_autograd(name):
    """The closed form the kernels implement against autograd of the restatement in float64: <= 1e-10 of the largest element, for the map's and
    the loss's gradient.  G22b: every pixel takes the fallback and its normal is its ray, whatever the depth — the exact gradient is 0 and the
    largest element of either array is round-off; there the yardstick is the size of the two terms that cancel, max|upstream| / min|depth|."""
    c = pc.case(name)
    r = pc.run_restatement(c, torch.float64, name=name, hand=True)
    B = c["pred"].shape[0]
    scales = {"grad_map": np.abs(pc.upstream(name)).max() / np.abs(c["pred"]).min(), "grad_loss": 1.0 / (B * c["mask"].sum() * np.abs(c["pred"]).min())}
    for k in ("grad_map", "grad_loss"):
        largest = np.abs(r[k]).max()
        if name == "G22b":
            assert largest <= 1e-14 * scales[k], (k, largest)
            largest = scales[k]
        err = np.abs(r["hand_" + k] - r[k]).max()
        print(f"{name} {k}: largest {largest:.3e} error {err:.2e}")
        assert err <= 1e-10 * largest, (k, err, largest)


@needs_reference
@pytest.mark.parametrize("name", pc.NAMES)
def test_restatement_equals_reference(name):
    """float64: to 1e-12 (what the generator asserts).  float32: both are the same formulae in other operation orders, so they differ by about the
    error of either against float64 — the fixture's ref32 figures; the branch may differ only within 1 % of the threshold."""
    c, g = pc.case(name), golden(name + "_planefit")
    ref, r = pc.run_reference(c, torch.float64, name), pc.run_restatement(c, torch.float64, name=name)
    for k in ref:
        assert np.abs(np.asarray(r[k]) - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k
    ref32, r32 = pc.run_reference(c, torch.float32, name), pc.run_restatement(c, torch.float32, name=name)
    flips = ((ref32["det"] >= pc.DET_MIN) != (r32["det"] >= pc.DET_MIN)) & ~pc.band(ref["det"], pc.G_BAND)
    assert not flips.any()
    same = (ref32["det"] >= pc.DET_MIN) == (r32["det"] >= pc.DET_MIN)
    e = np.abs(r32["normals"].astype(np.float64) - ref32["normals"])[np.broadcast_to(same[:, None], ref32["normals"].shape)].max()
    assert e <= max(1e-5, 8 * float(g["ref32_normals_err"])), e
