"""CPU: the DIBR / splat boundary — the modules import, bad inputs raise ValueError (no CPU path, inference only), the grids are
the reference's, the workspace size is consistent, and the G14a recipe reproduces the committed fixture bit for bit."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_loader


def test_modules_import_and_reject_cpu_and_grad():
    from omnifusion_amd.supervision.splatting import render
    from omnifusion_amd.util import dibr_horizontal, dibr_vertical
    from omnifusion_amd.spherical import create_image_grid, create_spherical_grid
    img, depth = torch.rand(1, 3, 8, 16), torch.rand(1, 1, 8, 16)
    uv, sg = create_image_grid(16, 8), create_spherical_grid(16)
    with pytest.raises(ValueError, match="no CPU path"):
        render(img, depth, uv.clone())
    for fn in (dibr_vertical, dibr_horizontal):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(depth, img, uv, sg, 0.26)
        with pytest.raises(ValueError, match="requires grad"):
            fn(depth.clone().requires_grad_(True), img, uv, sg, 0.26)
    with pytest.raises(ValueError, match="requires grad"):
        render(img.clone().requires_grad_(True), depth, uv.clone())


def test_grid_shapes_and_values():
    from omnifusion_amd.spherical import create_image_grid, create_spherical_grid
    uv = create_image_grid(32, 16)
    assert uv.shape == (1, 2, 16, 32) and uv.dtype == torch.float32
    assert torch.equal(uv[0, 0, 3], torch.arange(32, dtype=torch.float32)) and torch.equal(uv[0, 1, :, 5], torch.arange(16, dtype=torch.float32))
    sg = create_spherical_grid(32)
    assert sg.shape == (1, 2, 16, 32)
    assert abs(sg[0, 0, 0, 0].item() + 1.5 * np.pi) < 1e-6 and abs(sg[0, 1, 0, 0].item() + 0.5 * np.pi) < 1e-6
    assert create_spherical_grid(32, data_type=torch.float64).dtype == torch.float64


@pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
@pytest.mark.parametrize("W", [64, 256, 512, 1024])
def test_grids_equal_reference(W):
    import sys
    if ref_loader.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    import spherical as S360
    from omnifusion_amd import spherical as mine
    assert torch.equal(mine.create_image_grid(W, W // 2), S360.create_image_grid(W, W // 2))
    assert torch.equal(mine.create_spherical_grid(W), S360.create_spherical_grid(W))
    assert torch.equal(mine.create_spherical_grid(W, 0.5, -0.25), S360.create_spherical_grid(W, 0.5, -0.25))


def test_workspace_bytes_consistent():
    from omnifusion_amd import _lib
    L = _lib.load()
    for B, C, H, W in [(1, 1, 4, 8), (2, 3, 64, 128), (8, 3, 512, 1024), (3, 5, 7, 11)]:
        n = L.omni_dibr_workspace_bytes(B, C, H, W)
        need = 8 * B * (C + 1) * H * W + 4 * B * H * W             # int64 sums per channel + weight, one poison word per target
        assert need <= n <= need + 4096, (B, C, H, W, n)
        assert L.omni_dibr_workspace_bytes(B + 1, C, H, W) > n and L.omni_dibr_workspace_bytes(B, C + 1, H, W) > n
    assert L.omni_dibr_workspace_bytes(0, 3, 8, 8) == 0 and L.omni_dibr_workspace_bytes(1, 3, -1, 8) == 0


def test_fixture_checksums_match_regenerated_inputs():
    import _dibr_cases as dc
    from _util import golden
    for name in dc.NAMES:
        g = golden(name + "_dibr")
        for k, v in dc.checksums(dc.case(name)).items():
            assert float(g["sum_" + k]) == float(v), (name, k)


@pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
def test_g14a_recipe_reproduces_fixture():
    import _dibr_cases as dc
    from _util import golden
    recon, mask = dc.run_reference(dc.case("G14a"))
    g = golden("G14a_dibr")
    assert np.abs(recon - g["recon"]).max() == 0.0
    assert np.array_equal(mask.astype(np.uint8), g["mask"])
