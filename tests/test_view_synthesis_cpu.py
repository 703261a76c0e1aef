"""CPU: the boundary of differentiable view synthesis — supervision.photometric / supervision.ssim import and refuse CPU tensors and
bad arguments, the library exports the backward and photometric symbols, the G15 / G16 fixtures belong to the regenerated inputs, and
the G15a / G16a recipes reproduce the committed fixtures bit for bit."""
import numpy as np
import pytest
import torch

from oracle import ref_loader


def test_modules_import_and_defaults():
    from omnifusion_amd import supervision
    from omnifusion_amd.supervision import photometric, ssim
    assert supervision.calculate_loss is photometric.calculate_loss and supervision.ssim_loss is ssim.ssim_loss
    p = photometric.PhotometricLossParameters()
    assert (p.get_alpha(), p.get_l1_estimator(), p.get_ssim_estimator(), p.get_window(), p.get_std(), p.get_ssim_mode()) == \
        (0.85, 'none', 'none', 7, 1.5, 'gaussian')


def test_cpu_tensors_and_bad_arguments_raise():
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    from omnifusion_amd.supervision.ssim import ssim_loss
    a, b = torch.rand(1, 3, 16, 32), torch.rand(1, 3, 16, 32)
    m, w = torch.ones(1, 1, 16, 32), torch.ones(1, 1, 16, 32)
    with pytest.raises(ValueError, match="no CPU path"):
        ssim_loss(a, b)
    with pytest.raises(ValueError, match="no CPU path"):
        calculate_loss(a, b, PhotometricLossParameters(), m, w)
    with pytest.raises(ValueError, match="no CPU path"):
        calculate_loss(a.clone().requires_grad_(True), b, PhotometricLossParameters(), m, w)
    for window in (4, 13, 1):                                     # even, > 11, < 3: refused before the device is looked at
        with pytest.raises(ValueError, match="window"):
            calculate_loss(a, b, PhotometricLossParameters(window=window), m, w)
        with pytest.raises(ValueError, match="window"):
            ssim_loss(a, b, kernel_size=window)
    with pytest.raises(ValueError, match="mode"):
        ssim_loss(a, b, mode="hann")
    with pytest.raises(ValueError, match="mode"):
        calculate_loss(a, b, PhotometricLossParameters(ssim_mode="hann"), m, w)


def test_cpu_grad_tensor_error_names_both():
    """A CPU tensor that requires grad stays an error (tests/test_dibr_cpu.py matches "requires grad"); it also says why."""
    from omnifusion_amd.supervision.splatting import render
    from omnifusion_amd.spherical import create_image_grid
    img, depth = torch.rand(1, 3, 8, 16), torch.rand(1, 1, 8, 16)
    with pytest.raises(ValueError, match="requires grad.*no CPU path"):
        render(img, depth.clone().requires_grad_(True), create_image_grid(16, 8))


def test_window_weights_are_the_references():
    from omnifusion_amd.supervision.ssim import window_weights
    import math
    for k, std in ((7, 1.5), (5, 1.5), (11, 2.0)):
        win, code = window_weights(k, std, "gaussian")
        g = np.array([math.exp(-(x - k // 2) ** 2 / float(2 * std ** 2)) for x in range(k)])
        assert code == 0 and np.array_equal(np.array(list(win), np.float32), (g / g.sum()).astype(np.float32))
    win, code = window_weights(3, 1.5, "box")
    assert code == 1 and list(win) == [np.float32(1 / 3)] * 3


def test_library_exports_backward_and_photometric_symbols():
    from omnifusion_amd import _lib
    L = _lib.load()
    for name in ("omni_splat_render_wt_f32", "omni_dibr_wt_f32", "omni_dibr_bwd_workspace_bytes", "omni_splat_render_bwd_f32", "omni_dibr_bwd_f32",
                 "omni_ssim_f32", "omni_photometric_workspace_bytes", "omni_photometric_grad_scratch_bytes", "omni_photometric_loss_f32",
                 "omni_photometric_grad_f32"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.omni_dibr_bwd_workspace_bytes(2, 3, 64, 128) == 4 * 4 * 2 * 64 * 128          # one 16-byte record per target at C = 3
    assert L.omni_dibr_bwd_workspace_bytes(1, 4, 8, 8) == 4 * 8 * 64 and L.omni_dibr_bwd_workspace_bytes(0, 3, 8, 8) == 0
    assert L.omni_photometric_grad_scratch_bytes(2, 3, 64, 128) == 4 * 3 * 2 * 3 * 64 * 128
    assert L.omni_photometric_workspace_bytes(2, 3, 64, 128) >= 16 * 2 * 3 * 4 * 4 + 8


def test_fixture_checksums_match_regenerated_inputs():
    import _vs_cases as vc
    from _util import golden
    for name in vc.DIBR_NAMES:
        g = golden(name + "_dibr_bwd")
        for k, v in vc.checksums(vc.dibr_case(name)).items():
            assert float(g["sum_" + k]) == float(v), (name, k)
    for name in vc.PHOTO_NAMES:
        g = golden(name + "_photometric")
        for k, v in vc.checksums(vc.photo_case(name)).items():
            assert float(g["sum_" + k]) == float(v), (name, k)


def test_fixtures_record_the_references_own_error_inside_the_gate():
    """The parity gate of the GPU tests (share over 1e-4 <= 2e-4, nothing over 1e-2; photometric 1e-4 everywhere) is met by the
    reference's own float32 run against its float64 run; the depth gradient is non-finite exactly on the 13 x 11 zero block."""
    import _vs_cases as vc
    from _util import golden
    for name in vc.DIBR_NAMES:
        g = golden(name + "_dibr_bwd")
        c = vc.dibr_case(name)
        for k in vc.dibr_grad_names(c):
            assert float(g["ref32_share_" + k]) <= 2e-4 and float(g["ref32_max_" + k]) <= 1e-2, (name, k)
        assert np.array_equal(~np.isfinite(g["grad_depth"]), (c["depth"] == 0) & (c["kind"] != "render")), name
        assert np.isfinite(g["grad_img"]).all()
    for name in vc.PHOTO_NAMES:
        g = golden(name + "_photometric")
        assert float(g["ref32_grad_max"]) <= 1e-4 and float(g["ref32_loss_err"]) <= 2e-6 and 0.0 < float(g["dssim_min"]) and float(g["dssim_max"]) < 1.0


@pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
def test_g15a_and_g16a_recipes_reproduce_fixtures():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_golden_dibr_bwd
    import gen_golden_photometric
    from _util import golden
    for mod, name, suffix in ((gen_golden_dibr_bwd, "G15a", "_dibr_bwd"), (gen_golden_photometric, "G16a", "_photometric")):
        _, out = mod.build(name)
        g = golden(name + suffix)
        assert sorted(out) == sorted(g.files)
        for k, v in out.items():
            assert np.array_equal(np.asarray(v), g[k], equal_nan=True), (name, k)
