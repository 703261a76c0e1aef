"""GPU: the guided smoothness term (csrc/omni_smoothness.hip) against the fixtures G20a-e — the reference's own float64 loss, maps and autograd
gradient (tools/gen_golden_smoothness.py) — the fused form against the composition of the stand-alone mirrors, a directional derivative, and
the properties: repeated runs, the kinks of G20b, non-finite values at masked pixels, mask dtypes, the empty mask and bad arguments.

The gate is DESIGN.md §14's rule: max(1e-5, 4 x the reference's own float32 error stored in the fixture) — absolute for the loss and the maps,
relative to the largest reference gradient for the gradient."""
import numpy as np
import pytest
import torch

import _smoothness_cases as sc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def gate(g, key):
    return max(1e-5, 4 * float(g[key]))


def run(c, depth=None):
    """-> (loss, depth tensor with requires_grad) of depth_smoothness on the case."""
    from omnifusion_amd.supervision import depth_smoothness
    d, image, mask, weights, sg = sc.tensors(c if depth is None else dict(c, depth=depth), torch.float32, DEV)
    d.requires_grad_(True)
    return depth_smoothness(d, image, mask, weights, sg), d


def loss_and_grad(c):
    loss, d = run(c)
    grad, = torch.autograd.grad(loss, d)
    return loss.detach(), grad


@pytest.mark.parametrize("name", sc.NAMES)
def test_parity_with_reference(name):
    """The fused loss, the stand-alone maps and the gradient against the float64 golden."""
    from omnifusion_amd.spherical import coords_3d, dI_duv, dV_dxyz
    c, g = sc.case(name), golden(name + "_smoothness")
    loss, grad = loss_and_grad(c)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    err = abs(float(loss) - float(g["loss"]))
    print(f"{name} loss: {float(loss):.9f} golden {float(g['loss']):.9f} error {err:.2e} (reference float32: {float(g['ref32_loss_err']):.1e})")
    assert err <= gate(g, "ref32_loss_err"), err
    e = sc.rel_error(grad.cpu().numpy(), g["grad"]).max()
    print(f"{name} grad: max error {e:.2e} of the largest gradient (reference float32: {float(g['ref32_grad_max']):.1e})")
    assert grad.shape == c["depth"].shape and np.isfinite(grad.cpu().numpy()).all() and e <= gate(g, "ref32_grad_max"), e
    depth, image, _, _, sg = sc.tensors(c, torch.float32, DEV)
    for got, key in ((dV_dxyz(coords_3d(sg, depth)), "dV_dxyz"), (dI_duv(image), "dI_duv")):
        assert got.shape == c["depth"].shape and got.dtype == torch.float32
        e = np.abs(got.cpu().numpy().astype(np.float64) - g[key]).max()
        print(f"{name} {key}: max error {e:.2e} (reference float32: {float(g['ref32_' + key + '_err']):.1e})")
        assert e <= gate(g, "ref32_" + key + "_err"), (key, e)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fused_against_unfused(name):
    """depth_smoothness against guided_smoothness_loss over the stand-alone mirrors on the device (the same gate as the golden's, around the
    unfused value); its gradient against torch.autograd through the float64 restatement of that composition on the device."""
    from omnifusion_amd.spherical import coords_3d, dI_duv, dV_dxyz
    from omnifusion_amd.supervision import guided_smoothness_loss
    c, g = sc.case(name), golden(name + "_smoothness")
    loss, grad = loss_and_grad(c)
    depth, image, mask, weights, sg = sc.tensors(c, torch.float32, DEV)
    unfused = guided_smoothness_loss(dV_dxyz(coords_3d(sg, depth)), dI_duv(image), mask, torch.ones_like(depth) if weights is None else weights)
    assert unfused.dtype == torch.float32 and unfused.dim() == 0
    assert abs(float(loss) - float(unfused)) <= gate(g, "ref32_loss_err"), (float(loss), float(unfused))
    r = sc.run_restatement(c, torch.float64, DEV)
    assert sc.rel_error(grad.cpu().numpy(), r["grad"]).max() <= gate(g, "ref32_grad_max")


def test_stand_alone_maps_and_the_elementwise_gradient():
    """dI_du / dI_dv and dV_dx / dV_dy / dV_dz against the restatement's differences (exact: one float32 subtraction; the norms to 1e-6), the
    [1,1,H,W] weights of spherical_confidence, and the trivial backward of guided_smoothness_loss against autograd."""
    from omnifusion_amd.spherical import coords_3d, dI_du, dI_dv, dI_duv, dV_dx, dV_dy, dV_dz, spherical_confidence
    from omnifusion_amd.supervision import depth_smoothness, guided_smoothness_loss
    c = sc.case("G20c")
    depth, image, mask, weights, sg = sc.tensors(c, torch.float32, DEV)
    assert torch.equal(dI_du(image), sc.diff_u(image)) and torch.equal(dI_dv(image), sc.diff_v(image))
    assert float(dI_du(image)[..., -1].abs().max()) == 0.0 and float(dI_dv(image)[..., -1, :].abs().max()) == 0.0
    V = coords_3d(sg, depth)
    for k, fn in enumerate((dV_dx, dV_dy, dV_dz)):
        assert float((fn(V).double() - sc.image_norm(V[:, k:k + 1].double())).abs().max()) <= 1e-6
    mag = sc.vertex_norm(V).requires_grad_(True)
    guide = dI_duv(image)
    loss = guided_smoothness_loss(mag, guide, mask, weights)
    grad, = torch.autograd.grad(loss, mag)
    m64 = mag.detach().double().requires_grad_(True)
    ref = sc.loss_of_maps(m64, guide.double(), mask, weights.double())
    g64, = torch.autograd.grad(ref, m64)
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 and float((grad.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    conf = spherical_confidence(sg)
    assert conf.shape == (1, 1) + depth.shape[2:]
    a = depth_smoothness(depth, image, mask, conf, sg)
    b = depth_smoothness(depth, image, mask, conf.expand(depth.shape).contiguous(), sg)
    assert torch.equal(a, b) and abs(float(a) - float(sc.loss_of_depth(depth.double(), image.double(), mask, conf.double(), sg.double()))) <= 1e-5


def test_directional_derivative():
    """(L(d + h v) - L(d - h v)) / 2h against <grad, v> on G20a, h = 3e-3, v the modulated checkerboard of tests/_smoothness_cases.py; tolerance
    as in tests/test_geometry_gpu.py: twice the residual the same check leaves on the reference's float32 run (recorded in the fixture, 9.5e-6).
    The residual of the reference's float64 run is recorded beside it (4.4e-8); it is below what a float32 loss can resolve — one unit in the
    last place of the loss, 2.4e-7, over the difference of 2.2e-2 is 1.1e-5 — so it cannot gate a float32 result."""
    c, g = sc.case("G20a"), golden("G20a_smoothness")
    _, grad = loss_and_grad(c)
    res, fd, dot = sc.directional_residual(lambda d: float(run(c, depth=d)[0].detach()), grad.double().cpu().numpy(), c["depth"], sc.direction("G20a"), sc.DIRECTION_H)
    tol = 2 * float(g["ref32_direction_residual"])
    print(f"finite difference {fd:.8e}, <grad, v> {dot:.8e}, residual {res:.3e}, tolerance {tol:.3e} (reference float64 residual {float(g['ref64_direction_residual']):.1e})")
    assert res <= tol, (res, fd, dot)


def test_bitwise_repeatable_and_independent_of_workspace_contents():
    """Two runs give the same bits; so does a run whose workspace is a recycled block full of other values."""
    from omnifusion_amd import _lib
    c = sc.case("G20d")
    a = loss_and_grad(c)
    b = loss_and_grad(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    B, _, H, W = c["depth"].shape
    nbytes = _lib.load().omni_depth_smoothness_workspace_bytes(B, H, W)
    for fill in (float("nan"), 1e30):
        junk = torch.full((nbytes // 8 + 1,), fill, dtype=torch.float64, device=DEV)
        del junk
        assert all(torch.equal(x, y) for x, y in zip(a, loss_and_grad(c)))


def test_kinks_of_g20b():
    """2 x 2: with the mask on one pixel at a time, the gradient is exactly 0 — not NaN — wherever the restatement's is: the last column's du and
    the last row's dv contribute nothing (d|x|/dx = 0 at 0), the bottom-right term nothing at all (the 2-norm's gradient is 0 at 0); elsewhere
    it is the restatement's to the gate.  With the full mask every entry is finite and the restatement's."""
    c, g = sc.case("G20b"), golden("G20b_smoothness")
    masks = [np.array([[[[(a, b) == (i, j) for b in range(2)] for a in range(2)]]]) for i in range(2) for j in range(2)] + [np.ones((1, 1, 2, 2), bool)]
    for mask in masks:
        cm = dict(c, mask=mask)
        loss, grad = loss_and_grad(cm)
        r = sc.run_restatement(cm, torch.float64)
        got = grad.cpu().numpy()
        assert np.isfinite(got).all() and np.isfinite(float(loss))
        assert np.array_equal(got == 0, r["grad"] == 0), (mask, got, r["grad"])
        assert np.abs(got - r["grad"]).max() <= gate(g, "ref32_grad_max") * np.abs(r["grad"]).max() and abs(float(loss) - r["loss"]) <= gate(g, "ref32_loss_err")
    loss, _ = loss_and_grad(dict(c, mask=masks[3]))
    assert float(loss) == 0.0                                                # the bottom-right term is 0 / 1


def test_non_finite_values_at_masked_pixels():
    """A NaN depth and an infinite weight at a masked pixel whose left and upper neighbours are masked too: the loss is finite and the same
    bits as without them; the gradient is finite and the same bits everywhere but at that pixel's own entry, which is 0 as in the restatement's
    gather (tests/_smoothness_cases.py grad_by_hand)."""
    c = sc.case("G20e")
    poisoned, (b, i, j) = sc.poison(c)
    clean = dict(c, mask=poisoned["mask"])
    la, ga = loss_and_grad(clean)
    lp, gp = loss_and_grad(poisoned)
    assert np.isfinite(float(lp)) and torch.equal(la, lp)
    own = torch.zeros_like(gp, dtype=torch.bool)
    own[b, 0, i, j] = True
    assert bool(torch.isfinite(gp[~own]).all()) and torch.equal(ga[~own], gp[~own])
    hand = sc.grad_by_hand(*sc.tensors(poisoned, torch.float64, DEV))
    assert float(hand[b, 0, i, j]) == 0.0 and float(gp[b, 0, i, j]) == 0.0
    assert sc.rel_error(gp.cpu().numpy(), hand.cpu().numpy()).max() <= 1e-5


def test_mask_dtypes_and_layouts_give_the_same_bits():
    from omnifusion_amd.supervision import depth_smoothness
    c = sc.case("G20c")
    loss, grad = loss_and_grad(c)
    depth, image, mask, weights, sg = sc.tensors(c, torch.float32, DEV)
    for m in (mask.to(torch.uint8), mask.float(), mask.double() * 0.5, mask.to(torch.int64) * 7):
        assert torch.equal(depth_smoothness(depth, image, m, weights, sg), loss)
    wide = torch.cat((depth, depth), dim=3)
    d = wide[..., :depth.shape[3]].requires_grad_(True)                      # a non-contiguous depth, a double image
    assert not d.is_contiguous()
    l2 = depth_smoothness(d, image.double(), mask, weights, sg)
    g2, = torch.autograd.grad(l2, d)
    assert torch.equal(l2.detach(), loss) and torch.equal(g2, grad)


def test_default_grid_is_create_spherical_grid():
    """sgrid=None at H == W // 2 is create_spherical_grid(W): the same bits as passing it."""
    from omnifusion_amd.spherical import create_spherical_grid
    from omnifusion_amd.supervision import depth_smoothness
    g = torch.Generator(device=DEV).manual_seed(2051)
    depth = 1 + 3 * torch.rand(1, 1, 16, 32, device=DEV, generator=g)
    image = torch.rand(1, 3, 16, 32, device=DEV, generator=g)
    mask = torch.rand(1, 1, 16, 32, device=DEV, generator=g) < 0.8
    a = depth_smoothness(depth, image, mask)
    assert torch.equal(a, depth_smoothness(depth, image, mask, None, create_spherical_grid(32, device=DEV)))
    assert abs(float(a) - float(sc.loss_of_depth(depth.double(), image.double(), mask, None, create_spherical_grid(32, device=DEV).double()))) <= 1e-5


def test_empty_mask_is_nan_and_bad_arguments_raise():
    """sum(mask) == 0: the reference's 0 / 0."""
    from omnifusion_amd.supervision import depth_smoothness
    c = sc.case("G20a")
    loss, d = run(dict(c, mask=np.zeros_like(c["mask"])))
    assert np.isnan(float(loss.detach()))
    depth, image, mask, weights, sg = sc.tensors(c, torch.float32, DEV)
    with pytest.raises(ValueError, match="same shape"):
        depth_smoothness(depth, image, mask[:, :, :-1], weights, sg)
    with pytest.raises(ValueError, match=r"image must be \[B,C,H,W\]"):
        depth_smoothness(depth, image[..., :-1], mask, weights, sg)
    with pytest.raises(ValueError, match=r"depth must be a non-empty \[B,1,H,W\]"):
        depth_smoothness(image, image, mask, weights, sg)
    with pytest.raises(ValueError, match="weights must be"):
        depth_smoothness(depth, image, mask, weights[:1, :, :1], sg)
    with pytest.raises(ValueError, match="no CPU path"):
        depth_smoothness(depth.cpu(), image, mask, weights, sg)
    with pytest.raises(ValueError, match="must not require grad"):
        depth_smoothness(depth, image.clone().requires_grad_(True), mask, weights, sg)
    with pytest.raises(ValueError, match=r"sgrid must be a \[1,2,H,W\]"):
        depth_smoothness(depth, image, mask, weights, sg[..., :-1])
