"""GPU: the geometry terms of depth training (csrc/omni_normals.hip) against the fixtures G19a-e — the reference's own float64 losses, normals and
autograd gradients (tools/gen_golden_geometry.py) — against stock float64 torch arithmetic on the device, a directional derivative, and the
bitwise properties: the single-term entries, repeated runs, workspace contents, mask dtypes, layouts and erode_mask on a full mask."""
import numpy as np
import pytest
import torch

import _geometry_cases as gc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def t(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, **kw)


def run(c, fn=None, pred=None):
    """-> (outputs, pred tensor with requires_grad) of geometry_terms (or `fn`) on the case."""
    from omnifusion_amd.supervision import geometry_terms
    p = t(c["pred"] if pred is None else pred).requires_grad_(True)
    return (fn or geometry_terms)(p, t(c["gt"]), t(c["mask"]), erode_mask=c["erode"]), p


def grads(c):
    (n, g), p = run(c)
    gn, = torch.autograd.grad(n, p, retain_graph=True)
    gg, = torch.autograd.grad(g, p)
    return n, g, gn, gg


@pytest.mark.parametrize("name", gc.NAMES)
def test_parity_with_reference(name):
    """Each loss within 2e-6 * max(1, |loss|) of the float64 golden, each gradient within 1e-4 of the largest reference gradient at every element,
    depth2normal_gpu(pred) within max(1e-5, 4 x the reference's own float32 error) of the golden normals."""
    from omnifusion_amd.util import depth2normal_gpu
    c, g = gc.case(name), golden(name + "_geometry")
    n, gl, gn, gg = grads(c)
    assert n.dtype == torch.float32 and n.dim() == 0 and n.is_cuda and gl.dtype == torch.float32 and gl.dim() == 0
    for got, key in ((n, "normal_loss"), (gl, "grad_loss")):
        want = float(g[key])
        err = abs(float(got.detach()) - want)
        print(f"{name} {key}: {float(got.detach()):.9f} golden {want:.9f} error {err:.2e} (reference float32: {float(g['ref32_' + key + '_err']):.1e})")
        assert err <= 2e-6 * max(1.0, abs(want)), (key, err)
    for got, key in ((gn, "grad_normal"), (gg, "grad_grad")):
        e = gc.rel_error(got.cpu().numpy(), g[key]).max()
        print(f"{name} {key}: max error {e:.2e} of the largest gradient (reference float32: {float(g['ref32_' + key + '_max']):.1e})")
        assert np.isfinite(got.cpu().numpy()).all() and e <= 1e-4, (key, e)
    normals = depth2normal_gpu(t(c["pred"]))
    assert normals.shape == (c["pred"].shape[0], 3) + c["pred"].shape[2:] and normals.dtype == torch.float32
    e = np.abs(normals.cpu().numpy().astype(np.float64) - g["normals"]).max()
    print(f"{name} normals: max error {e:.2e} (reference float32: {float(g['ref32_normals_err']):.1e})")
    assert e <= max(1e-5, 4 * float(g["ref32_normals_err"])), e


def test_imgrad_and_l1_against_float64_conv2d():
    """imgrad (3 channels: the mean comes first), imgrad_yx and calculate_l1_loss against stock float64 conv2d arithmetic on the device, <= 2e-6 (inputs
    in [0, 1): a Sobel value is at most 4, one float32 rounding of it 2.4e-7); the gradient of calculate_l1_loss against autograd, for a
    [B,1,H,W] and a [B,C,H,W] mask."""
    from omnifusion_amd.supervision.direct import calculate_l1_loss
    from omnifusion_amd.util import imgrad, imgrad_yx
    g = torch.Generator(device=DEV).manual_seed(1970)
    img = torch.rand(2, 3, 19, 70, device=DEV, generator=g)
    gy, gx = imgrad(img)
    ry, rx = gc.imgrad(img.double())
    assert gy.shape == (2, 1, 19, 70) and gy.dtype == torch.float32
    assert float((gy.double() - ry).abs().max()) <= 2e-6 and float((gx.double() - rx).abs().max()) <= 2e-6
    one = img[:, 1:2]                                                     # a non-contiguous single-channel view
    yx = imgrad_yx(one)
    assert yx.shape == (2, 2, 19, 70) and float((yx.double() - gc.imgrad_yx(one.double())).abs().max()) <= 2e-6
    with pytest.raises(ValueError, match="single-channel"):
        imgrad_yx(img)
    for mask_c in (1, 3):
        pred = torch.rand(2, 3, 19, 70, device=DEV, generator=g).requires_grad_(True)
        mask = torch.rand(2, mask_c, 19, 70, device=DEV, generator=g) < 0.7
        loss = calculate_l1_loss(pred, img, mask)
        grad, = torch.autograd.grad(loss, pred)
        p64 = pred.detach().double().requires_grad_(True)
        ref = gc.l1_loss(p64, img.double(), mask.double())                # the mask broadcasts; count is its sum as given, not multiplied by C
        g64, = torch.autograd.grad(ref, p64)
        assert abs(float(loss.detach()) - float(ref.detach())) <= 2e-6, (mask_c, float(loss.detach()), float(ref.detach()))
        assert float((grad.double() - g64).abs().max()) <= 1e-4 * float(g64.abs().max())


def test_single_term_entries_are_the_same_bits():
    """normal_loss / gradient_loss return the bits of geometry_terms; a backward through one output is that term's gradient, and the gradient of a
    weighted sum is the weighted sum of the gradients to round-off."""
    from omnifusion_amd.supervision import gradient_loss, normal_loss
    c = gc.case("G19c")
    n, g, gn, gg = grads(c)
    n1, p1 = run(c, normal_loss)
    g1, p2 = run(c, gradient_loss)
    assert torch.equal(n1, n) and torch.equal(g1, g)
    gn1, = torch.autograd.grad(n1, p1)
    gg1, = torch.autograd.grad(g1, p2)
    assert torch.equal(gn1, gn) and torch.equal(gg1, gg)
    (n2, g2), p3 = run(c)
    (0.2 * n2 + 0.05 * g2).backward()
    want = 0.2 * gn.double() + 0.05 * gg.double()
    # the weights enter the kernel's chain of about ten float32 operations at its start instead of multiplying its end: 16 ulp of the largest element
    assert float((p3.grad.double() - want).abs().max()) <= 16 * 2.0 ** -24 * float(want.abs().max())


def test_bitwise_repeatable_and_independent_of_workspace_contents():
    """Two runs give the same bits; so does a run whose workspace is a recycled block full of other values (the caching allocator hands the
    block of a freed tensor to the next request of its size)."""
    from omnifusion_amd import _lib
    c = gc.case("G19d")
    a = grads(c)
    b = grads(c)
    B, _, H, W = c["pred"].shape
    nbytes = _lib.load().omni_geometry_terms_workspace_bytes(B, H, W)
    for fill in (float("nan"), 1e30):
        junk = torch.full((nbytes // 8 + 1,), fill, dtype=torch.float64, device=DEV)
        del junk
        b2 = grads(c)
        assert all(torch.equal(x, y) for x, y in zip(a, b2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_directional_derivative():
    """(L(p + h v) - L(p - h v)) / 2h against <grad, v> on G19a for L = normal_loss + grad_loss, v smooth, h = 3e-3; tolerance: twice the residual the
    same check leaves on the reference's float32 run (recorded in the fixture)."""
    c, g = gc.case("G19a"), golden("G19a_geometry")
    n, gl, gn, gg = grads(c)

    def loss_of(pred):
        (a, b), _ = run(c, pred=pred)
        return float(a.detach()) + float(b.detach())
    res, fd, dot = gc.directional_residual(loss_of, gn.double().cpu().numpy() + gg.double().cpu().numpy(), c["pred"], gc.direction("G19a"), gc.DIRECTION_H)
    tol = 2 * float(g["ref32_direction_residual"])
    print(f"finite difference {fd:.8e}, <grad, v> {dot:.8e}, residual {res:.3e}, tolerance {tol:.3e}")
    assert res <= tol, (res, fd, dot)


def test_b3_crosses_over_channels():
    """B = 3 (where the reference crosses over the batch axis) against the float64 restatement on the device."""
    from omnifusion_amd.util import depth2normal_gpu
    c = gc.b3_case()
    r = gc.run_restatement(c, torch.float64, DEV)
    n, gl, gn, gg = grads(c)
    assert abs(float(n.detach()) - r["normal_loss"]) <= 2e-6 * max(1.0, abs(r["normal_loss"])) and abs(float(gl.detach()) - r["grad_loss"]) <= 2e-6 * max(1.0, abs(r["grad_loss"]))
    assert gc.rel_error(gn.cpu().numpy(), r["grad_normal"]).max() <= 1e-4 and gc.rel_error(gg.cpu().numpy(), r["grad_grad"]).max() <= 1e-4
    assert np.abs(depth2normal_gpu(t(c["pred"])).cpu().numpy() - r["normals"]).max() <= 1e-5


def test_mask_dtypes_and_layouts_give_the_same_bits():
    from omnifusion_amd.supervision import geometry_terms
    c = gc.case("G19c")
    a = grads(c)
    for mask in (t(c["mask"]).bool(), t(c["mask"]).to(torch.uint8), t(c["mask"]).double()):
        p = t(c["pred"]).requires_grad_(True)
        n, g = geometry_terms(p, t(c["gt"]), mask)
        assert torch.equal(n, a[0]) and torch.equal(g, a[1])
    wide = t(np.concatenate([c["pred"], c["pred"]], axis=3))
    p = wide[..., :c["pred"].shape[3]].requires_grad_(True)               # a non-contiguous pred, a transposed mask view
    assert not p.is_contiguous()
    n, g = geometry_terms(p, t(c["gt"]), t(np.ascontiguousarray(c["mask"].transpose(0, 1, 3, 2))).transpose(2, 3))
    gn, = torch.autograd.grad(n, p, retain_graph=True)
    gg, = torch.autograd.grad(g, p)
    assert all(torch.equal(x, y) for x, y in zip(a, (n, g, gn, gg)))


@pytest.mark.parametrize("name", ["G19a", "G19d"])
def test_erode_on_a_full_mask_changes_nothing(name):
    c = dict(gc.case(name), erode=False)
    c["mask"] = np.ones_like(c["mask"])
    a = grads(c)
    b = grads(dict(c, erode=True))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_erode_mask_is_the_eroded_mask():
    """erode_mask=True equals erode_mask=False on the mask eroded beforehand, bit for bit (G19e: holes in the ground truth)."""
    c = gc.case("G19e")
    a = grads(c)
    b = grads(dict(c, erode=False, mask=gc.eroded(torch.from_numpy(c["mask"])).numpy()))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_empty_masks_are_nan_and_bad_arguments_raise():
    """The empty-mask rule of calculate_berhu_loss (0 / 0): an item without valid pixels makes grad_loss NaN, a batch without any makes normal_loss NaN."""
    from omnifusion_amd.supervision import geometry_terms
    from omnifusion_amd.util import depth2normal_gpu
    c = gc.case("G19a")
    mask = c["mask"].copy()
    mask[1] = 0
    (n, g), p = run(dict(c, mask=mask))
    assert np.isfinite(float(n.detach())) and np.isnan(float(g.detach()))
    gn, = torch.autograd.grad(n, p)
    assert bool(torch.isfinite(gn).all()) and float(gn[1].abs().max()) == 0.0
    (n, g), _ = run(dict(c, mask=np.zeros_like(mask)))
    assert np.isnan(float(n.detach())) and np.isnan(float(g.detach()))
    with pytest.raises(NotImplementedError, match="H, W >= 2"):
        depth2normal_gpu(torch.ones(1, 1, 1, 8, device=DEV))
    with pytest.raises(ValueError, match="same shape"):
        geometry_terms(t(c["pred"]), t(c["gt"]), t(c["mask"])[:, :, :-1])
