"""GPU: the plane-fit normals (csrc/omni_planefit.hip) against the fixtures G22a-g — the reference's own float64 normals, loss and autograd
gradients (tools/gen_golden_planefit.py) — against stock float64 torch arithmetic on the device, the window's footprint through a NaN, a
directional derivative, the loss against its composition from two maps, and the bitwise properties: repeated runs, workspace contents, batch
items alone, mask dtypes, layouts and erode_mask on a full mask."""
import numpy as np
import pytest
import torch

import _planefit_cases as pc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -24


def t(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, **kw)


def normals_of(depth):
    from omnifusion_amd.equi_pers.depth2normal import depth2normal
    return depth2normal(depth)


def map_run(depth, U):
    """-> (normals, d sum(normals * U) / d depth) of depth2normal; depth and U are arrays or device tensors."""
    d = (depth if isinstance(depth, torch.Tensor) else t(depth)).detach().requires_grad_(True)
    out = normals_of(d)
    grad, = torch.autograd.grad((out * (U if isinstance(U, torch.Tensor) else t(U))).sum(), d)
    return out.detach(), grad


def loss_run(c, pred=None, mask=None, erode=None):
    """-> (loss, d loss / d pred) of planefit_normal_loss on the case."""
    from omnifusion_amd.supervision import planefit_normal_loss
    p = (t(c["pred"]) if pred is None else pred).detach().requires_grad_(True)
    l = planefit_normal_loss(p, t(c["gt"]), t(c["mask"]) if mask is None else mask, erode_mask=c["erode"] if erode is None else erode)
    grad, = torch.autograd.grad(l, p)
    return l.detach(), grad


def gate_normals(name, got, want, ref32, where=None):
    e = np.abs(got.cpu().numpy().astype(np.float64) - want)
    e = float((e if where is None else e[where]).max())
    gate = max(1e-5, 4 * ref32)
    print(f"{name} normals: max error {e:.2e} gate {gate:.1e} (reference float32: {ref32:.1e})")
    assert e <= gate, e


def gate_loss(name, got, want, ref32):
    e = abs(float(got) - want)
    gate = max(2e-6 * max(1.0, abs(want)), 4 * ref32)
    print(f"{name} loss: {float(got):.9f} against {want:.9f} error {e:.2e} gate {gate:.1e} (reference float32: {ref32:.1e})")
    assert e <= gate, e


def gate_grad(name, key, got, want, ref32):
    got = got.cpu().numpy()
    e = float(pc.rel_error(got, want).max())
    gate = max(1e-4, 4 * ref32)
    print(f"{name} {key}: max error {e:.2e} of the largest gradient, gate {gate:.1e} (reference float32: {ref32:.1e})")
    assert np.isfinite(got).all() and e <= gate, (key, e)


@pytest.mark.parametrize("name", pc.LOSS_NAMES)
def test_parity_with_reference(name):
    """The normals within max(1e-5, 4 x the reference's own float32 error) of the float64 golden, the loss within max(2e-6 max(1, |loss|), 4 x
    that error), both gradients finite and within max(1e-4, 4 x that error) of the largest reference gradient at every element."""
    c, g = pc.case(name), golden(name + "_planefit")
    out, grad_map = map_run(c["pred"], pc.upstream(name))
    assert out.shape == (c["pred"].shape[0], 3) + c["pred"].shape[2:] and out.dtype == torch.float32 and out.is_cuda
    l, grad_loss = loss_run(c)
    assert l.dtype == torch.float32 and l.dim() == 0 and l.is_cuda and grad_loss.shape == c["pred"].shape
    gate_normals(name, out, g["normals"].astype(np.float64), float(g["ref32_normals_err"]))
    gate_loss(name, l, float(g["loss"]), float(g["ref32_loss_err"]))
    gate_grad(name, "grad_map", grad_map, g["grad_map"], float(g["ref32_grad_map_max"]))
    gate_grad(name, "grad_loss", grad_loss, g["grad_loss"], float(g["ref32_grad_loss_max"]))


def test_determinants_straddling_the_threshold():
    """G22g: the determinants of a smooth field lie on both sides of 1e-5.  Outside the band of 1 % about the threshold (the fixture's float64
    determinants) the gate of the parity test holds at every pixel; inside, a pixel matches one of the two branches of the float64 restatement."""
    c, g = pc.case("G22g"), golden("G22g_planefit")
    out = normals_of(t(c["pred"]))
    near = pc.band(g["det"], pc.G_BAND)
    assert 0 < near.sum() == int(g["band_pixels"]) <= 0.01 * near.size
    print(f"G22g: {int(near.sum())} of {near.size} pixels within 1 % of the threshold are exempt; {int((g['det'] >= pc.DET_MIN).sum())} above it")
    where = np.broadcast_to(~near[:, None], out.shape)
    gate_normals("G22g", out, g["normals"].astype(np.float64), float(g["ref32_normals_err"]), where)
    d64 = torch.from_numpy(c["pred"]).double()
    gate = max(1e-5, 4 * float(g["ref32_normals_err"]))
    e = np.minimum(*[np.abs(out.cpu().numpy() - pc.normals(d64, branch).numpy()).max(axis=1) for branch in (True, False)])
    assert e[near].max() <= gate, e[near]


@pytest.mark.parametrize("where", ["interior", "corner"])
def test_window_footprint(where):
    """One NaN depth in G22c: NaN normals at exactly the centres at offsets {-4,-2,0,2,4}^2 inside the image — not at the odd offsets a dense
    9 x 9 window would cover — and the bits of the clean run everywhere else."""
    c = pc.case("G22c")
    B, _, H, W = c["pred"].shape
    b, i, j = (1, 9, 31) if where == "interior" else (0, 0, W - 1)
    clean = normals_of(t(c["pred"]))
    depth = c["pred"].copy()
    depth[b, 0, i, j] = np.nan
    got = normals_of(t(depth))
    want = np.zeros((B, H, W), bool)
    for a in pc.OFFSETS:
        for e in pc.OFFSETS:
            if 0 <= i + a < H and 0 <= j + e < W:
                want[b, i + a, j + e] = True
    assert want.sum() == (25 if where == "interior" else 9)
    nan = torch.isnan(got).cpu().numpy()
    assert np.array_equal(nan.all(axis=1), want) and np.array_equal(nan.any(axis=1), want)
    keep = torch.from_numpy(np.broadcast_to(~want[:, None], nan.shape).copy()).to(DEV)
    assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("shape", [(3, 21, 70), (1, 9, 130)])
def test_against_float64_torch_on_the_device(shape):
    """Shapes in no fixture against the restatement in float64 on the device: the map, its gradient, the loss and its gradient, under the floors of
    the parity gates alone."""
    B, H, W = shape
    gt = 2.5 + 1.5 * pc.smooth_field(2270 + H, B, H, W)
    pred = (gt + 0.2 * pc.smooth_field(2271 + H, B, H, W)).astype(np.float32)
    rng = np.random.default_rng(2272 + H)
    c = dict(pred=pred, gt=gt.astype(np.float32), mask=(rng.random((B, 1, H, W)) < 0.8).astype(np.float32), erode=False)
    U = (rng.random((B, 3, H, W)) * 2 - 1).astype(np.float32)
    p64 = t(pred).double().requires_grad_(True)
    want = pc.normals(p64)
    want_map, = torch.autograd.grad((want * t(U).double()).sum(), p64, retain_graph=True)
    want_l = pc.loss_of_normals(want, pc.normals(t(c["gt"]).double()), t(c["mask"]))
    want_loss, = torch.autograd.grad(want_l, p64)
    out, grad_map = map_run(pred, U)
    l, grad_loss = loss_run(c)
    gate_normals(str(shape), out, want.detach().cpu().numpy(), 0.0)
    gate_loss(str(shape), l, float(want_l.detach()), 0.0)
    gate_grad(str(shape), "grad_map", grad_map, want_map.cpu().numpy(), 0.0)
    gate_grad(str(shape), "grad_loss", grad_loss, want_loss.cpu().numpy(), 0.0)


def test_bitwise_repeatable_and_independent_of_workspace_contents():
    """Two runs give the same bits, forward and backward; so does a run whose workspace is a recycled block full of other values (the caching
    allocator hands the block of a freed tensor to the next request of its size)."""
    from omnifusion_amd import _lib
    c = pc.case("G22c")
    U = pc.upstream("G22c")
    run = lambda: map_run(c["pred"], U) + loss_run(c)
    a = run()
    b = run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    B, _, H, W = c["pred"].shape
    nbytes = _lib.load().omni_planefit_workspace_bytes(B, H, W)
    for fill in (float("nan"), 1e30):
        junk = torch.full((nbytes // 8 + 1,), fill, dtype=torch.float64, device=DEV)
        del junk
        assert all(torch.equal(x, y) for x, y in zip(a, run()))


def test_batch_items_alone_give_the_bits_of_the_batch():
    c = pc.case("G22c")
    U = pc.upstream("G22c")
    out, grad = map_run(c["pred"], U)
    for b in range(c["pred"].shape[0]):
        o1, g1 = map_run(c["pred"][b:b + 1], U[b:b + 1])
        assert torch.equal(o1, out[b:b + 1]) and torch.equal(g1, grad[b:b + 1])


@pytest.mark.parametrize("name", ["G22a", "G22e"])
def test_erode_on_a_full_mask_changes_nothing(name):
    c = pc.case(name)
    ones = t(np.ones_like(c["mask"]))
    a, b = loss_run(c, mask=ones, erode=False), loss_run(c, mask=ones, erode=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_erode_mask_is_the_eroded_mask():
    """erode_mask=True equals erode_mask=False on the mask eroded beforehand, bit for bit (G22e: holes in the ground truth)."""
    c = pc.case("G22e")
    a = loss_run(c)
    b = loss_run(c, mask=pc.eroded(t(c["mask"])), erode=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_mask_dtypes_and_layouts_give_the_same_bits():
    c = pc.case("G22c")
    a = loss_run(c)
    for mask in (t(c["mask"]).bool(), t(c["mask"]).to(torch.uint8), t(c["mask"]).double()):
        assert all(torch.equal(x, y) for x, y in zip(a, loss_run(c, mask=mask)))
    W = c["pred"].shape[3]
    wide = t(np.concatenate([c["pred"], c["pred"]], axis=3))
    p = wide[..., :W]                                                      # a non-contiguous pred, a transposed mask view
    assert not p.is_contiguous()
    b = loss_run(c, pred=p, mask=t(np.ascontiguousarray(c["mask"].transpose(0, 1, 3, 2))).transpose(2, 3))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    U = t(pc.upstream("G22c"))
    m1, m2 = map_run(t(c["pred"]), U), map_run(p, U)
    assert all(torch.equal(x, y) for x, y in zip(m1, m2))
    m3 = map_run(t(c["pred"]).double(), U)                                 # float64 input is converted
    assert m3[1].dtype == torch.float64 and all(torch.equal(x, y.float()) for x, y in zip(m1, m3))


def test_loss_is_the_composition_of_two_maps():
    """planefit_normal_loss against the formula applied in float64 to two depth2normal maps, <= 2e-6; its gradient against autograd through
    depth2normal (the formula in float64, the map's backward kernels), <= 16 ulp of the largest element: the fused backward forms the
    upstream in float64 where autograd rounds it to float32 once."""
    for name in ("G22a", "G22e"):
        c = pc.case(name)
        l, grad = loss_run(c)
        p = t(c["pred"]).requires_grad_(True)
        mask = t(c["mask"])
        want = pc.loss_of_normals(normals_of(p).double(), normals_of(t(c["gt"])).double(), (pc.eroded(mask) if c["erode"] else mask).double())
        want_grad, = torch.autograd.grad(want, p)
        e = float((grad.double() - want_grad.double()).abs().max())
        largest = float(want_grad.abs().max())
        print(f"{name}: loss {float(l):.9f} composed {float(want.detach()):.9f}; gradient error {e:.2e} = {e / (ULP * largest):.2f} ulp of the largest element {largest:.2e}")
        assert abs(float(l) - float(want.detach())) <= 2e-6
        assert e <= 16 * ULP * largest


def test_directional_derivative():
    """(L(p + h v) - L(p - h v)) against <grad, step> on G22a, v the main component of pred - gt, h = 3e-3; tolerance: max(1e-3, 4 x the residual
    the same check leaves on the reference's float32 run (recorded in the fixture))."""
    c, g = pc.case("G22a"), golden("G22a_planefit")
    _, grad = loss_run(c)
    res, fd, dot = pc.directional_residual(lambda pred: float(loss_run(c, pred=t(pred))[0]), grad.double().cpu().numpy(), c["pred"], pc.direction("G22a"), pc.DIRECTION_H)
    tol = max(1e-3, 4 * float(g["ref32_direction_residual"]))
    print(f"finite difference {fd:.8e}, <grad, v> {dot:.8e}, residual {res:.3e}, tolerance {tol:.3e} (reference float32 {float(g['ref32_direction_residual']):.2e}, "
          f"float64 {float(g['ref64_direction_residual']):.2e})")
    assert res <= tol, (res, fd, dot)


def test_degenerate_sizes_and_bad_arguments():
    """H = W = 1 and a single row: every window holds one row of vertices at most, M is singular and the normal is normalize(s)."""
    from omnifusion_amd.supervision import planefit_normal_loss
    for H, W in [(1, 1), (1, 70)]:
        d = torch.rand(2, 1, H, W, device=DEV) + 1
        out, grad = map_run(d, torch.ones(2, 3, H, W, device=DEV))
        assert float((out.double() - pc.normals(d.double())).abs().max()) <= 1e-5 and bool(torch.isfinite(grad).all())
    c = pc.case("G22a")
    l, grad = loss_run(c, mask=t(np.zeros_like(c["mask"])))
    assert np.isnan(float(l))                                             # an empty batch mask: 0 / 0, as normal_loss
    with pytest.raises(ValueError, match="same shape"):
        planefit_normal_loss(t(c["pred"]), t(c["gt"]), t(c["mask"])[:, :, :-1])
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        normals_of(torch.ones(1, 3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="floating-point"):
        normals_of(torch.ones(1, 1, 8, 8, device=DEV, dtype=torch.int32))
