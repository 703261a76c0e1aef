"""GPU: the backward of render / dibr_vertical / dibr_horizontal (csrc/omni_dibr.hip, a gather) against the reference's own autograd
(G15a-e, tools/gen_golden_dibr_bwd.py), directional derivatives, bitwise determinism, and depth refinement by view synthesis."""
import numpy as np
import pytest
import torch

import _vs_cases as vc
from _util import golden, pin_outliers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# elements of a gradient over 1e-4 (relative to the largest reference gradient) from the reference's float64 autograd, measured on
# MI355X: sources whose corner set differs at the 1e-3 / floor steps because sin / cos / exp are another library's
GRAD_OUTLIERS = {("G15a", "img"): 0, ("G15a", "depth"): 0, ("G15a", "coords"): 0, ("G15b", "img"): 0, ("G15b", "depth"): 0,
                 ("G15c", "img"): 3, ("G15c", "depth"): 3, ("G15d", "img"): 0, ("G15d", "depth"): 3, ("G15e", "img"): 0, ("G15e", "depth"): 0}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_case(c, tensors=None, need=None, grids=None):
    """-> (recon, dict of leaves).  `need`: the names that require grad (default: all the operator differentiates)."""
    from omnifusion_amd import spherical, util
    from omnifusion_amd.supervision.splatting import render
    names = vc.dibr_grad_names(c)
    need = names if need is None else need
    src = dict(c, **(tensors or {}))
    leaf = {k: (t(src[k]).requires_grad_(True) if k in need else t(src[k])) for k in names}
    if c["kind"] == "render":
        return render(leaf["img"], leaf["depth"], leaf["coords"], max_depth=c["max_depth"])[0], leaf
    B, C, H, W = c["img"].shape
    uv, sg = grids if grids is not None else (spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV))
    fn = util.dibr_vertical if c["kind"] == "vertical" else util.dibr_horizontal
    return fn(leaf["depth"], leaf["img"], uv, sg, c["baseline"]), leaf


def grads_of(c, **kw):
    recon, leaf = run_case(c, **kw)
    recon.backward(t(c["grad_out"]))
    return {k: (v.grad if v.requires_grad else None) for k, v in leaf.items()}


@pytest.mark.parametrize("name", vc.DIBR_NAMES)
def test_parity_with_reference_autograd(name):
    """Per tensor: at most a share of 2e-4 of the elements over 1e-4, none over 1e-2 (the reference's own float32 run stays inside both,
    tests/test_view_synthesis_cpu.py); the counts over 1e-4 are pinned.  Where the reference's depth gradient is NaN — exactly the
    depth == 0 block — ours is exactly 0."""
    c = vc.dibr_case(name)
    g = golden(name + "_dibr_bwd")
    got = grads_of(c)
    for k in vc.dibr_grad_names(c):
        mine, want = got[k].cpu().numpy(), g["grad_" + k]
        assert mine.shape == want.shape and np.isfinite(mine).all(), (name, k)
        e = vc.rel_error(mine, want)
        print(f"{name} {k}: share over 1e-4 {(e > 1e-4).mean():.3e}, max {e.max():.3e}")
        pin_outliers((name, k), mine / np.abs(want[np.isfinite(want)]).max(), want / np.abs(want[np.isfinite(want)]).max(), 1e-4, GRAD_OUTLIERS)
        assert (e > 1e-4).mean() <= 2e-4, (name, k, float((e > 1e-4).mean()))
        assert e.max() <= 1e-2, (name, k, float(e.max()))
    if c["kind"] != "render":
        bad = ~np.isfinite(g["grad_depth"])
        assert np.array_equal(bad, c["depth"] == 0)
        assert (got["depth"].cpu().numpy()[bad] == 0).all()


@pytest.mark.parametrize("kind,h,tol", [("render", 1e-1, 1.13e-1), ("vertical", 1e-1, 7.9e-6), ("horizontal", 3e-2, 6.7e-1)])
def test_directional_derivative(kind, h, tol):
    """(L(x + h v) - L(x - h v)) / 2h against <grad, v> on smooth inputs, x = all differentiable inputs jointly, L = sum(recon * G)
    in float64 over the float32 result.  h and the tolerance are the reference's: the same check run on the reference's float32
    autograd on the CPU leaves a relative residual of 5.6e-2 (render, h = 1e-1), 3.9e-6 (vertical, h = 1e-1) and 3.3e-1 (horizontal,
    h = 3e-2); the tolerance is twice that.  The vertical mode is smooth in the depth; render moves coordinates across the
    1e-3 corner-weight step and the horizontal mode across its clamps, which a finite difference sees and autograd (rightly) does
    not — their residuals do not fall with h on the reference either (render 5.6e-2 .. 6.2e-1, horizontal 2.9e-1 .. 1.3e+1 over
    h = 1e-1 .. 1e-3), so those two bounds only catch a gradient of the wrong sign or scale."""
    c, v = vc.direction_case(kind)
    G = t(c["grad_out"]).double()
    grads = {k: g.cpu().numpy() for k, g in grads_of(c).items()}

    def loss_of(x):
        with torch.no_grad():
            return float((run_case(c, tensors=x, need=())[0].double() * G).sum())
    res, fd, dot = vc.directional_residual(loss_of, grads, c, v, h)
    print(f"{kind}: finite difference {fd:.8e}, <grad, v> {dot:.8e}, residual {res:.3e}")
    assert res <= tol, (kind, res, fd, dot)


def _batch4():
    import _dibr_cases as dc
    B, C, H, W = 4, 3, 128, 256
    img = dc.smooth_erp(1451, B, C, H, W)
    depth = dc.zero_block(dc.smooth_depth(1452, B, H, W))
    coords = (dc.image_grid(H, W) + 30.0 * (dc.smooth_erp(1453, B, 2, H, W) - 0.5)).astype(np.float32)
    return img, depth, coords, (dc.smooth_erp(77, B, C, H, W) - 0.5).astype(np.float32)


@pytest.mark.parametrize("kind", ["render", "vertical", "horizontal"])
def test_bitwise_deterministic_graph_and_batch_split(kind):
    img, depth, coords, G = _batch4()
    c = dict(kind=kind, img=img, depth=depth, coords=coords, grad_out=G, baseline=0.26, max_depth=8.0)
    names = vc.dibr_grad_names(c)
    a, b = grads_of(c), grads_of(c)
    for k in names:
        assert torch.equal(a[k], b[k]), k
    for i in range(img.shape[0]):
        ci = dict(c, **{k: c[k][i:i + 1] for k in ("img", "depth", "coords", "grad_out")})
        gi = grads_of(ci)
        for k in names:
            assert torch.equal(gi[k], a[k][i:i + 1]), (k, i)
    # capture forward + backward, replay twice
    from omnifusion_amd import spherical, util
    from omnifusion_amd.supervision.splatting import render
    B, C, H, W = img.shape
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    leaf = {k: t(c[k]).requires_grad_(True) for k in names}
    Gt = t(G)

    def step():
        if kind == "render":
            recon = render(leaf["img"], leaf["depth"], leaf["coords"], max_depth=8.0)[0]
        else:
            recon = (util.dibr_vertical if kind == "vertical" else util.dibr_horizontal)(leaf["depth"], leaf["img"], uv, sg, 0.26)
        return torch.autograd.grad(recon, [leaf[k] for k in names], Gt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, o in zip(names, outs):
            assert torch.equal(o, a[k]), k


def test_grid_batched_same_gradient_bits():
    from omnifusion_amd import spherical
    img, depth, coords, G = _batch4()
    B, C, H, W = img.shape
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    for kind in ("vertical", "horizontal"):
        c = dict(kind=kind, img=img, depth=depth, grad_out=G, baseline=0.26)
        a = grads_of(c, grids=(uv, sg))
        b = grads_of(c, grids=(uv.expand(B, 2, H, W).contiguous(), sg.expand(B, 2, H, W).contiguous()))
        assert torch.equal(a["img"], b["img"]) and torch.equal(a["depth"], b["depth"])


def test_only_requested_gradients_and_same_forward():
    from omnifusion_amd import spherical, util
    from omnifusion_amd.supervision.splatting import render
    img, depth, coords, G = _batch4()
    B, C, H, W = img.shape
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    full = {kind: grads_of(dict(kind=kind, img=img, depth=depth, coords=coords, grad_out=G, baseline=0.26, max_depth=8.0))
            for kind in ("render", "vertical")}
    for kind in ("render", "vertical"):
        c = dict(kind=kind, img=img, depth=depth, coords=coords, grad_out=G, baseline=0.26, max_depth=8.0)
        for only in vc.dibr_grad_names(c):
            recon, leaf = run_case(c, need=(only,))
            recon.backward(t(G))
            for k, v in leaf.items():
                assert (v.grad is None) == (k != only), (kind, only, k)
            assert torch.equal(leaf[only].grad, full[kind][only]), (kind, only)
    # mask: not differentiable; the forward with grad-requiring inputs is the inference forward, bit for bit
    i, d, co = t(img), t(depth), t(coords)
    r0, m0 = render(i, d, co, max_depth=8.0)
    r1, m1 = render(i.clone().requires_grad_(True), d, co, max_depth=8.0)
    assert r1.requires_grad and not m1.requires_grad and m1.dtype == torch.bool
    assert torch.equal(r0, r1.detach()) and torch.equal(m0, m1)
    for fn in (util.dibr_vertical, util.dibr_horizontal):
        assert torch.equal(fn(d, i, uv, sg, 0.26), fn(d.clone().requires_grad_(True), i, uv, sg, 0.26).detach())
    with torch.no_grad():
        assert not util.dibr_vertical(d.clone().requires_grad_(True), i, uv, sg, 0.26).requires_grad


def test_nonfinite_upstream_gradient_reaches_only_its_sources():
    """A NaN in dL/drecon at one target: exactly the sources with a surviving corner on that target get a NaN gradient."""
    from omnifusion_amd import spherical, util
    import _dibr_cases as dc
    B, C, H, W = 1, 3, 32, 64
    img, depth = t(dc.smooth_erp(1461, B, C, H, W)).requires_grad_(True), t(dc.smooth_depth(1462, B, H, W)).requires_grad_(True)
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    recon = util.dibr_vertical(depth, img, uv, sg, 0.0)                  # zero baseline: every source lands on itself
    G = torch.ones_like(recon)
    G[0, 1, 12, 40] = float("nan")
    recon.backward(G)
    want = np.zeros((H, W), bool)
    want[12, 40] = True
    assert np.array_equal(torch.isnan(img.grad).any(dim=1)[0].cpu().numpy(), want)
    assert np.array_equal(torch.isnan(depth.grad)[0, 0].cpu().numpy(), want)


def test_benchmark_size_zero_baseline_identity():
    """Zero baseline, vertical, B = 8 at 512 x 1024: the warp is the identity, so dL/dimage = G (to 1e-6)."""
    from omnifusion_amd import spherical, util
    B, C, H, W = 8, 3, 512, 1024
    g = torch.Generator(device=DEV).manual_seed(7)
    img = torch.rand(B, C, H, W, device=DEV, generator=g).requires_grad_(True)
    depth = (0.3 + 7.7 * torch.rand(B, 1, H, W, device=DEV, generator=g)).requires_grad_(True)
    G = torch.rand(B, C, H, W, device=DEV, generator=g) - 0.5
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    util.dibr_vertical(depth, img, uv, sg, 0.0).backward(G)
    assert (img.grad - G).abs().max().item() <= 1e-6
    assert torch.isfinite(depth.grad).all()


def test_depth_refinement_by_view_synthesis():
    """End to end at 128 x 256: the target view is dibr_vertical(true depth, image); from true * (1 + 0.15 * smooth noise), 30 Adam steps
    (lr 0.05) on the depth through dibr_vertical -> photometric.calculate_loss lower the loss.  The same loop on the reference on the
    CPU goes from 7.04e-4 to 4.98e-5 (0.071 of the initial loss; required of the reference: <= 0.7); here: <= 0.85 of the initial loss."""
    from omnifusion_amd import spherical, util
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    img, true, start = vc.e2e_case()
    B, C, H, W = img.shape
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    image = t(img)
    target = util.dibr_vertical(t(true), image, uv, sg, vc.E2E_BASELINE)
    ones = torch.ones(B, 1, H, W, device=DEV)
    d = t(start).requires_grad_(True)
    opt = torch.optim.Adam([d], lr=vc.E2E_LR)
    losses = []
    for i in range(vc.E2E_STEPS + 1):
        opt.zero_grad()
        loss = calculate_loss(util.dibr_vertical(d, image, uv, sg, vc.E2E_BASELINE), target, PhotometricLossParameters(), ones, ones)
        losses.append(loss.item())
        if i < vc.E2E_STEPS:
            loss.backward()
            opt.step()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e} ({losses[-1] / losses[0]:.3f})")
    assert np.isfinite(losses).all() and losses[-1] <= 0.85 * losses[0], losses
