"""GPU: supervision.photometric.calculate_loss and supervision.ssim.ssim_loss (csrc/omni_photometric.hip) against the reference's own
float64 loss and autograd (G16a-c, tools/gen_golden_photometric.py), a directional derivative, and bitwise determinism."""
import numpy as np
import pytest
import torch

import _vs_cases as vc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def loss_of(c, pred=None, grad=True, sl=slice(None)):
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    p = t((c["pred"] if pred is None else pred)[sl]).requires_grad_(grad)
    params = PhotometricLossParameters(alpha=c["alpha"], window=c["window"], std=c["std"], ssim_mode=c["mode"])
    return calculate_loss(p, t(c["gt"][sl]), params, t(c["mask"][sl]), t(c["weights"][sl])), p


@pytest.mark.parametrize("name", vc.PHOTO_NAMES)
def test_parity_with_reference(name):
    """Loss within 2e-6 of the float64 golden; gradient within 1e-4 of the largest reference gradient at every element (the reference's
    own float32 run: 4.5e-8 / 2.1e-5, 7.8e-9 / 2.9e-5, 4.7e-8 / 3.6e-5 on G16a / b / c)."""
    c = vc.photo_case(name)
    g = golden(name + "_photometric")
    loss, p = loss_of(c)
    loss.backward()
    e = vc.rel_error(p.grad.cpu().numpy(), g["grad"])
    print(f"{name}: loss {loss.item():.9f} golden {float(g['loss']):.9f} |d| {abs(loss.item() - float(g['loss'])):.2e}; grad max rel {e.max():.2e}")
    assert loss.shape == () and abs(loss.item() - float(g["loss"])) <= 2e-6
    assert e.max() <= 1e-4, float(e.max())


@pytest.mark.parametrize("name", vc.PHOTO_NAMES)
def test_ssim_map_against_torch(name):
    """ssim_loss against the same arithmetic in stock float64 torch ops (conv2d / avg_pool2d), on the masked images of the fixture."""
    import math
    import torch.nn.functional as F
    from omnifusion_amd.supervision.ssim import ssim_loss
    c = vc.photo_case(name)
    x, y = t(c["pred"]) * t(c["mask"]), t(c["gt"]) * t(c["mask"])
    k, r = c["window"], c["window"] // 2
    got = ssim_loss(x, y, kernel_size=k, std=c["std"], mode=c["mode"])
    xd, yd = x.double(), y.double()
    if c["mode"] == "gaussian":
        g1 = torch.tensor([math.exp(-(i - r) ** 2 / float(2 * c["std"] ** 2)) for i in range(k)], dtype=torch.float64)
        g1 = (g1 / g1.sum()).float().double()
        K = torch.outer(g1, g1)[None, None].repeat(3, 1, 1, 1).to(DEV)
        win = lambda z: F.conv2d(z, K, padding=r, groups=3)
    else:
        win = lambda z: F.avg_pool2d(z, k, stride=1)
    mx, my = win(xd), win(yd)
    sxx, syy, sxy = win(xd * xd) - mx * mx, win(yd * yd) - my * my, win(xd * yd) - mx * my
    want = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    if c["mode"] == "box":
        want = F.pad(want, (r, r, r, r))
    assert got.shape == want.shape and (got.double() - want).abs().max().item() <= 2e-6
    with pytest.raises(ValueError, match="forward only"):
        ssim_loss(x.clone().requires_grad_(True), y)


def test_directional_derivative():
    """(L(p + h v) - L(p - h v)) / 2h against <grad, v> for a smooth v on G16a's inputs, h = 3e-3.  The same check on the reference's
    float32 loss on the CPU leaves a relative residual of 7.2e-4 (it falls linearly with h: the kinks of |gt - pred|); tolerance: twice
    that, 1.44e-3."""
    c = vc.photo_case("G16a")
    v = dict(pred=(vc.smooth_erp(1521, *c["pred"].shape) - 0.5).astype(np.float32))
    loss, p = loss_of(c)
    loss.backward()

    def f(x):
        with torch.no_grad():
            return float(loss_of(c, pred=x["pred"], grad=False)[0].double())
    res, fd, dot = vc.directional_residual(f, dict(pred=p.grad.cpu().numpy()), c, v, 3e-3)
    print(f"finite difference {fd:.8e}, <grad, v> {dot:.8e}, residual {res:.3e}")
    assert res <= 1.44e-3, (res, fd, dot)


def _case4():
    from _util import rng_uniform, smooth_erp
    B, C, H, W = 4, 3, 96, 160                                       # not a multiple of the 16 x 32 tile in either direction... 160 = 5 x 32
    gt = (0.2 + 0.6 * smooth_erp(1531, B, C, H, W, k=9)).astype(np.float32)
    pred = (gt + 0.1 * (smooth_erp(1532, B, C, H, W) - 0.5) + 0.05 * (rng_uniform(1533, (B, C, H, W)) - 0.5)).astype(np.float32)
    mask = (rng_uniform(1534, (B, 1, H, W)) < 0.8).astype(np.float32)
    weights = (0.5 + smooth_erp(1535, B, C, H, W)).astype(np.float32)            # [B,C,H,W] weights
    return dict(pred=pred[..., :90, :150].copy(), gt=gt[..., :90, :150].copy(), mask=mask[..., :90, :150].copy(),
                weights=weights[..., :90, :150].copy(), window=7, std=1.5, mode="gaussian", alpha=0.85)


@pytest.mark.parametrize("mode,window", [("gaussian", 7), ("box", 5), ("gaussian", 11)])
def test_bitwise_deterministic_graph_and_batch_split(mode, window):
    c = dict(_case4(), mode=mode, window=window)
    B = c["pred"].shape[0]
    la, pa = loss_of(c)
    la.backward()
    lb, pb = loss_of(c)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(pa.grad, pb.grad) and torch.isfinite(pa.grad).all()
    items = []
    for i in range(B):
        li, pi = loss_of(c, sl=slice(i, i + 1))
        li.backward()
        items.append(li.item())
        assert torch.equal(pi.grad * (1.0 / B), pa.grad[i:i + 1]), i          # B = 4: the batch mean's 1/B is an exact scaling
    # per-item terms bit for bit; the batch mean is one more rounding of their float64 mean
    assert np.float32(np.sum(np.asarray(items, np.float64)) / B) == np.float32(la.item())
    # capture forward + backward, replay twice
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    p = t(c["pred"]).requires_grad_(True)
    gt, m, w = t(c["gt"]), t(c["mask"]), t(c["weights"])
    params = PhotometricLossParameters(window=window, ssim_mode=mode)

    def step():
        loss = calculate_loss(p, gt, params, m, w)
        return loss, torch.autograd.grad(loss, p)[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step()
    for _ in range(2):
        loss.zero_(); grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, la.detach()) and torch.equal(grad, pa.grad)


def test_mask_shapes_gradient_gates_and_bad_arguments():
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    c = _case4()
    p, gt, m, w = t(c["pred"]).requires_grad_(True), t(c["gt"]).requires_grad_(True), t(c["mask"]), t(c["weights"])
    loss = calculate_loss(p, gt, PhotometricLossParameters(), m.bool(), w)              # a bool mask, as the reference's .type(gt.dtype)
    loss.backward()
    assert gt.grad is None                                                             # gt, mask and weights are constants of the backward
    assert (p.grad[(m == 0).expand_as(p)] == 0).all()                                  # a masked-out pixel gets no gradient
    # a [B,C,H,W] mask counts C times as many elements: the loss is a third of the [B,1,H,W] one's
    l3 = calculate_loss(p, gt, PhotometricLossParameters(), m.expand_as(p).contiguous(), w)
    assert abs(l3.item() * 3 - loss.item()) <= 1e-6
    with pytest.raises(ValueError):
        calculate_loss(p, gt[:, :2], PhotometricLossParameters(), m, w)
    with pytest.raises(ValueError):
        calculate_loss(p, gt, PhotometricLossParameters(), m[..., :8], w)
    with pytest.raises(ValueError):
        calculate_loss(p.double(), gt.double(), PhotometricLossParameters(), m, w)
    with pytest.raises(ValueError, match="fit"):
        calculate_loss(p[..., :4, :], gt[..., :4, :], PhotometricLossParameters(window=5, ssim_mode="box"), m[..., :4, :], w[..., :4, :])
