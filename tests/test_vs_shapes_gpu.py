"""GPU: render / dibr_vertical / dibr_horizontal and the photometric loss (csrc/omni_dibr.hip, csrc/omni_photometric.hip), forward and
backward, against the float64 restatement (tests/_vs_restatement.py, proved on the CPU by tests/test_vs_restatement_cpu.py) at the
cases of tests/_vs_shape_cases.py: ragged images, images smaller than a tile, C = 1, 2, 4, 5, 8 (the C == 2 lane and the generic
record branch of the backward gather), the LDS window at and over equality, the 512 wrap inside the image, windows 3 - 11 of both
SSIM modes, channel-wise masks and weights, a fractional mask and the kink of the L1 term.  Through the public mirrors only.

Gates: none is new.  The ceiling of a quantity is the gate the existing tests apply to it (_vs_shape_cases.CEILING: recon 1e-4 with
at most 1e-3 of the elements over it and none over 1e-2, test_dibr_gpu.py; DIBR gradients 1e-4 of the largest float64 gradient with at
most 2e-4 of the elements over it and none over 1e-2, test_dibr_bwd_gpu.py; photometric loss 2e-6, gradient 1e-4 at every element,
SSIM map 2e-6, test_photometric_gpu.py).  Where the restatement's own float32 run is within half the ceiling of its float64 run at every
element (_vs_shape_cases.GAPS, measured on the CPU), the gate is twice that gap at every element instead — the margin
test_directional_derivative gives "the reference's own residual" — but never below 8 half-units of the last place of float32
(FORMAT_FLOOR).  E.g. recon of R1: gap 1.86e-7 -> gate 3.7e-7; depth gradient of V1: gap 3.5e-5 -> 7.0e-5; of Hz1: gap 7.8e-5, over
half the ceiling -> the ceiling; Hz2 (9 - 12 elements of the float32 run over 1e-4): the ceiling with its share."""
import numpy as np
import pytest
import torch

import _vs_shape_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def names_of(c):
    return ("img", "depth", "coords") if c["kind"] == "render" else ("img", "depth")


def run_dibr(c, need=None):
    """-> (recon, mask or None, dict of leaves) through the public mirrors; `need`: the names that require grad (default: all)."""
    from omnifusion_amd import spherical, util
    from omnifusion_amd.supervision.splatting import render
    names = names_of(c)
    need = names if need is None else need
    leaf = {k: (t(c[k]).requires_grad_(True) if k in need else t(c[k])) for k in names}
    if c["kind"] == "render":
        recon, mask = render(leaf["img"], leaf["depth"], leaf["coords"], max_depth=c["max_depth"])
        return recon, mask, leaf
    B, C, H, W = c["img"].shape
    uv, sg = spherical.create_image_grid(W, H, device=DEV), spherical.create_spherical_grid(W, device=DEV)
    fn = util.dibr_vertical if c["kind"] == "vertical" else util.dibr_horizontal
    return fn(leaf["depth"], leaf["img"], uv, sg, c["baseline"]), None, leaf


def grads_of(c, need=None):
    recon, _, leaf = run_dibr(c, need)
    recon.backward(t(c["grad_out"]))
    return recon.detach(), {k: (v.grad if v.requires_grad else None) for k, v in leaf.items()}


def gate(case, quantity, kind, err, scale=1.0):
    """Print the figures, then hold `err` (an array of errors, already in the gate's measure) to the gate of (case, quantity)."""
    tol, share, max_tol = sc.tolerance(case, quantity, kind, scale)
    over = int((err > tol).sum())
    print(f"VS {case} {quantity}: max {err.max():.3e}, over {tol:.2e}: {over} of {err.size} (allowed share {share:g}, bound {max_tol:.2e})")
    assert over <= share * err.size, (case, quantity, over, err.size, float(err.max()), np.argwhere(err > tol)[:4].tolist())
    assert err.max() <= max_tol, (case, quantity, float(err.max()), np.argwhere(err == err.max())[:4].tolist())


# ------------------------------------------------------------------ render / DIBR
@pytest.mark.parametrize("name", sc.DIBR_NAMES)
def test_forward_against_float64_restatement(name):
    """recon elementwise (gate: see the module docstring; the float32 gaps of recon are 6e-8 .. 4.5e-7 at every case but Hz1, 2.4e-6,
    and Hz2, which keeps the ceiling), mask flips 0 (MASK_FLIPS of test_dibr_gpu.py; the restatement's two precisions agree on every
    mask).  R3: recon is also the image shifted by (3, -2) wherever the source exists, and 0 with a clear mask elsewhere — no
    restatement involved; to FORMAT_FLOOR, since acc / wsum = (img w) / w leaves only the roundings."""
    c, ref = sc.dibr_case(name), sc.reference64(name)
    with torch.no_grad():
        recon, mask, _ = run_dibr(c, need=())
    got = recon.cpu().numpy()
    assert got.shape == ref["recon"].shape and np.isfinite(got).all()
    gate(name, "recon", "recon", np.abs(got.astype(np.float64) - ref["recon"]), scale=max(1.0, float(np.abs(ref["recon"]).max())))
    if mask is not None:
        flips = int((mask.cpu().numpy() != ref["mask"]).sum())
        print(f"VS {name} mask: flips {flips}")
        assert flips == 0
    if name == "R3":
        du, dv = sc.R3_SHIFT
        H, W = got.shape[-2:]
        want = np.zeros_like(got)
        want[..., :H + dv, du:] = c["img"][..., -dv:, :W - du]
        exists = np.zeros((H, W), bool)
        exists[:H + dv, du:] = True
        assert np.abs(got - want).max() <= sc.FORMAT_FLOOR and np.array_equal(mask.cpu().numpy()[:, 0], np.broadcast_to(exists, (got.shape[0], H, W)))
        assert (got[..., ~exists] == 0).all()


@pytest.mark.parametrize("name", sc.DIBR_NAMES)
def test_backward_against_float64_autograd(name):
    """Every gradient the mirror offers against float64 autograd of the restatement, relative to the largest float64 gradient of
    the tensor (R3's depth and coordinate gradients, exactly 0 in exact arithmetic: relative to the terms that cancel,
    _vs_shape_cases.gradient_scale).  Float32 gaps: image 6e-8 .. 1.9e-5, depth 5e-7 .. 7.8e-5, coordinates 1.6e-7 .. 2e-5 ->
    twice that; Hz1's depth gradient and all of Hz2 keep the ceiling.  Where stock autograd gives NaN — exactly the depth == 0 block
    of V2 / Hz1 — the device gives 0."""
    c, ref = sc.dibr_case(name), sc.reference64(name)
    _, got = grads_of(c)
    for k in names_of(c):
        mine, want = got[k].cpu().numpy(), ref["grad_" + k]
        assert mine.shape == want.shape and np.isfinite(mine).all(), (name, k)
        gate(name, "grad_" + k, "grad", sc.rel_error(name, k, mine, ref))
        bad = ~np.isfinite(want)
        if k == "depth" and c["kind"] != "render":
            assert np.array_equal(bad, c["depth"] == 0) and (mine[bad] == 0).all()
        else:
            assert not bad.any()


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_gradient_subsets_are_the_same_bits(name):
    """img only, depth only, coords only (null pointers for the others in the gather kernel): the one gradient asked for is the bits of
    the full backward, at C = 2 (the 16-byte record) and C = 4 (the generic record)."""
    c = sc.dibr_case(name)
    _, full = grads_of(c)
    for only in names_of(c):
        _, part = grads_of(c, need=(only,))
        for k in names_of(c):
            assert (part[k] is None) == (k != only), (name, only, k)
        assert torch.equal(part[only], full[only]), (name, only)


def _pair(c):
    """A batch of two distinct items from a one-item case (the second: another image, a deeper scene, the same targets)."""
    if c["img"].shape[0] > 1:
        return c
    second = dict(img=(0.1 + 0.5 * c["img"][:, ::-1]).astype(np.float32), depth=(c["depth"] + 0.75).astype(np.float32), coords=c["coords"],
                  grad_out=-c["grad_out"])
    return dict(c, **{k: np.ascontiguousarray(np.concatenate([c[k], second[k]], 0)) for k in second})


@pytest.mark.parametrize("name", ["R1", "R2", "R4"])
def test_bitwise_deterministic_and_batch_equals_items(name):
    """C = 2, 4, 8, forward and backward: two calls give the same bits, and a batch of two the bits of its items one at a time."""
    c = _pair(sc.dibr_case(name))
    ra, a = grads_of(c)
    rb, b = grads_of(c)
    assert torch.equal(ra, rb)
    for k in names_of(c):
        assert torch.equal(a[k], b[k]), k
    for i in range(c["img"].shape[0]):
        ci = dict(c, **{k: c[k][i:i + 1] for k in ("img", "depth", "coords", "grad_out")})
        ri, gi = grads_of(ci)
        assert torch.equal(ri, ra[i:i + 1]), i
        for k in names_of(c):
            assert torch.equal(gi[k], a[k][i:i + 1]), (k, i)


# ------------------------------------------------------------------ photometric loss
def loss_of(c, grad=True, sl=slice(None)):
    from omnifusion_amd.supervision.photometric import PhotometricLossParameters, calculate_loss
    p = t(c["pred"][sl]).requires_grad_(grad)
    params = PhotometricLossParameters(alpha=c["alpha"], window=c["window"], std=c["std"], ssim_mode=c["mode"])
    return calculate_loss(p, t(c["gt"][sl]), params, t(c["mask"][sl]), t(c["weights"][sl])), p


@pytest.mark.parametrize("name,alpha", [(n, 0.85) for n in sc.PHOTO_NAMES] + [("P6", 0.0), ("P6", 1.0)])
def test_photometric_against_float64_restatement(name, alpha):
    """Loss (ceiling 2e-6; float32 gaps 2e-9 .. 7.8e-8 -> twice that, not below FORMAT_FLOOR of the loss), gradient w.r.t. pred at every
    element (ceiling 1e-4 of the largest; gaps 6.8e-8 .. 2.9e-5 -> twice that) and the SSIM map of the masked images (2e-6: the gate
    between two float64 evaluations, never tightened — see test_float32_restatement_stays_inside_the_gates_photometric)."""
    from omnifusion_amd.supervision.ssim import ssim_loss
    c, ref = sc.photo_case(name, alpha), sc.reference64(name, alpha)
    loss, p = loss_of(c)
    loss.backward()
    assert loss.shape == () and torch.isfinite(p.grad).all()
    gate((name, alpha), "loss", "loss", np.array([abs(float(loss.item()) - ref["loss"])]), scale=abs(ref["loss"]))
    gate((name, alpha), "grad", "pgrad", np.abs(p.grad.cpu().numpy() - ref["grad"]) / np.abs(ref["grad"]).max())
    m = t(c["mask"])
    s = ssim_loss(t(c["pred"]) * m, t(c["gt"]) * m, kernel_size=c["window"], std=c["std"], mode=c["mode"])
    d = np.abs(s.cpu().numpy().astype(np.float64) - ref["ssim"])
    print(f"VS {(name, alpha)} ssim: max {d.max():.3e}")
    assert d.max() <= sc.CEILING["ssim"][0]
    assert (p.grad[(m == 0).expand_as(p.grad)] == 0).all()


def test_p6_equal_block_and_fractional_mask_reach_the_gradient():
    """What P6 is there for, stated on the restatement so that the parity test above means it: inside the 8 x 8 block pred == gt the L1
    term has no gradient (alpha = 0: the gradient there is exactly 0 on the device, as torch.abs' subgradient), and the half-valued
    mask pixels carry a gradient (so a missing mask factor shows: it would double them)."""
    c = sc.photo_case("P6", 0.0)
    loss, p = loss_of(c)
    loss.backward()
    g = p.grad.cpu().numpy()
    assert (g[sc.P6_EQUAL_BLOCK] == 0).all() and (sc.reference64("P6", 0.0)["grad"][sc.P6_EQUAL_BLOCK] == 0).all()
    half = np.broadcast_to(c["mask"] == 0.5, g.shape)
    assert half.sum() > 0.2 * g.size and (np.abs(g[half]) > 0).mean() > 0.9


def test_p6_empty_mask_item_is_nan_and_leaves_the_others_alone():
    """Forward only: with a third item whose mask is all zero the loss is NaN (0 / 0, as in the reference); that item alone is NaN; the
    other two alone give the terms they give inside P6 — the float32 mean of their float64 mean is P6's loss bit for bit."""
    c3, c = sc.p6_with_empty_item(), sc.photo_case("P6")
    with torch.no_grad():
        assert torch.isnan(loss_of(c3, grad=False)[0]) and torch.isnan(loss_of(c3, grad=False, sl=slice(2, 3))[0])
        items = [float(loss_of(c3, grad=False, sl=slice(i, i + 1))[0].item()) for i in range(2)]
        both = loss_of(c, grad=False)[0]
    assert np.isfinite(items).all() and np.float32(np.sum(np.asarray(items, np.float64)) / 2) == np.float32(both.item())
    assert np.isnan(sc.run_photo(c3, torch.float64, grad=False)["loss"])
