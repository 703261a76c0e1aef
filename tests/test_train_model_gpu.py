"""GPU: the trainable spherical_fusion (omnifusion_amd/model/trainable.py) at the smallest size the architecture admits:
bs = 1, nrows = 3 — ten 128 x 128 patches of one 128 x 256 panorama — on make_state_dict(42, 10).

Eval parity: `.eval()` under no_grad against the inference spherical_fusion(precision="f16x3") on the same state dict, max|d| <= 1e-3 (the
project's parity gate).

Training forward: the (a, c) planes and every batch normalisation's updated running mean and variance against the float64 restatement
tests/_train_model_ref.py in training mode, fed the DEVICE's own patches.  Gate per tensor: max(8 . e32, 3e-5) on max|d| / max(1, rms), e32
the restatement's own float32 run; 3e-5 is CONV_GATE of test_conv_bwd_gpu.py, because the products are f16x3.

Gradients, from seeded grad_a and grad_c, for every parameter tensor: the relative L2 error err_k = |g - g64| / |g64|.  A max-norm gate
at 3e-5 cannot hold: about 2e7 ReLU inputs have density ~0.4 at zero, a pre-activation error d flips the mask of a fraction 0.8 d of them,
each flip changes a gradient discontinuously, and the expected relative L2 effect is about sqrt(0.8 d) whatever the size of the map.  So the
gate is measured from the reference alone: e_flip,k is the relative L2 distance between the float64 gradients and those of the same
restatement with every ReLU written relu(z + 3e-5) — which moves every activation CONV_GATE could move — and the device must satisfy
err_k <= 4 . max(e_flip,k, e32_k); the factor 4 allows a pre-activation error 16 times the shift, because the effect grows as the square
root.  This catches what the assembly can get wrong, each an O(0.1 - 1) error: a layout permutation, a missing skip or residual, a gradient
not summed over a tensor used twice, a broadcast reduced over the wrong axis.  Fine accuracy is the operator tests' business.

End to end: rgb -> model -> calculate_berhu_loss(mask, ones) -> backward -> AdamW(lr 1e-4, weight_decay 0.01).step(), ten times on one
fixed batch (seed 0: rgb uniform, gt = 1 + 3 . uniform, mask 90 % ones): every loss finite, the tenth below the first; the stepped
state_dict() then loads into the inference module and runs.  Whether the torch restatement itself meets this with that seed: see the
docstring of test_ten_adamw_steps_lower_the_loss.

Largest ratios measured on an MI355X: see DESIGN.md §23."""
import functools

import pytest
import torch

import _train_model_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS, NROWS, N, P, H, W = 1, 3, 10, 128, 128, 256
FOV = (80, 80)
CONV_GATE = 3e-5                                                                # tests/test_conv_bwd_gpu.py: the f16x3 products' gate
SHIFT = 3e-5
PARITY_GATE = 1e-3
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def nerr(got, want):
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def rel_l2(got, want):
    return ((got.double() - want.double()).norm() / want.double().norm()).item()


@functools.lru_cache(maxsize=None)
def case():
    from omnifusion_amd.weights import make_state_dict
    gen = torch.Generator().manual_seed(0)
    return {"sd": make_state_dict(42, N), "rgb": torch.rand(BS, 3, H, W, generator=gen),
            "ga": torch.randn(BS * N, 1, P, P, generator=gen), "gc": torch.randn(BS * N, 1, P, P, generator=gen)}


def device_model():
    from omnifusion_amd.model import trainable
    net = trainable.spherical_fusion(NROWS, N, (P, P), FOV)
    net.load_state_dict(case()["sd"])
    return net.to(DEV)


@functools.lru_cache(maxsize=None)
def device_patches():
    from omnifusion_amd import _lib
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
    return equi2pers_patches(case()["rgb"].to(DEV), FOV, NROWS, (P, P), layout=_lib.LAYOUT_BNCHW)


def param_names():
    return [k for k in case()["sd"] if k.rsplit(".", 1)[-1] not in _BUFFERS]


@functools.lru_cache(maxsize=None)
def restatement(dtype, shift):
    """(a, c), the updated running statistics and every parameter gradient of the restatement in training mode, on the CPU"""
    d = case()
    names = param_names()
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d["sd"].items()}
    for k in names:
        sd[k].requires_grad_(True)
    points_in = device_model().point_input("cpu").to(dtype)
    patches = device_patches().cpu().to(dtype).reshape(BS * N, 3, P, P)
    stats = {}
    pf = ref.mlp_points(sd, points_in, True, shift, stats)
    pred, weight = ref.network(sd, patches, pf, BS, N, True, shift, stats)
    a = pred * weight
    loss = (a * d["ga"].to(dtype)).sum() + (weight * d["gc"].to(dtype)).sum()
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    return {"a": a.detach(), "c": weight.detach(), "stats": stats, "grads": dict(zip(names, grads))}


def device_step():
    d = case()
    net = device_model()
    assert net.training
    a, c = net.network(device_patches(), net.mlp_points(net.point_input(DEV)), True)
    torch.autograd.backward([a, c], [d["ga"].to(DEV).reshape(a.shape), d["gc"].to(DEV).reshape(c.shape)])
    return {"a": a.detach().reshape(BS * N, 1, P, P).cpu(), "c": c.detach().reshape(BS * N, 1, P, P).cpu(),
            "stats": {k: v.cpu() for k, v in net.named_buffers() if not k.endswith("num_batches_tracked")},
            "tracked": {k: int(v) for k, v in net.named_buffers() if k.endswith("num_batches_tracked")},
            "grads": {k: (p.grad.cpu() if p.grad is not None else None) for k, p in net.named_parameters()}}


@functools.lru_cache(maxsize=None)
def device_result():
    return device_step()


def test_eval_parity_with_the_inference_module():
    from omnifusion_amd.model.spherical_model import spherical_fusion as inference_fusion
    d = case()
    net = device_model().eval()
    inf = inference_fusion(NROWS, N, (P, P), FOV, precision="f16x3")
    inf.load_state_dict(net.state_dict(), strict=True)
    inf = inf.to(DEV).eval()
    rgb = d["rgb"].to(DEV)
    for confidence in (True, False):
        with torch.no_grad():
            got, want = net(rgb, confidence=confidence), inf(rgb, confidence=confidence)
        e = (got - want).abs().max().item()
        print(f"train model eval parity, confidence={confidence}: max|d| = {e:.3e} (gate {PARITY_GATE:.0e}), max|want| = {want.abs().max().item():.3f}")
        assert got.shape == want.shape == (BS, 1, H, W) and not got.requires_grad and torch.isfinite(got).all() and e <= PARITY_GATE
    assert all(int(v) == 0 for k, v in net.named_buffers() if k.endswith("num_batches_tracked"))


def test_training_forward_against_float64():
    got, r64, r32 = device_result(), restatement(torch.float64, 0.0), restatement(torch.float32, 0.0)
    pairs = [("a", got["a"], r64["a"], r32["a"]), ("c", got["c"], r64["c"], r32["c"])]
    assert sorted(got["stats"]) == sorted(r64["stats"])
    pairs += [(k, got["stats"][k], r64["stats"][k], r32["stats"][k]) for k in r64["stats"]]
    worst = (0.0, None)
    for k, g, w64, w32 in pairs:
        gate = max(8.0 * nerr(w32, w64), CONV_GATE)
        e = nerr(g, w64)
        worst = max(worst, (e / gate, k))
        print(f"train model forward {k}: normalised error {e:.3e}  gate {gate:.3e}  ratio {e / gate:.3f}")
        assert g.shape == w64.shape and torch.isfinite(g).all() and e <= gate, f"{k}: {e:.3e} > {gate:.3e}"
    print(f"train model forward: largest ratio {worst[0]:.3f} ({worst[1]})")
    assert all(v == 1 for v in got["tracked"].values()) and len(got["tracked"]) == len(r64["stats"]) // 2
    sd = case()["sd"]
    assert any(not torch.equal(got["stats"][k], sd[k]) for k in got["stats"])


def test_every_parameter_gradient_against_float64():
    got = device_result()["grads"]
    g64, g32, gflip = (restatement(torch.float64, 0.0)["grads"], restatement(torch.float32, 0.0)["grads"],
                       restatement(torch.float64, SHIFT)["grads"])
    assert list(got) == param_names()
    worst, failed = (0.0, None), []
    for k, w in g64.items():
        g = got[k]
        assert g is not None and g.shape == w.shape and torch.isfinite(g).all(), f"{k}: no gradient, a wrong shape or a non-finite value"
        assert w.norm().item() > 0, k
        err, e_flip, e32 = rel_l2(g, w), rel_l2(gflip[k], w), rel_l2(g32[k], w)
        gate = 4.0 * max(e_flip, e32)
        worst = max(worst, (err / gate, k))
        print(f"train model gradient {k}: err {err:.3e}  e_flip {e_flip:.3e}  e32 {e32:.3e}  ratio {err / gate:.3f}")
        if not err <= gate:
            failed.append(f"{k}: {err:.3e} > {gate:.3e}")
    print(f"train model gradients: largest ratio {worst[0]:.3f} ({worst[1]})")
    assert not failed, failed


def test_two_identical_steps_give_the_same_bits():
    a, b = device_result(), device_step()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert torch.equal(a["a"], b["a"]) and torch.equal(a["c"], b["c"])
    for k in a["stats"]:
        assert torch.equal(a["stats"][k], b["stats"][k]), k


def test_ten_adamw_steps_lower_the_loss():
    """Confirmed first on the torch restatement (tests/_train_model_ref.py in float32 on an MI355X, blended by the differentiable pers2equi
    and a torch division, the same batch, seed and optimiser): its ten BerHu losses were 2.354615 2.115075 2.006027 1.925538 1.862327
    1.806829 1.756567 1.710194 1.667132 1.627229 — all finite, the tenth below the first.  The trainable model gave 2.354615 2.115048
    2.005976 1.925663 1.862567 1.807126 1.756981 1.710660 1.667656 1.627765 on the same box."""
    from omnifusion_amd.model.spherical_model import spherical_fusion as inference_fusion
    from omnifusion_amd.supervision.direct import calculate_berhu_loss
    gen = torch.Generator().manual_seed(0)
    rgb = torch.rand(BS, 3, H, W, generator=gen).to(DEV)
    gt = (1.0 + 3.0 * torch.rand(BS, 1, H, W, generator=gen)).to(DEV)
    mask = (torch.rand(BS, 1, H, W, generator=gen) < 0.9).float().to(DEV)
    net = device_model()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.01)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = calculate_berhu_loss(net(rgb, confidence=True), gt, mask, torch.ones_like(gt))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("train model ten AdamW steps, BerHu loss:", " ".join(f"{v:.6f}" for v in losses))
    assert all(map(lambda v: v == v and abs(v) != float("inf"), losses)) and losses[9] < losses[0]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    inf = inference_fusion(NROWS, N, (P, P), FOV)
    inf.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        out = inf.to(DEV).eval()(rgb, confidence=True)
    assert out.shape == (BS, 1, H, W) and torch.isfinite(out).all()
