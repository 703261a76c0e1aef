"""GPU: the trainable ITERATIVE spherical_fusion (omnifusion_amd/model/trainable_iterative.py) at the smallest size the
architecture admits: iter = 2, bs = 1, nrows = 3 — ten 128 x 128 patches of one 64 x 128 panorama — on make_state_dict(42, 10, True).  The
golden test alone runs nrows = 4.

Eval parity, with and without confidence: `.eval()` under no_grad against tests/golden/G7_model_iterative (the reference's own two maps,
nrows 4) and against the inference iterative module (precision="f16x3") on the same state dict: max|d| <= 1e-3 on both maps.

Training forward: both panorama maps and every batch normalisation's running mean and variance after the forward against the float64
restatement tests/_train_iterative_ref.py in training mode, fed the DEVICE's own RGB patches and rays and — pass 2 — the VALUES of the
device's own P/4 depth patches (the graph behind them stays the restatement's).  Gate per tensor, that of test_train_model_gpu.py for the
same reason (the products are f16x3): max(8 . e32, 3e-5) on max|d| / max(1, rms), e32 the restatement's own float32 run.
num_batches_tracked: 2 on the shared layers, 1 on mlp_points1.* and mlp_points2.*.

Gradients of every parameter through the whole chain — both blends and the feedback out[0] -> equi2pers -> mlp_points2 -> pass 2 — from
loss = sum_k <out_k, g_k> with seeded g_k: relative L2 against the float64 restatement, gate 4 . max(e_flip, e32) with e_flip from the
restatement's own relu(z + 3e-5) run (the docstring of test_train_model_gpu.py derives it).  The feedback alone: with the loss on out[1]
only, mlp_points1.* are reached only through out[0] -> equi2pers -> mlp_points2 and must be non-zero inside the same gate; with the loss
on out[0] only, mlp_points2.* get nothing.

End to end: ten AdamW steps on the script's loss, sum_k berhu(out_k) / iter (train_erp_depth_iterative.py:268-279), see
test_ten_adamw_steps_lower_the_loss.

Largest ratios measured on an MI355X: see DESIGN.md §25."""
import functools

import numpy as np
import pytest
import torch

import _train_iterative_ref as ref
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS, NROWS, N, P, H, W, ITERS = 1, 3, 10, 128, 64, 128, 2
P4 = P // 4
FOV = (80, 80)
CONV_GATE = 3e-5                                                                # tests/test_conv_bwd_gpu.py: the f16x3 products' gate
SHIFT = 3e-5
PARITY_GATE = 1e-3
LOSSES = ("all", "second", "first")                                             # sum_k <out_k, g_k>; <out_1, g_1> alone; <out_0, g_0> alone
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
    return {"sd": make_state_dict(42, N, True), "rgb": torch.rand(BS, 3, H, W, generator=gen),
            "g": [torch.randn(BS, 1, H, W, generator=gen) for _ in range(ITERS)]}


def device_model(nrows=NROWS, npatches=N, sd=None):
    from omnifusion_amd.model import trainable_iterative
    net = trainable_iterative.spherical_fusion(nrows, npatches, (P, P), FOV)
    net.load_state_dict(case()["sd"] if sd is None else sd)
    return net.to(DEV)


@functools.lru_cache(maxsize=None)
def device_patches():
    from omnifusion_amd import _lib
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
    return equi2pers_patches(case()["rgb"].to(DEV), FOV, NROWS, (P, P), layout=_lib.LAYOUT_BNCHW)


def param_names():
    return [k for k in case()["sd"] if k.rsplit(".", 1)[-1] not in _BUFFERS]


def _losses(outs, g):
    first, second = (outs[0] * g[0]).sum(), (outs[1] * g[1]).sum()
    return {"all": first + second, "second": second, "first": first}


def device_step(which=LOSSES):
    from omnifusion_amd import _lib
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
    d = case()
    net = device_model()
    assert net.training
    outs = net(d["rgb"].to(DEV), ITERS, confidence=True)
    assert isinstance(outs, list) and len(outs) == ITERS and all(o.shape == (BS, 1, H, W) and o.requires_grad for o in outs)
    names, params = zip(*net.named_parameters())
    losses = _losses(outs, [g.to(DEV) for g in d["g"]])
    grads = {}
    for k in which:
        got = torch.autograd.grad(losses[k], params, retain_graph=True, allow_unused=True)
        grads[k] = {n: (g.cpu() if g is not None else None) for n, g in zip(names, got)}
    depth = equi2pers_patches(outs[0].detach(), FOV, NROWS, (P4, P4), layout=_lib.LAYOUT_BNCHW).reshape(BS * N, 1, P4, P4)
    return {"outs": [o.detach().cpu() for o in outs], "depth": depth.cpu(), "rays": net.rays(DEV).cpu(),
            "stats": {k: v.cpu() for k, v in net.named_buffers() if not k.endswith("num_batches_tracked")},
            "tracked": {k: int(v) for k, v in net.named_buffers() if k.endswith("num_batches_tracked")}, "grads": grads}


@functools.lru_cache(maxsize=None)
def device_result():
    return device_step()


@functools.lru_cache(maxsize=None)
def restatement(dtype, shift):
    """both maps, the updated running statistics and every parameter gradient under the three losses, of the restatement in training mode
    on the CPU, fed the device's patches, rays and depth values"""
    d, dev = case(), device_result()
    names = param_names()
    sd = {k: (v.to(dtype).clone() if v.is_floating_point() else v) for k, v in d["sd"].items()}      # (clone: float32 -> float32 is no copy)
    for k in names:
        sd[k].requires_grad_(True)
    patches = device_patches().cpu().to(dtype).reshape(BS * N, 3, P, P)
    r = ref.forward(sd, patches, dev["rays"].to(dtype), ITERS, BS, NROWS, (H, W), True, True, shift, depth_values=[dev["depth"]])
    losses = _losses(r["outs"], [g.to(dtype) for g in d["g"]])
    grads = {k: dict(zip(names, torch.autograd.grad(losses[k], [sd[n] for n in names], retain_graph=True, allow_unused=True))) for k in LOSSES}
    return {"outs": [o.detach() for o in r["outs"]], "stats": r["stats"], "tracked": r["tracked"], "grads": grads}


def test_eval_parity_with_the_reference_golden():
    from omnifusion_amd.weights import make_state_dict
    g = golden("G7_model_iterative")
    net = device_model(4, 18, make_state_dict(42, 18, True)).eval()
    rgb = torch.from_numpy(g["rgb"]).to(DEV)
    for confidence, keys in ((False, ("it0", "it1")), (True, ("it0_conf", "it1_conf"))):
        with torch.no_grad():
            outs = net(rgb, ITERS, confidence=confidence)
        assert len(outs) == ITERS
        for o, k in zip(outs, keys):
            e = np.abs(o.cpu().numpy() - g[k]).max()
            print(f"train iterative eval against the golden {k}: max|d| = {e:.3e} (gate {PARITY_GATE:.0e}), max|want| = {np.abs(g[k]).max():.3f}")
            assert o.shape == g[k].shape and not o.requires_grad and torch.isfinite(o).all() and e <= PARITY_GATE
    assert all(int(v) == 0 for k, v in net.named_buffers() if k.endswith("num_batches_tracked"))


def test_eval_parity_with_the_inference_module():
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as inference_iterative
    net = device_model().eval()
    inf = inference_iterative(NROWS, N, (P, P), FOV, precision="f16x3")
    inf.load_state_dict(net.state_dict(), strict=True)
    inf = inf.to(DEV).eval()
    rgb = case()["rgb"].to(DEV)
    for confidence in (False, True):
        with torch.no_grad():
            got, want = net(rgb, ITERS, confidence=confidence), inf(rgb, ITERS, confidence=confidence)
        for k, (a, b) in enumerate(zip(got, want)):
            e = (a - b).abs().max().item()
            print(f"train iterative eval parity, confidence={confidence}, pass {k + 1}: max|d| = {e:.3e} (gate {PARITY_GATE:.0e}), "
                  f"max|want| = {b.abs().max().item():.3f}")
            assert a.shape == b.shape == (BS, 1, H, W) and torch.isfinite(a).all() and e <= PARITY_GATE
        assert not torch.equal(got[0], got[1])


def test_training_forward_against_float64():
    got, r64, r32 = device_result(), restatement(torch.float64, 0.0), restatement(torch.float32, 0.0)
    pairs = [(f"out[{k}]", got["outs"][k], r64["outs"][k], r32["outs"][k]) for k in range(ITERS)]
    assert sorted(got["stats"]) == sorted(r64["stats"])
    pairs += [(k, got["stats"][k], r64["stats"][k], r32["stats"][k]) for k in r64["stats"]]
    worst, failed = (0.0, None), []
    for k, g, w64, w32 in pairs:
        gate = max(8.0 * nerr(w32, w64), CONV_GATE)
        e = nerr(g, w64)
        worst = max(worst, (e / gate, k))
        print(f"train iterative forward {k}: normalised error {e:.3e}  gate {gate:.3e}  ratio {e / gate:.3f}")
        assert g.shape == w64.shape and torch.isfinite(g).all(), k
        if not e <= gate:
            failed.append(f"{k}: {e:.3e} > {gate:.3e}")
    print(f"train iterative forward: largest ratio {worst[0]:.3f} ({worst[1]})")
    assert not failed, failed
    for k, v in got["tracked"].items():
        want = 1 if k.startswith("mlp_points") else ITERS
        assert v == want == r64["tracked"][k[:-len(".num_batches_tracked")]], f"{k}: {v}"
    assert len(got["tracked"]) == len(r64["stats"]) // 2
    sd = case()["sd"]
    assert all(not torch.equal(got["stats"][k], sd[k]) for k in got["stats"] if k.endswith("running_mean"))


def _check_gradients(which, names):
    got = device_result()["grads"][which]
    g64, g32, gflip = (restatement(torch.float64, 0.0)["grads"][which], restatement(torch.float32, 0.0)["grads"][which],
                       restatement(torch.float64, SHIFT)["grads"][which])
    worst, failed = (0.0, None), []
    for k in names:
        g, w = got[k], g64[k]
        assert g is not None and w is not None and g.shape == w.shape and torch.isfinite(g).all(), f"{k}: no gradient, a wrong shape or a non-finite value"
        assert w.norm().item() > 0 and g.norm().item() > 0, k
        err, e_flip, e32 = rel_l2(g, w), rel_l2(gflip[k], w), rel_l2(g32[k], w)
        gate = 4.0 * max(e_flip, e32)
        worst = max(worst, (err / gate, k))
        print(f"train iterative gradient ({which}) {k}: err {err:.3e}  e_flip {e_flip:.3e}  e32 {e32:.3e}  ratio {err / gate:.3f}")
        if not err <= gate:
            failed.append(f"{k}: {err:.3e} > {gate:.3e}")
    print(f"train iterative gradients ({which}): largest ratio {worst[0]:.3f} ({worst[1]})")
    assert not failed, failed


def test_every_parameter_gradient_against_float64():
    assert list(device_result()["grads"]["all"]) == param_names()
    _check_gradients("all", param_names())


def test_the_feedback_path_alone():
    names = param_names()
    first_mlp, second_mlp = [k for k in names if k.startswith("mlp_points1.")], [k for k in names if k.startswith("mlp_points2.")]
    assert len(first_mlp) == len(second_mlp) == 6
    _check_gradients("second", first_mlp)                                       # reached only through out[0] -> equi2pers -> mlp_points2
    got, g64 = device_result()["grads"]["first"], restatement(torch.float64, 0.0)["grads"]["first"]
    for k in second_mlp:                                                        # pass 1 never reads mlp_points2
        assert g64[k] is None and (got[k] is None or not got[k].any()), k
    assert all(got[k] is not None and got[k].any() for k in first_mlp)


def test_two_identical_steps_give_the_same_bits():
    a, b = device_result(), device_step(("all",))
    for k in a["grads"]["all"]:
        assert torch.equal(a["grads"]["all"][k], b["grads"]["all"][k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"])) and torch.equal(a["depth"], b["depth"])
    for k in a["stats"]:
        assert torch.equal(a["stats"][k], b["stats"][k]), k


def _batch(seed):
    gen = torch.Generator().manual_seed(seed)
    rgb = torch.rand(BS, 3, H, W, generator=gen)
    gt = 1.0 + 3.0 * torch.rand(BS, 1, H, W, generator=gen)
    mask = (torch.rand(BS, 1, H, W, generator=gen) < 0.9).float()
    return rgb, gt, mask


def torch_restatement_losses(seed=0, steps=10):
    """The ten losses of the float32 torch restatement on the CPU (no device involved: its own resamplers, rays from the float64 geometry
    rounded to float32), the same batch, loss and optimiser as test_ten_adamw_steps_lower_the_loss:
        python -c "import sys; sys.path.insert(0, 'tests'); import test_train_iterative_gpu as t; print(t.torch_restatement_losses())" """
    import _resample_cases as rc
    rgb, gt, mask = _batch(seed)
    sd = {k: v.clone() for k, v in case()["sd"].items()}
    params = [sd[k].requires_grad_(True) for k in param_names()]
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01)
    patches = ref._to_planar(rc.equi2pers(rgb, FOV, NROWS, (P, P), dtype=torch.float32))
    c = rc.e2p_coords(NROWS, FOV, (P4, P4), (H, W), torch.float64)
    rays = rc.xyz_of(c["lon"].contiguous(), c["lat"]).float()

    def berhu(pred):                                                           # supervision/direct.py:3-18 with weights = 1
        diff = (gt - pred).abs()
        c5 = diff.max().item() / 5
        loss = torch.where(diff <= c5, diff, (diff * diff + c5 * c5) / (2 * c5))
        return ((loss * mask).reshape(BS, -1).sum(1) / mask.reshape(BS, -1).sum(1)).mean()

    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        r = ref.forward(sd, patches, rays, ITERS, BS, NROWS, (H, W), False, True)
        with torch.no_grad():
            sd.update({k: v for k, v in r["stats"].items()})                   # the buffers move as the module's do
        loss = sum(berhu(o) for o in r["outs"]) / ITERS
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def test_ten_adamw_steps_lower_the_loss():
    """The script's step (train_erp_depth_iterative.py:259-279: network(rgb, iter=2), confidence left at its default False,
    loss = sum_k berhu(out_k, gt, mask, ones) / iter, AdamW lr 1e-4, weight decay 0.01) ten times on one fixed batch — seed 0: rgb uniform,
    gt = 1 + 3 . uniform, mask 90 % ones.  Every loss finite, the tenth below the first.

    Seed 0 was confirmed first on the torch restatement: torch_restatement_losses(0) above — tests/_train_iterative_ref.py in float32 on
    the CPU, its own resamplers, the same batch, loss and optimiser — gave the ten losses listed in DESIGN.md §25, all finite, the tenth
    below the first."""
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as inference_iterative
    from omnifusion_amd.supervision.direct import calculate_berhu_loss
    rgb, gt, mask = (t.to(DEV) for t in _batch(0))
    net = device_model()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.01)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        outs = net(rgb, iter=ITERS)
        loss = sum(calculate_berhu_loss(o, gt, mask, torch.ones_like(gt)) for o in outs) / ITERS
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("train iterative ten AdamW steps, BerHu loss:", " ".join(f"{v:.6f}" for v in losses))
    assert all(map(lambda v: v == v and abs(v) != float("inf"), losses)) and losses[9] < losses[0]
    live = [k for k, p in net.named_parameters() if p.grad is not None]
    assert set(param_names()) - set(live) == {"weight_pred.weight", "weight_pred.bias"}       # without confidence nothing reads weight_pred
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    assert all(int(v) == (10 if k.startswith("mlp_points") else 10 * ITERS) for k, v in net.named_buffers() if k.endswith("num_batches_tracked"))
    inf = inference_iterative(NROWS, N, (P, P), FOV)
    inf.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        outs = inf.to(DEV).eval()(rgb, ITERS, confidence=True)
    assert len(outs) == ITERS and all(o.shape == (BS, 1, H, W) and torch.isfinite(o).all() for o in outs)
