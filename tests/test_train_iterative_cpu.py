"""CPU: the trainable iterative spherical_fusion (omnifusion_amd/model/trainable_iterative.py) as a container — the
reference's iterative state-dict schema, the checkpoint round trip with the inference iterative module, its rejections — and the yardstick
of tests/test_train_iterative_gpu.py: the float64 restatement tests/_train_iterative_ref.py must equal, in eval mode, the restatement that
is already pinned against the reference's own goldens (oracle.model_ref.spherical_fusion_iterative_forward).  The forward itself needs the
GPU."""
import numpy as np
import pytest
import torch
from torch import nn

import _resample_cases as rc
from omnifusion_amd import ops
from omnifusion_amd.model import trainable, trainable_iterative
from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as inference_iterative
from omnifusion_amd.weights import make_state_dict, schema

NPATCH = {3: 10, 4: 18, 5: 26, 6: 46}
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def build(nrows):
    return trainable_iterative.spherical_fusion(nrows, NPATCH[nrows], (128, 128), (80, 80))


@pytest.mark.parametrize("nrows", list(NPATCH))
def test_parameters_and_buffers_are_the_reference_iterative_schema(nrows):
    net = build(nrows)
    assert isinstance(net, trainable.spherical_fusion) and net.training
    want = schema(NPATCH[nrows], iterative=True)
    got = net.state_dict()
    assert list(got) == list(want)                                             # same names, same ORDER
    for k, (shape, dtype) in want.items():
        assert tuple(got[k].shape) == tuple(shape) and str(got[k].dtype) == "torch." + dtype, k
    params, buffers = dict(net.named_parameters()), dict(net.named_buffers())
    assert sorted(list(params) + list(buffers)) == sorted(want)                # nothing else is registered
    assert all((k.rsplit(".", 1)[-1] in _BUFFERS) == (k in buffers) for k in want)
    assert all(p.requires_grad for p in params.values())
    assert "down1.weight" in got and "down.weight" not in got and "mlp_points.0.weight" not in got
    points = [m for m in net.modules() if isinstance(m, ops.PointConv2d)]
    assert len(points) == 4 and [tuple(m.weight.shape) for m in points] == [(16, 3, 1, 1), (64, 16, 1, 1)] * 2


def test_the_single_pass_module_keeps_its_schema():
    net = trainable.spherical_fusion(3, 10, (128, 128), (80, 80))
    assert list(net.state_dict()) == list(schema(10)) and not any(isinstance(m, ops.PointConv2d) for m in net.modules())


def test_checkpoints_move_between_the_iterative_modules():
    sd = make_state_dict(42, 18, True)
    net = build(4)
    out = net.load_state_dict(sd, strict=True)
    assert not out.missing_keys and not out.unexpected_keys
    back = net.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    inf = inference_iterative(4, 18, (128, 128), (80, 80))
    out = inf.load_state_dict(back, strict=True)
    assert not out.missing_keys and not out.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in inf.state_dict().items())
    net2 = build(4)
    net2.load_state_dict(inf.state_dict(), strict=True)                        # and back
    residue = {"module." + k: v for k, v in sd.items()}                        # a DataParallel checkpoint with the residue of thop
    residue["module.total_ops"], residue["module.conv1.total_params"] = torch.zeros(1), torch.zeros(1)
    net2.load_state_dict(residue, strict=True)
    assert torch.equal(net2.state_dict()["mlp_points2.3.weight"], sd["mlp_points2.3.weight"])
    with pytest.raises(RuntimeError):
        net2.load_state_dict(make_state_dict(42, 18, False), strict=True)      # the single pass's schema: down, mlp_points


def test_rejections():
    with pytest.raises(ValueError, match="token width is 512"):
        trainable_iterative.spherical_fusion()                                 # the reference's default, (256, 256)
    with pytest.raises(ValueError, match="token width is 512"):
        trainable_iterative.spherical_fusion(4, 18, (64, 64), (80, 80))
    with pytest.raises(ValueError, match="npatches does not match nrows"):
        trainable_iterative.spherical_fusion(4, 10, (128, 128), (80, 80))
    with pytest.raises(ValueError, match="presets"):
        trainable_iterative.spherical_fusion(7, 18, (128, 128), (80, 80))
    net = build(3)
    with pytest.raises(ValueError, match="no CPU path"):
        net(torch.zeros(1, 3, 64, 128), 2)
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        net(torch.zeros(1, 1, 64, 128), 2)


class _Float64Resamplers:
    """oracle.c_oracle's three resamplers as oracle.model_ref calls them (numpy in, numpy out, the reference's [B,C,h,w,N]), computed by the
    float64 restatements of tests/_resample_cases.py; xyz is the C oracle's own, widened."""

    def __init__(self, co):
        self.co = co

    def equi2pers(self, erp, fov, nrows, patch_size, want_pers=True):
        pers = rc.equi2pers(torch.from_numpy(np.asarray(erp)), fov, nrows, patch_size).numpy() if want_pers else None
        xyz = self.co.equi2pers(np.zeros((1, 1, 2, 2), np.float32), fov, nrows, patch_size, want_pers=False)[1]
        return pers, xyz.astype(np.float64), None, None

    def pers2equi(self, pers, fov, nrows, patch_size, erp_size):
        return rc.pers2equi(torch.from_numpy(pers), rc.p2e_tables(nrows, fov, patch_size, erp_size)).numpy()

    def pers2equi_conf(self, pred_w, conf, fov, nrows, patch_size, erp_size):
        return rc.conf_blend(torch.from_numpy(pred_w), torch.from_numpy(conf), rc.p2e_tables(nrows, fov, patch_size, erp_size)).numpy()


@pytest.mark.parametrize("confidence", [False, True])
def test_restatement_equals_the_pinned_one_in_eval_mode(confidence, monkeypatch):
    """tests/_train_iterative_ref.forward (training flag off, no ReLU shift, two passes) against
    oracle.model_ref.spherical_fusion_iterative_forward on make_state_dict(42, 10, True), one random 64 x 128 panorama, all in float64: the
    oracle's resamplers are float32 C, so for this comparison they are replaced by the float64 restatements of tests/_resample_cases.py
    (themselves pinned against the reference's goldens by tests/test_resample_restatement_cpu.py) — what is tied here is the assembly: the
    network under `down1`, mlp_points1 / mlp_points2, the rays times the depth, the full-size addition, the layouts around the blend and
    the loop.  Gate 1e-10 relative on both maps, the tie of tests/test_train_model_cpu.py.  Measured: see DESIGN.md §25."""
    from oracle import model_ref
    import _train_iterative_ref as ref
    shim = _Float64Resamplers(model_ref.co)
    monkeypatch.setattr(model_ref, "co", shim)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in make_state_dict(42, 10, True).items()}
    gen = torch.Generator().manual_seed(0)
    rgb = torch.rand(1, 3, 64, 128, generator=gen, dtype=torch.float64)
    want = model_ref.spherical_fusion_iterative_forward(sd, rgb, 2, nrows=3, patch_size=128, fov=(80, 80), confidence=confidence)
    rays = torch.from_numpy(shim.equi2pers(None, (80, 80), 3, (32, 32), want_pers=False)[1])
    patches = ref._to_planar(rc.equi2pers(rgb, (80, 80), 3, (128, 128)))
    with torch.no_grad():
        got = ref.forward(sd, patches, rays, 2, 1, 3, (64, 128), confidence, training=False)
    assert len(want) == len(got["outs"]) == 2 and not got["stats"] and not got["tracked"]
    for k, (g, w) in enumerate(zip(got["outs"], want)):
        e = ((g - w).abs().max() / w.abs().max()).item()
        print(f"iterative restatement against oracle.model_ref, confidence={confidence}, pass {k + 1}: {e:.3e} relative")
        assert g.shape == w.shape == (1, 1, 64, 128) and g.dtype == w.dtype == torch.float64 and w.abs().max() > 0 and e <= 1e-10
    assert (got["outs"][0] - got["outs"][1]).abs().max() > 1e-6                # the feedback does something
