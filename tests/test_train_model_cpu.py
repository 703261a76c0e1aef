"""CPU: the trainable spherical_fusion (omnifusion_amd/model/trainable.py) as a container — the reference's state-dict
schema, the checkpoint round trip with the inference module, the constants of its layers, its rejections — and the yardstick of
tests/test_train_model_gpu.py: the float64 training restatement tests/_train_model_ref.py must equal, in eval mode, the restatement that is
already pinned against the reference's own goldens (oracle.model_ref._network).  The forward itself needs the GPU."""
import pytest
import torch
from torch import nn

from omnifusion_amd import ops
from omnifusion_amd.model import trainable
from omnifusion_amd.model.spherical_model import spherical_fusion as inference_fusion
from omnifusion_amd.weights import make_state_dict, schema

NPATCH = {3: 10, 4: 18, 5: 26, 6: 46}
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def build(nrows):
    return trainable.spherical_fusion(nrows, NPATCH[nrows], (128, 128), (80, 80))


@pytest.mark.parametrize("nrows", list(NPATCH))
def test_parameters_and_buffers_are_the_reference_schema(nrows):
    net = build(nrows)
    assert isinstance(net, nn.Module) and net.training
    want = schema(NPATCH[nrows])
    got = net.state_dict()
    assert list(got) == list(want)                                             # same names, same ORDER
    for k, (shape, dtype) in want.items():
        assert tuple(got[k].shape) == tuple(shape) and str(got[k].dtype) == "torch." + dtype, k
    params, buffers = dict(net.named_parameters()), dict(net.named_buffers())
    assert sorted(list(params) + list(buffers)) == sorted(want)                # nothing else is registered
    assert all((k.rsplit(".", 1)[-1] in _BUFFERS) == (k in buffers) for k in want)
    assert all(p.requires_grad for p in params.values())


def test_checkpoints_move_between_the_modules():
    sd = make_state_dict(42, 18)
    net = build(4)
    out = net.load_state_dict(sd, strict=True)
    assert not out.missing_keys and not out.unexpected_keys
    back = net.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    inf = inference_fusion(4, 18, (128, 128), (80, 80))
    out = inf.load_state_dict(back, strict=True)
    assert not out.missing_keys and not out.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in inf.state_dict().items())
    # what the inference module accepts: the 'module.' prefix of a DataParallel checkpoint and the residue of thop
    residue = {"module." + k: v for k, v in sd.items()}
    residue["module.total_ops"], residue["module.conv1.total_params"] = torch.zeros(1), torch.zeros(1)
    net2 = build(4)
    net2.load_state_dict(residue, strict=True)
    assert torch.equal(net2.state_dict()["pred.bias"], sd["pred.bias"])
    with pytest.raises(RuntimeError):
        net2.load_state_dict({k: v for k, v in sd.items() if k != "pred.bias"}, strict=True)


def test_layer_constants():
    net = build(3)
    norms = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(norms) == 1 + 32 + 3 + 9 + 2                                    # bn1, 16 blocks x 2, the downsamples of layer2-4, the decoder, mlp_points
    assert all(m.eps == 1e-5 and m.momentum == 0.1 for m in norms)
    assert all(isinstance(m, ops.BatchNorm2d) for m in norms)
    assert net.transformer.encoder_norm.eps == 1e-6
    assert all(b.norm1.eps == 1e-5 and b.norm2.eps == 1e-5 for b in net.transformer.layer) and len(net.transformer.layer) == 6
    assert tuple(net.pred.weight.shape) == (1, 32, 3, 3, 1) and tuple(net.down.weight.shape) == (32, 512, 1, 1, 1)
    assert tuple(net.point_input("cpu").shape) == (10, 5, 32, 32)
    x = net.point_input("cpu")
    assert torch.equal(x[:, 0], x[:, 3]) and torch.equal(x[:, 1], x[:, 4]) and (x[:, 2] == 1).all() and (x[:, :, :1, :1] == x).all()


def test_rejections():
    with pytest.raises(ValueError, match="token width is 512"):
        trainable.spherical_fusion(4, 18, (64, 64), (80, 80))
    with pytest.raises(ValueError, match="token width is 512"):
        trainable.spherical_fusion(4, 18, (128, 256), (80, 80))
    with pytest.raises(ValueError, match="npatches does not match nrows"):
        trainable.spherical_fusion(4, 10, (128, 128), (80, 80))
    with pytest.raises(ValueError, match="presets"):
        trainable.spherical_fusion(7, 18, (128, 128), (80, 80))
    net = build(3)
    with pytest.raises(ValueError, match="no CPU path"):
        net(torch.zeros(1, 3, 128, 256))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        net(torch.zeros(1, 1, 128, 256))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.depth_heads(torch.zeros(1, 32, 4, 4), torch.zeros(1, 32, 3, 3), torch.zeros(1), torch.zeros(1, 32, 3, 3), torch.zeros(1))


def test_restatement_equals_the_pinned_one_in_eval_mode():
    """tests/_train_model_ref.py (training flag off, no ReLU shift) against oracle.model_ref._network on make_state_dict(42, 10), ten random
    128 x 128 patches, float64: 1e-10 relative."""
    from oracle import model_ref
    import _train_model_ref as ref
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in make_state_dict(42, 10).items()}
    gen = torch.Generator().manual_seed(0)
    patches = torch.rand(10, 3, 128, 128, generator=gen, dtype=torch.float64)
    points_in = build(3).point_input("cpu").double()
    with torch.no_grad():
        pf = ref.mlp_points(sd, points_in, training=False)
        assert torch.equal(pf, model_ref._mlp_points(sd, "mlp_points", points_in))
        pred, weight = ref.network(sd, patches, pf, 1, 10, training=False)
        want_pred, want_weight = model_ref._network(sd, patches, pf, 1, 10, 128, model_ref._Q(False), "down")
    for got, want, name in ((pred, want_pred, "pred"), (weight, want_weight, "weight")):
        e = ((got - want).abs().max() / want.abs().max()).item()
        print(f"restatement against oracle.model_ref._network, {name}: {e:.3e} relative")
        assert got.shape == want.shape and want.abs().max() > 0 and e <= 1e-10
    assert (pred > 0).any() and (pred == 0).any()
