"""The yardstick of tests/test_train_iterative_gpu.py: a plain-torch restatement of the ITERATIVE spherical_fusion
(model/spherical_model_iterative.py:308-457) over a state dict with the reference's iterative schema, in whatever dtype the state dict
has (the tests use float64), with TRAINING-mode batch normalisation and autograd through everything — the blend, the re-projection of the
previous depth and mlp_points2 included, so the loss of pass k reaches pass k - 1 as it does in the reference, which detaches nothing.

    r = forward(sd, patches, rays, iters, bs, nrows, erp_hw, confidence, training, relu_shift=0.0, depth_values=None)
    r["outs"]  the `iters` panorama maps [bs,1,H,W]      r["depth"]  the P/4 depth patches [bs.N,1,P/4,P/4] each later pass was fed
    r["stats"] the updated running statistics            r["tracked"] {batch norm: how many updates it took}

The network between the resamplers is tests/_train_model_ref._Net; new here are `down1`, mlp_points1 / mlp_points2 and the full-size
addition `layer1 + point_feat` of the later passes.  The resamplers are the float64-capable restatements of tests/_resample_cases.py
(equi2pers, pers2equi, conf_blend), which autograd differentiates.

Running statistics: _Net.bn reads them from the state dict it is given and leaves that dict unchanged, so they are THREADED here — pass k
runs on a copy of the dict in which pass k - 1's results stand, and the second update works on the first one's result, as the module's
buffers do.

depth_values[i] (optional, [bs.N,1,P/4,P/4]): the VALUES pass i + 2 is fed in place of the restatement's own re-projection, e.g. the
device's own patches — `own + (given - own).detach()`, so the graph, and with it the gradient through the feedback, stays the
restatement's."""
import torch
import torch.nn.functional as F

import _resample_cases as rc
from _train_model_ref import _Net, _LAYERS, _up

_STATS = ("running_mean", "running_var")


def point_mlp(sd, name, x, training, relu_shift=0.0, stats=None):
    """mlp_points1 / mlp_points2: 1x1 conv -> BN -> ReLU twice over x [M,3,P/4,P/4] (the batch statistics over all M maps)"""
    n = _Net(sd, training, relu_shift, stats)
    x = n.relu(n.bn(name + ".1", n.conv(name + ".0", x, 1, 0)))
    return n.relu(n.bn(name + ".4", n.conv(name + ".3", x, 1, 0)))


def network(sd, patches, point_feat, bs, n_patch, training, relu_shift=0.0, stats=None):
    """patches planar [bs.N,3,P,P]; point_feat [N,64,P/4,P/4] (broadcast over the batch) or [bs.N,64,P/4,P/4] -> (relu(pred), sigmoid(weight))"""
    n = _Net(sd, training, relu_shift, stats)
    M = bs * n_patch
    conv1 = n.relu(n.bn("bn1", n.conv("conv1", patches, 2, 3)))
    x = F.max_pool2d(conv1, 3, 2, 1)
    feats = {}
    for name, nblk, stride in _LAYERS:
        for b in range(nblk):
            x = n.block(f"{name}.{b}", x, stride if b == 0 else 1)
        if name == "layer1":
            x = x + (point_feat if point_feat.shape[0] == M else point_feat.repeat(bs, 1, 1, 1))
        feats[name] = x
    layer4 = feats["layer4"]
    tok = n.conv("down1", layer4, 1, 0).reshape(bs, n_patch, -1)
    layer4 = layer4 + n.transformer(tok).reshape(M, 512, 1, 1)
    x = n.cbr("de_conv0_1", torch.cat([n.cbr("de_conv0_0", _up(layer4)), feats["layer3"]], 1))
    x = n.cbr("de_conv1_1", torch.cat([n.cbr("de_conv1_0", _up(x)), feats["layer2"]], 1))
    x = n.cbr("de_conv2_1", torch.cat([n.cbr("de_conv2_0", _up(x)), feats["layer1"]], 1))
    x = n.cbr("de_conv3_1", torch.cat([n.cbr("de_conv3_0", _up(x)), conv1], 1))
    x = n.cbr("de_conv4_0", _up(x))
    return n.relu(n.conv("pred", x, 1, 1)), torch.sigmoid(n.conv("weight_pred", x, 1, 1))


def _to_ref(x, bs, n_patch):
    """[bs.N,1,P,P] -> the resamplers' [bs,1,P,P,N]"""
    return x.reshape(bs, n_patch, *x.shape[1:]).permute(0, 2, 3, 4, 1)


def _to_planar(x):
    """[bs,C,p,p,N] -> [bs.N,C,p,p]"""
    B, C, ph, pw, N = x.shape
    return x.permute(0, 4, 1, 2, 3).reshape(B * N, C, ph, pw)


def blend(pred, weight, confidence, bs, n_patch, tab):
    if confidence:
        return rc.conf_blend(_to_ref(pred * weight, bs, n_patch), _to_ref(weight, bs, n_patch), tab)
    return rc.pers2equi(_to_ref(pred, bs, n_patch), tab)


def forward(sd, patches, rays, iters, bs, nrows, erp_hw, confidence, training, relu_shift=0.0, depth_values=None, fov=rc.FOV):
    dtype = patches.dtype
    n_patch, P = rc.NPATCH[nrows], patches.shape[-1]
    tab = rc.p2e_tables(nrows, fov, (P, P), erp_hw, dtype)
    cur, stats, tracked, outs, fed = dict(sd), {}, {}, [], []

    def run(point_feat_of):
        s = {} if training else None
        pred, weight = network(cur, patches, point_feat_of(s), bs, n_patch, training, relu_shift, s)
        if training:
            cur.update(s); stats.update(s)
            for k in s:
                if k.endswith("running_mean"):
                    tracked[k[:-13]] = tracked.get(k[:-13], 0) + 1
        outs.append(blend(pred, weight, confidence, bs, n_patch, tab))

    run(lambda s: point_mlp(cur, "mlp_points1", rays, training, relu_shift, s))
    for i in range(iters - 1):
        depth = _to_planar(rc.equi2pers(outs[i], fov, nrows, (P // 4, P // 4), dtype=dtype))
        if depth_values is not None:
            depth = depth + (depth_values[i].to(dtype) - depth).detach()
        fed.append(depth)
        run(lambda s: point_mlp(cur, "mlp_points2", rays.repeat(bs, 1, 1, 1) * depth, training, relu_shift, s))
    return {"outs": outs, "depth": fed, "stats": stats, "tracked": tracked}
