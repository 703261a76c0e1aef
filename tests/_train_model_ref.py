"""The yardstick of tests/test_train_model_gpu.py: a plain-torch restatement of the network of spherical_fusion between the two resamplers
(model/spherical_model.py:250-306) over a state dict with the reference's schema, in whatever dtype the state dict has (the tests use
float64), with TRAINING-mode batch normalisation and autograd through everything.

    pf = mlp_points(sd, points_in, training, relu_shift=0.0, stats=None)          # [N,5,P/4,P/4] -> [N,64,P/4,P/4]
    pred, weight = network(sd, patches, pf, bs, n_patch, training, relu_shift=0.0, stats=None)

patches planar [bs.N,3,P,P]; pred = relu(pred(x)), weight = sigmoid(weight_pred(x)), both [bs.N,1,P,P] — the return of
oracle.model_ref._network, which this equals in eval mode (tests/test_train_model_cpu.py ties the two at 1e-10 in float64).  `training`:
batch statistics over [bs.N,P,P] (the reference's BatchNorm3d over [B,C,P,P,N]; mlp_points over its own [N,.,P/4,P/4]) with eps 1e-5; the
updated running statistics (momentum 0.1, unbiased variance) go to `stats` {name + ".running_mean" / ".running_var": tensor} and the
state dict is left unchanged.  `relu_shift`: every ReLU is written relu(z + relu_shift) — the gradient test measures with it how far a
pre-activation error of that size moves the gradients."""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
_LAYERS = (("layer1", 3, 1), ("layer2", 4, 2), ("layer3", 6, 2), ("layer4", 3, 2))


class _Net:
    def __init__(self, sd, training, relu_shift, stats):
        self.sd, self.training, self.shift, self.stats = sd, training, relu_shift, stats

    def relu(self, z):
        return F.relu(z + self.shift) if self.shift else F.relu(z)

    def conv(self, name, x, stride, pad):
        w = self.sd[name + ".weight"]
        return F.conv2d(x, w[..., 0] if w.dim() == 5 else w, self.sd.get(name + ".bias"), stride=stride, padding=pad)

    def bn(self, name, x):
        sd = self.sd
        rm, rv = sd[name + ".running_mean"].detach().clone(), sd[name + ".running_var"].detach().clone()
        y = F.batch_norm(x, rm, rv, sd[name + ".weight"], sd[name + ".bias"], self.training, BN_MOMENTUM, BN_EPS)
        if self.training and self.stats is not None:
            self.stats[name + ".running_mean"], self.stats[name + ".running_var"] = rm, rv
        return y

    def block(self, p, x, stride):
        out = self.relu(self.bn(p + ".bn1", self.conv(p + ".conv1", x, stride, 1)))
        out = self.bn(p + ".bn2", self.conv(p + ".conv2", out, 1, 1))
        if (p + ".downsample.0.weight") in self.sd:
            x = self.bn(p + ".downsample.1", self.conv(p + ".downsample.0", x, stride, 0))
        return self.relu(out + x)

    def cbr(self, name, x):
        return self.relu(self.bn(name + ".bn", self.conv(name + ".conv", x, 1, 1)))

    def attention(self, p, x):
        sd = self.sd
        B, N, C = x.shape
        h = 4
        q = F.linear(x, sd[p + ".q.weight"]).reshape(B, N, h, C // h).permute(0, 2, 1, 3)
        kv = F.linear(x, sd[p + ".kv.weight"]).reshape(B, N, 2, h, C // h).permute(2, 0, 3, 1, 4)
        attn = ((q @ kv[0].transpose(-2, -1)) * ((C // h) ** -0.5)).softmax(dim=-1)
        y = (attn @ kv[1]).transpose(1, 2).reshape(B, N, C)
        return F.linear(y, sd[p + ".proj.weight"], sd[p + ".proj.bias"])

    def transformer(self, x):
        sd = self.sd
        x = x + sd["transformer.pos_emb"]
        for i in range(6):
            p = f"transformer.layer.{i}"
            x = x + self.attention(p + ".attn", F.layer_norm(x, (512,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5))
            y = F.layer_norm(x, (512,), sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5)
            x = x + F.linear(F.gelu(F.linear(y, sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"])), sd[p + ".mlp.fc2.weight"],
                             sd[p + ".mlp.fc2.bias"])
        return F.layer_norm(x, (512,), sd["transformer.encoder_norm.weight"], sd["transformer.encoder_norm.bias"], 1e-6)


def _up(x):
    return F.interpolate(x, size=(2 * x.shape[-2], 2 * x.shape[-1]), mode="bilinear", align_corners=False)


def mlp_points(sd, points_in, training, relu_shift=0.0, stats=None):
    n = _Net(sd, training, relu_shift, stats)
    x = n.relu(n.bn("mlp_points.1", n.conv("mlp_points.0", points_in, 1, 0)))
    return n.relu(n.bn("mlp_points.4", n.conv("mlp_points.3", x, 1, 0)))


def network(sd, patches, point_feat, bs, n_patch, training, relu_shift=0.0, stats=None):
    n = _Net(sd, training, relu_shift, stats)
    M = bs * n_patch
    conv1 = n.relu(n.bn("bn1", n.conv("conv1", patches, 2, 3)))
    x = F.max_pool2d(conv1, 3, 2, 1)
    feats = {}
    for name, nblk, stride in _LAYERS:
        for b in range(nblk):
            x = n.block(f"{name}.{b}", x, stride if b == 0 else 1)
        if name == "layer1":
            x = (x.reshape(bs, n_patch, *x.shape[1:]) + point_feat[None]).reshape(x.shape)
        feats[name] = x
    layer4 = feats["layer4"]
    tok = n.conv("down", layer4, 1, 0).reshape(bs, n_patch, -1)                 # token element = c . 16 + h . 4 + w
    layer4 = layer4 + n.transformer(tok).reshape(M, 512, 1, 1)
    x = n.cbr("de_conv0_1", torch.cat([n.cbr("de_conv0_0", _up(layer4)), feats["layer3"]], 1))
    x = n.cbr("de_conv1_1", torch.cat([n.cbr("de_conv1_0", _up(x)), feats["layer2"]], 1))
    x = n.cbr("de_conv2_1", torch.cat([n.cbr("de_conv2_0", _up(x)), feats["layer1"]], 1))
    x = n.cbr("de_conv3_1", torch.cat([n.cbr("de_conv3_0", _up(x)), conv1], 1))
    x = n.cbr("de_conv4_0", _up(x))
    return n.relu(n.conv("pred", x, 1, 1)), torch.sigmoid(n.conv("weight_pred", x, 1, 1))
