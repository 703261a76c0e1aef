"""spherical_fusion (iterative) for TRAINING — the reference's model/spherical_model_iterative.py:253-457 assembled from the differentiable
operators of omnifusion_amd.ops, so that the loss of train_erp_depth_iterative.py:268-279 back-propagates on the device:

    from omnifusion_amd.model.trainable_iterative import spherical_fusion      # the one import train_erp_depth_iterative.py changes
    net = spherical_fusion(nrows=4, npatches=18, patch_size=(128, 128), fov=(80, 80)).cuda()
    net.load_state_dict(ckpt)                   # the reference's iterative schema, 'module.' prefix optional
    outs = net(rgb, 2, confidence=True)         # a list of `iter` maps [B,1,H,W], each with a graph behind it
    (sum(berhu(o, gt, mask) for o in outs) / 2).backward(); optimiser.step()

The single-pass module (model/trainable.py) with `down1` for `down` and `mlp_points1` / `mlp_points2` for `mlp_points`: parameters and
buffers are exactly `weights.schema(npatches, iterative=True)`, so a checkpoint moves between this module, the reference and the inference
module (model/spherical_model_iterative.py) with strict=True.  The default patch size is the reference's (256, 256), at which the network
does not exist: it is rejected with the single-pass module's message; 128 is the only size.

The forward (:308-457): the RGB patches and the unit rays at P/4 are sampled once.  Pass 1 adds mlp_points1(rays) [N,64,P/4,P/4] to layer1,
broadcast over the batch.  Pass k >= 2 re-projects the previous panorama depth into P/4 patches — equi2pers_patches WITH its graph: the
reference does not detach pred_list[i], so the loss of pass k sends a gradient through pass k - 1 — scales the rays by it inside
ops.point_conv (mlp_points2.0; the product [bs.N,3,P/4,P/4] is never written), runs the rest of mlp_points2 over [bs.N,.,P/4,P/4] (its batch
statistics are taken over all bs.N maps, as the reference's are) and adds one feature map per item to layer1.  Every pass runs the whole
network with the shared parameters, so in training mode every shared batch normalisation takes one momentum update per pass and
num_batches_tracked rises by `iter` per forward (mlp_points1: by 1, mlp_points2: by iter - 1).  The blend is pers2equi_conf with
confidence, pers2equi without (the reference's default).  `.eval()` runs the same operators from the running statistics.

All six 1x1 convolutions of the point MLPs are ops.PointConv2d (csrc/omni_point_conv.hip): fp32 FMAs, a deterministic weight gradient.

Several GPUs: `omnifusion_amd.sync_batchnorm.convert_model(net)` synchronises every batch normalisation but mlp_points1's
(`SYNCBN_REPLICATED`: its input, the rays, is the same on every rank; mlp_points2's is not), `omnifusion_amd.dist.sync_gradients(net)` adds
the ranks' gradients.

Not built: sharing conv1 .. layer1 between the passes, DataParallel (threads in one process), fp16 storage, an image gradient,
capture of a whole step in a graph, `iter` as a tensor.  fp32 CUDA input, one device per process.
"""
import torch
from torch import nn

from .. import _lib, ops
from ..equi_pers.equi2pers_v3 import equi2pers_patches, equi2pers_aux, pair
from ..equi_pers.pers2equi_v3 import pers2equi, pers2equi_conf
from . import trainable
from .trainable import _bn


def _point_mlp(cin):
    return nn.Sequential(ops.PointConv2d(cin, 16, kernel_size=1, stride=1, padding=0, bias=False), _bn(16, "relu"), nn.Identity(),
                         ops.PointConv2d(16, 64, kernel_size=1, stride=1, padding=0, bias=False), _bn(64, "relu"), nn.Identity())


class spherical_fusion(trainable.spherical_fusion):
    _DOWN = "down1"
    SYNCBN_REPLICATED = ("mlp_points1",)                                       # fed the unit rays alone; mlp_points2 sees rays . depth: synchronised

    def __init__(self, nrows=4, npatches=18, patch_size=(256, 256), fov=(80, 80), *, precision="f16x3"):
        super().__init__(nrows, npatches, patch_size, fov, precision=precision)
        self.__dict__["_rays"] = {}                                            # device -> the unit rays; not a buffer: not in the state dict

    def _add_point_mlps(self):
        self.mlp_points1, self.mlp_points2 = _point_mlp(3), _point_mlp(3)

    def rays(self, device):
        """the unit rays [N,3,P/4,P/4] of the patches' pixels (equi2pers' xyz at P/4, :316): constants"""
        key = str(device)
        if key not in self._rays:
            p4 = int(pair(self.patch_size)[0]) // 4
            self._rays[key] = equi2pers_aux(device, self.fov, self.nrows, (p4, p4), want_xyz=True, want_uv=False)[0]
        return self._rays[key]

    def point_features(self, rays, depth=None):
        """mlp_points1(rays) [N,64,P/4,P/4], or mlp_points2(rays . depth) [bs.N,64,P/4,P/4] for depth [bs.N,1,P/4,P/4] (:387-393)"""
        if depth is None:
            return self.mlp_points1(rays)
        m = self.mlp_points2
        return m[4](m[3](m[1](m[0](rays, scale=depth))))

    def _blend(self, a, c, confidence, erp_hw):
        P = tuple(int(v) for v in pair(self.patch_size))
        if confidence:                                                                                                    # :371-378, 444-451
            return pers2equi_conf(a, c, self.fov, self.nrows, P, erp_hw, layout=_lib.LAYOUT_BNCHW)
        return pers2equi(a, self.fov, self.nrows, P, erp_hw, None, layout=_lib.LAYOUT_BNCHW)                              # :380, 453

    def forward(self, high_res, iter, confidence=False):
        self._check(high_res)
        if isinstance(iter, torch.Tensor) or int(iter) != iter or iter < 1:
            raise ValueError(f"iter must be a Python integer >= 1 (got {iter!r})")
        bs, _, H, W = high_res.shape
        N = self.npatches
        p4 = int(pair(self.patch_size)[0]) // 4
        with torch.cuda.device(high_res.device):
            patches = equi2pers_patches(high_res, self.fov, self.nrows, self.patch_size, layout=_lib.LAYOUT_BNCHW)       # :315 (= :384)
            rays = self.rays(high_res.device)                                                                             # :316
            a, c = self.network(patches, self.point_features(rays), confidence)                                           # :319-369
            outs = [self._blend(a, c, confidence, (H, W))]
            for i in range(int(iter) - 1):                                                                                # :383
                depth = equi2pers_patches(outs[i], self.fov, self.nrows, (p4, p4), layout=_lib.LAYOUT_BNCHW)              # :385, not detached
                a, c = self.network(patches, self.point_features(rays, depth.reshape(bs * N, 1, p4, p4)), confidence)     # :387-442
                outs.append(self._blend(a, c, confidence, (H, W)))
        return outs
