"""Host-side engine of the network: weight packing (BN folding, NHWC-GEMM layouts) and the launch
sequence of one forward over the C-ABI operators of libomnifusion_hip.so.

Everything numeric runs in the HIP library; PyTorch only owns the device buffers (caching
allocator), the stream and — once per `load_state_dict` — the constant folding of the weights
(BatchNorm -> conv, the input-independent `mlp_points` branch of the single-pass model).

`Engine` holds what outlives a forward: packed weights, switches, the split-K workspace and `last`.  A forward's stream, batch size and what
follows from them live in a `_Forward`, made at the top of `Engine.network` / `Engine.transformer`; the launching helpers are its methods.

Reference: model/spherical_model.py:238-314 (single pass), model/spherical_model_iterative.py:308-456.
"""
import ctypes
import os

import torch

from .. import _lib
from .._lib import ptr as _p
from ..equi_pers.equi2pers_v3 import equi2pers_patches, equi2pers_aux, pair, _NPATCH
from ..equi_pers.pers2equi_v3 import pers2equi, pers2equi_conf

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
_LAYERS = [("layer1", 3, 1, 64), ("layer2", 4, 2, 128), ("layer3", 6, 2, 256), ("layer4", 3, 2, 512)]     # name, blocks, stride of the first, width
_BN_EPS = 1e-5
PRECISIONS = ("f16x3", "f16x1", "fp32")


def split_weights_f16x3(w):
    """[Cout][K] fp32 (K % 32 == 0) -> halfs [Cout][K/32][2][32]: hi = fp16(w) (0 below the fp16 normal range),
    lo = fp16((w - hi) * 2048) — the operand format of omni_conv2d_nhwc_f16x3_ws."""
    w = w.to(torch.float32)
    wmax = float(w.abs().max()) if w.numel() else 0.0
    if not wmax < 65504.0:                      # also catches NaN / inf
        raise ValueError(f"folded weight magnitude {wmax:g} is outside the fp16 range of the f16x3 operand format: "
                         "run this checkpoint with OMNI_NET_PRECISION=fp32")
    hi = w.half()
    hi = torch.where(w.abs() < 6.103515625e-05, torch.zeros_like(hi), hi)
    lo = ((w - hi.float()) * 2048.0).half()
    co, k = w.shape
    return torch.stack([hi.reshape(co, k // 32, 32), lo.reshape(co, k // 32, 32)], 2).contiguous()


def strip_module_prefix(sd):
    """checkpoints saved through nn.DataParallel carry a 'module.' prefix (train_erp_depth.py:307)"""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


class Engine:
    # ------------------------------------------------------------------ switches (class attributes: tests, tools and bench.py set them on the class)
    NOMINAL_BATCH = 8
    SINGLE_BATCH = 4           # the batch a lone panorama plans its split-K factors for (latency_plan)
    latency_plan = True
    rows_gemm = True           # ... and its transformer GEMMs (18 rows) take the register-streaming kernel
    fuse_fc2_ln = os.environ.get("OMNI_FUSE_FC2_LN", "1") != "0"   # fc2's split-K second pass also applies the LayerNorm that follows (one launch fewer per layer, same bits)
    fc2_slices = int(os.environ.get("OMNI_FC2_SLICES", "4"))       # a lone panorama: fc2 in this many K slices (1: off) — 16 blocks stream its 4 MB of weights otherwise
    fuse_ln = os.environ.get("OMNI_FUSE_LN", "1") != "0"   # a lone panorama: LayerNorm inside the following rows GEMM (one launch instead of two, same bits)
    fold_point_feat = True     # `layer1 + point_feat` inside layer1's last convolution (one rounding to the SH format instead of two: results move by ~1e-7)
    fuse_up = True             # decoder: up-sampling computed inside the following convolution's halo fill where the shape allows
    # Decoder stages that multiply BEFORE up-sampling: conv3x3(up2(x)) = tap sum of up2(W_t . x), nine 1x1 products on a quarter of the pixels
    # (a quarter of the stage's matrix instructions; the up-sampled tensor never exists).  The set of layer keys that take this path; the
    # operands exist for de_conv0_0 (K = 512) and de_conv1_0 (K = 128).  tools/taps_ab.py, three forwards of 8 panoramas in flight:
    # de_conv0_0 3980 -> 4050 panoramas/s, every round above every round without; de_conv1_0 3980 -> 3975, its 42 MB of fp32 tap products
    # cost what the matrix work saves, so it stays on the up-sampling path (profiles/EXPERIMENTS.md, r13a).  f16x3 only (the other modes'
    # pinned accuracy figures stay); never a function of the batch size.  Results equal the two-kernel form to rounding (< 1e-5 m of depth).
    # (The wider stages de_conv2_0 / de_conv3_0 would write 85 / 340 MB of tap products: they take the one-launch form, `taps_fused` below.)
    taps_first = frozenset(("de_conv0_0",))
    # The 64 -> 64 stages de_conv2_0 (16 x 16 -> 32 x 32) and de_conv3_0 (32 x 32 -> 64 x 64) take the same identity in ONE launch (omni_conv3x3_up2_taps_sh_f16x3,
    # csrc/omni_conv_up2_taps.hip): the tap products are formed, parked in LDS and summed inside a block, so their fp32 values — 85 MB and 340 MB at 144 patches —
    # never reach memory.  The set of layer keys that take this path in `_Forward.up_conv`; the operands `<key>.tapsf.w16` (packed like `.taps.w16`) exist for both stages.  f16x3 with an SH result
    # only; never a function of the batch size or of the latency plan.  tools/taps_fused_ab.py, three forwards of 8 panoramas in
    # flight: none 4218, de_conv3_0 4261, de_conv2_0 4236, both 4278 panoramas/s, every round of each case above every round without — although either launch
    # ALONE is no faster than the halo kernel (174 -> 178 us, 53 -> 61 us): the region runs at the power cap and the stages issue 0.375x / 0.25x the matrix
    # instructions (profiles/EXPERIMENTS.md, r25a).
    taps_fused = frozenset(("de_conv2_0", "de_conv3_0"))
    # de_conv4_0 and the two heads in one pass (omni_conv3x3_up2_heads_sh_f16x3): the decoder's last feature map is never written.  False: the two
    # kernels (fp32 heads; `Engine.last["de_conv4_0"]` then holds that map — the G6 check-point test reads it).  The outputs agree to ~1e-6 relative.
    fuse_heads = os.environ.get("OMNI_FUSE_HEADS", "1") != "0"
    # Passes of a few panoramas through the widest stages (same kernels, same bits) were worth +1.3 % with three forwards in flight while the
    # up-sampled tensors still went through HBM; since the up-sampling is computed inside the convolution (fuse_up) they change nothing
    # (tools/chunk_ab.py: 3515 vs 3517 panoramas/s), so the default is the whole batch at once.
    tail_chunk = 0             # panoramas per pass through the decoder's two widest stages (0: the whole batch at once)
    front_chunk = 0            # ... and through stem -> max-pool

    def __init__(self, nrows, npatches, patch_size, fov, iterative, precision=None):
        self.nrows, self.npatches, self.iterative = nrows, npatches, iterative
        self.patch_size = pair(patch_size)
        self.fov = pair(fov)
        if self.patch_size[0] != self.patch_size[1]:
            raise ValueError("square patches only")
        self.w = None          # packed weights (device tensors)
        self.device = None
        self._ws, self._ws_retired = None, []      # the split-K workspace (`_workspace`)
        # "f16x3": conv products on the fp16 matrix cores with split operands (fp32-class accuracy, 3/16 of the MFMA time),
        # activations between the convolutions in the split-half layout; "f16x1": the same layout and weights, but every convolution
        # of the encoder / decoder multiplies the hi halves only (one MFMA per product block, ~1e-3 relative; the transformer's
        # GEMMs and the heads' own products stay f16x3); "fp32": the exact fp32 MFMA, fp32 NHWC activations.
        # `precision` (the constructor's keyword) first, then OMNI_NET_PRECISION, then "f16x3".
        self.precision = precision if precision is not None else os.environ.get("OMNI_NET_PRECISION", "f16x3")

    @property
    def sh(self):
        """activations between the convolutions are split-half (SH) tensors"""
        return self.precision in ("f16x3", "f16x1")

    @property
    def terms(self):
        """fp16 matrix instructions per product block of the convolutions: 3 (f16x3), 1 (f16x1); 0 for the exact fp32 path"""
        return {"f16x3": 3, "f16x1": 1}.get(self.precision, 0)

    @property
    def _x1(self):
        """fmt bit 3 of the SH convolution entry points: the f16x1 instantiation"""
        return 8 if self.terms == 1 else 0

    def lane(self):
        """A second execution context over the SAME packed weights (own split-K workspace): the model runs the two halves
        of a batch on two streams so that one half's kernel tails overlap the other half's work."""
        e = Engine(self.nrows, self.npatches, self.patch_size, self.fov, self.iterative, precision=self.precision)
        e.w, e.device, e.head_bias = self.w, self.device, getattr(self, "head_bias", None)
        return e

    # ------------------------------------------------------------------ packing
    @staticmethod
    def _fold(sd, conv, bn):
        w = sd[conv + ".weight"].double()
        if w.dim() == 5:
            w = w[..., 0]
        g = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + _BN_EPS)
        b = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * g
        return w * g[:, None, None, None], b

    @staticmethod
    def _gemm_layout(w):
        # [O, I, kh, kw] -> [O][kh*kw*I] with k = (ky, kx, c)
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)

    def pack(self, state_dict, device):
        sd = {k: v.detach().cpu() for k, v in strip_module_prefix(state_dict).items()}
        dev = torch.device(device)
        f = lambda t: t.to(torch.float32).contiguous().to(dev)
        W = {}
        w, b = self._fold(sd, "conv1", "bn1")                                    # stem: [147][64], k = (ky*7+kx)*3 + c
        W["stem.w"] = f(w.permute(2, 3, 1, 0).reshape(147, 64)); W["stem.b"] = f(b)
        wk = torch.zeros((64, 3, 7, 8), dtype=torch.float64); wk[..., :7] = w                 # k = (c*7 + ky)*8 + kx, kx = 7 zero
        W["stem.w16"] = split_weights_f16x3(torch.cat([wk.reshape(64, 168), torch.zeros((64, 24), dtype=torch.float64)], 1)).to(dev)

        def convbn(key, conv, bn):
            w, b = self._fold(sd, conv, bn)
            wg = self._gemm_layout(w).to(torch.float32)
            W[key + ".w"] = f(wg); W[key + ".b"] = f(b)
            W[key + ".w16"] = split_weights_f16x3(wg).to(dev)
        for lname, nblk, _, _ in _LAYERS:
            for i in range(nblk):
                p = f"{lname}.{i}"
                convbn(p + ".c1", p + ".conv1", p + ".bn1")
                convbn(p + ".c2", p + ".conv2", p + ".bn2")
                if (p + ".downsample.0.weight") in sd:
                    convbn(p + ".ds", p + ".downsample.0", p + ".downsample.1")
        for name in ("de_conv0_0", "de_conv0_1", "de_conv1_0", "de_conv1_1", "de_conv2_0", "de_conv2_1",
                     "de_conv3_0", "de_conv3_1", "de_conv4_0"):
            convbn(name, name + ".conv", name + ".bn")
        for name, op in (("de_conv0_0", ".taps.w16"), ("de_conv1_0", ".taps.w16"), ("de_conv2_0", ".tapsf.w16"), ("de_conv3_0", ".tapsf.w16")):
            # the same folded weights tap-major, [9*Cout][Cin] with row t*Cout + co = W[co][t][:]: the operand of the nine 1x1 tap products on the
            # low-resolution map — `.taps.w16` for the two-launch stages (taps_first), `.tapsf.w16` for the one-launch stages (taps_fused) of `_Forward.up_conv`
            w, _ = self._fold(sd, name + ".conv", name + ".bn")
            W[name + op] = split_weights_f16x3(w.permute(2, 3, 0, 1).reshape(9 * w.shape[0], w.shape[1]).to(torch.float32)).to(dev)
        down = "down1" if self.iterative else "down"
        W["down.w"] = f(sd[down + ".weight"].reshape(32, 512)); W["down.b"] = f(sd[down + ".bias"])
        W["down.w16"] = split_weights_f16x3(sd[down + ".weight"].reshape(32, 512)).to(dev)
        W["pos"] = f(sd["transformer.pos_emb"].reshape(self.npatches, 512))
        for i in range(6):
            p = f"transformer.layer.{i}"
            for k in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "attn.q.weight", "attn.kv.weight",
                      "attn.proj.weight", "attn.proj.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"):
                W[f"t{i}.{k}"] = f(sd[f"{p}.{k}"])
        for i in range(6):                                                       # f16x3 operands of the transformer GEMMs
            t = f"t{i}."
            W[t + "attn.qkv.w16"] = split_weights_f16x3(torch.cat([W[t + "attn.q.weight"], W[t + "attn.kv.weight"]], 0).cpu()).to(dev)
            for k in ("attn.proj", "mlp.fc1", "mlp.fc2"):
                W[t + k + ".w16"] = split_weights_f16x3(W[t + k + ".weight"].cpu()).to(dev)
        W["enc_norm.w"] = f(sd["transformer.encoder_norm.weight"]); W["enc_norm.b"] = f(sd["transformer.encoder_norm.bias"])
        hw = torch.stack([sd["pred.weight"][0, :, :, :, 0], sd["weight_pred.weight"][0, :, :, :, 0]])    # [2,32,3,3]
        W["heads.w"] = f(hw.permute(0, 2, 3, 1).reshape(2, 9, 32))
        import numpy as np                                                       # the same weights as the f16x3 operand of the fused de_conv4_0 + heads kernel
        hw_host = np.ascontiguousarray(hw.permute(0, 2, 3, 1).reshape(2, 9, 32).to(torch.float32).numpy())
        frag = np.zeros(4 * 64 * 8, np.float16)
        _lib.check(_lib.load().omni_heads_pack_f16x3(hw_host.ctypes.data_as(ctypes.c_void_p), frag.ctypes.data_as(ctypes.c_void_p)), "heads_pack")
        W["heads.w16f"] = torch.from_numpy(frag).to(dev)
        self.head_bias = (float(sd["pred.bias"][0]), float(sd["weight_pred.bias"][0]))

        def mlp(name):
            w1, b1 = self._fold(sd, name + ".0", name + ".1")
            w2, b2 = self._fold(sd, name + ".3", name + ".4")
            return w1[:, :, 0, 0], b1, w2[:, :, 0, 0], b2
        P4 = self.patch_size[0] // 4
        if self.iterative:
            for name in ("mlp_points1", "mlp_points2"):
                w1, b1, w2, b2 = mlp(name)
                W[name + ".w1"], W[name + ".b1"], W[name + ".w2"], W[name + ".b2"] = f(w1), f(b1), f(w2), f(b2)
        else:
            # single pass: the input of mlp_points is [cx, cy, 1, cx, cy] broadcast over the patch
            # (spherical_model.py:245-251) — a constant of the weights: fold it to one vector per patch.
            cp = (ctypes.c_float * (2 * self.npatches))()
            _lib.check(_lib.load().omni_patch_centers(int(self.nrows), 0, cp), "patch_centers")
            c = torch.tensor(list(cp), dtype=torch.float64).reshape(self.npatches, 2)
            x = torch.cat([c, torch.ones(self.npatches, 1, dtype=torch.float64), c], 1)          # [N,5]
            w1, b1, w2, b2 = mlp("mlp_points")
            h = torch.relu(x @ w1.T + b1)
            pf = torch.relu(h @ w2.T + b2)                                                         # [N,64]
            W["point_feat"] = f(pf[:, None, None, :].expand(self.npatches, P4, P4, 64))
        self.w, self.device = W, dev

    def read_overflow_flag(self, reset=True):
        """sticky range flag of the split-half format on this engine's device (omni_sh_overflow); synchronises"""
        if self.device is None:
            return False
        flag = ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().omni_sh_overflow(ctypes.byref(flag), 1 if reset else 0), "sh_overflow")
        return bool(flag.value)

    def _workspace(self, nbytes, device):
        """split-K scratch: one buffer reused by every launch of the stream (launches are stream-ordered)"""
        nbytes = int(nbytes)
        if nbytes == 0:
            return None, 0
        ws = self._ws
        if ws is None or ws.numel() * 4 < nbytes or ws.device != device:
            if ws is not None:                   # a hipGraph captured earlier (graphed()) still replays into the old buffer:
                self._ws_retired.append(ws)      # keep it alive for the engine's lifetime
            self._ws = ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        return ws, ws.numel() * 4

    # ------------------------------------------------------------------ the two entry points of a forward
    def transformer(self, d, bs):
        """The transformer over the N tokens of each panorama (:263-268): position embedding, six blocks, encoder_norm.
        d: fp32 [bs*N, P/32, P/32, 32] (the `down` projection of layer4).  Returns the fp32 token matrix [bs*N, 512]."""
        return _Forward(self, bs, d).transformer(d)

    def network(self, patches, point_feat, bs, confidence, out=None):
        """patches: planar [bs, N, 3, P, P]; point_feat: NHWC [N or bs*N, P/4, P/4, 64].
        Returns (a, c) planar [bs, N, 1, P, P]: a = relu(pred) (* conf), c = sigmoid(weight) or None."""
        f = _Forward(self, bs, patches)
        new, sh, wp = f.new, f.sh, f.wp                             # sh: activations between the convolutions are SH, else fp32 NHWC
        N, P = self.npatches, self.patch_size[0]
        M = bs * N
        P2, P4, P8, P16, P32 = P // 2, P // 4, P // 8, P // 16, P // 32
        conv1 = new(M, P2, P2, 64)
        x = new(M, P4, P4, 64)
        pat = patches.view(M, 3, P, P)
        if self.terms == 1 and P % 32:
            raise ValueError(f"precision f16x1 needs a patch size that is a multiple of 32 (got {P})")
        if sh and P % 32 == 0:
            stem, stem_w = ("omni_stem_sh_f16x1" if f.x1 else "omni_stem_sh_f16x3"), "stem.w16"
        else:
            stem, stem_w = ("omni_stem_sh" if sh else "omni_stem_f32"), "stem.w"
        for m0, m1 in self._chunks(bs, N, self.front_chunk):        # stem -> maxpool per chunk: conv1 is re-read while still cached
            f.run(stem, "stem", _p(pat[m0:m1]), wp(stem_w), wp("stem.b"), _p(conv1[m0:m1]), m1 - m0, P)
            f.run("omni_maxpool3x3s2_sh" if sh else "omni_maxpool3x3s2_f32", "maxpool", _p(conv1[m0:m1]), _p(x[m0:m1]), m1 - m0, P2, P2, 64)
        feats = {}
        cin, size = 64, P4
        fold = sh and self.fold_point_feat                          # layer1 + point_feat (:258) in the epilogue of layer1's last convolution ...
        for lname, nblk, stride, cout in _LAYERS:
            for i in range(nblk):
                p = f"{lname}.{i}"
                s = stride if i == 0 else 1
                ident = x
                if (p + ".ds.w") in self.w:
                    ident = f.conv(x, p + ".ds", M, size, size, cin, cout, 1, s, 0, ACT_NONE)
                y = f.conv(x, p + ".c1", M, size, size, cin, cout, 3, s, 1, ACT_RELU)
                size = (size + 2 - 3) // s + 1
                post = point_feat if (fold and lname == "layer1" and i == nblk - 1) else None
                x = f.conv(y, p + ".c2", M, size, size, cout, cout, 3, 1, 1, ACT_RELU, res=ident, post=post)
                cin = cout
            if lname == "layer1" and not fold:                      # ... or as a pass of its own
                f.run("omni_add_period_sh" if sh else "omni_add_period_f32", "add point_feat", _p(x), _p(point_feat), x.numel(), point_feat.numel())
            feats[lname] = x
        layer1, layer2, layer3, layer4 = (feats[k] for k in ("layer1", "layer2", "layer3", "layer4"))
        # ---- transformer over the N tokens of each panorama (:263-268)
        if 32 * P32 * P32 != 512:
            raise RuntimeError(f"patch size {P}: token dim {32 * P32 * P32} != 512 — the reference network only exists at "
                               "patch size 128 (SURVEY.md finding 0.1)")
        tok = f.transformer(f.conv(layer4, "down", M, P32, P32, 512, 32, 1, 1, 0, ACT_NONE, out_f32=True))
        f.run("omni_add_hw_sh" if sh else "omni_add_hw_f32", "token bias", _p(layer4), _p(tok), M, P32 * P32, 512)
        # ---- decoder (:270-302); torch.cat is the two-source form of the conv
        x = f.up_conv(layer4, "de_conv0_0", M, P32, P32, 512, 256, ACT_RELU)
        x = f.conv(x, "de_conv0_1", M, P16, P16, 256, 128, 3, 1, 1, ACT_RELU, x2=layer3, C2=256)
        x = f.up_conv(x, "de_conv1_0", M, P16, P16, 128, 128, ACT_RELU)
        x = f.conv(x, "de_conv1_1", M, P8, P8, 128, 64, 3, 1, 1, ACT_RELU, x2=layer2, C2=128)
        x = f.up_conv(x, "de_conv2_0", M, P8, P8, 64, 64, ACT_RELU)
        x = f.conv(x, "de_conv2_1", M, P4, P4, 64, 64, 3, 1, 1, ACT_RELU, x2=layer1, C2=64)
        # the two widest stages, optionally a few panoramas at a time (Engine.tail_chunk; no operator here mixes patches)
        a, c = out if out is not None else (new(bs, N, 1, P, P), new(bs, N, 1, P, P) if confidence else None)
        av, cv = a.view(M, P, P), c.view(M, P, P) if c is not None else None
        fused = sh and self.fuse_heads and P % 32 == 0              # (the fused kernel up-samples inside whatever `fuse_up` says)
        x_in, de4 = x, (None if fused else new(M, P, P, 32))
        for m0, m1 in self._chunks(bs, N, self.tail_chunk):
            Mc = m1 - m0
            x = f.up_conv(x_in[m0:m1], "de_conv3_0", Mc, P4, P4, 64, 64, ACT_RELU)
            x = f.conv(x, "de_conv3_1", Mc, P2, P2, 64, 32, 3, 1, 1, ACT_RELU, x2=conv1[m0:m1], C2=64)
            planes = (_p(av[m0:m1]), _p(cv[m0:m1]) if cv is not None else None, Mc, P, 1 if confidence else 0)
            if fused:                                                # de_conv4_0 + pred / weight_pred in one pass: its 302-MB output (8 panoramas) never exists
                nb = int(f.lib.omni_up2_heads_scratch_bytes(Mc, P))
                hs = new((nb + 3) // 4)
                f.run("omni_conv3x3_up2_heads_sh_f16x1" if f.x1 else "omni_conv3x3_up2_heads_sh_f16x3", "up+conv+heads",
                      _p(x), wp("de_conv4_0.w16"), wp("de_conv4_0.b"), wp("heads.w16f"), *self.head_bias, _p(hs), nb, *planes)
                continue
            f.up_conv(x, "de_conv4_0", Mc, P2, P2, 32, 32, ACT_RELU, out_f32=True, out=de4[m0:m1])
            f.run("omni_heads_f32", "heads", _p(de4[m0:m1]), wp("heads.w"), *self.head_bias, *planes)
        self.last = {"de_conv4_0": de4, "layer4": layer4}
        return a, c

    @staticmethod
    def _chunks(bs, N, per):
        per = bs if per <= 0 else min(per, bs)
        return [(b0 * N, min(bs, b0 + per) * N) for b0 in range(0, bs, per)]

    def blend(self, a, c, erp_hw):
        P = self.patch_size
        if c is not None:
            return pers2equi_conf(a, c, self.fov, self.nrows, P, erp_hw, layout=_lib.LAYOUT_BNCHW)
        return pers2equi(a, self.fov, self.nrows, P, erp_hw, None, layout=_lib.LAYOUT_BNCHW)

    def mlp_points(self, name, xyz, depth, Mo):
        lib = _lib.load()
        P4 = self.patch_size[0] // 4
        out = torch.empty((Mo, P4, P4, 64), dtype=torch.float32, device=xyz.device)
        s = _lib.stream_of(xyz)
        _lib.check(lib.omni_mlp_points_f32(_p(xyz), _p(depth), _p(self.w[name + ".w1"]), _p(self.w[name + ".b1"]),
                                           _p(self.w[name + ".w2"]), _p(self.w[name + ".b2"]), _p(out), Mo, self.npatches,
                                           P4 * P4, s), "mlp_points")
        return out

    def check_input(self, rgb):
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[1] != 3:
            raise ValueError("expected an RGB panorama batch [B,3,H,W]")
        if not rgb.is_cuda:
            raise ValueError("the model runs on an MI355X only (got a CPU tensor); there is no CPU path")
        if rgb.dtype != torch.float32:
            raise ValueError("float32 input expected")
        if _NPATCH[self.nrows] != self.npatches:
            raise ValueError("npatches does not match nrows")


class _Tokens:
    """The token matrix between two transformer blocks of the SH path, in one of three states: plain (`tok`); with the LayerNorm its next
    consumer needs already made by fc2's second pass (`normed`); or not summed yet (a lone panorama) — fc2's K slices `parts`, to which the
    next kernel adds the bias `bkey` and the residual `tok`.  `_Forward.next_norm` is the one consumer."""
    __slots__ = ("tok", "normed", "parts", "bkey")

    def __init__(self, tok, normed=None, parts=None, bkey=None):
        self.tok, self.normed, self.parts, self.bkey = tok, normed, parts, bkey


class _Forward:
    """What one call of Engine.network / Engine.transformer needs beside the engine: the stream and device of its input, the batch size, and
    what follows from them.  Made at the top of the entry point and dropped at its end; the launching helpers are its methods, so none of
    them can meet another forward's stream or batch."""

    def __init__(self, engine, bs, like):
        self.e, self.w, self.lib = engine, engine.w, _lib.load()
        self.bs, self.M, self.stream, self.device = bs, bs * engine.npatches, _lib.stream_of(like), like.device
        self.sh, self.x1 = engine.sh, engine._x1
        # A LONE panorama (BASELINE cfg 2) is latency-bound — every layer is one round of at most one block per CU and costs the length of its
        # K loop.  This is the one statement of that rule; everything a lone panorama does differently follows from the four names below.
        self.lone = bs == 1 and engine.latency_plan
        self.lat = 4 if self.lone else 0                            # fmt bit 2 of the SH convolutions: keep the im2col tiles for 16-wide images
        self.rows_form = self.lone and engine.rows_gemm and self.M <= 32      # its transformer GEMMs (at most 32 rows) in the register-streaming kernels
        self.plan_batch = engine.SINGLE_BATCH if self.lone else engine.NOMINAL_BATCH        # the batch `splitk` plans for

    def run(self, name, label, *args):
        """one library call on this forward's stream"""
        _lib.check(getattr(self.lib, name)(*args, self.stream), label)

    def new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def wp(self, key):
        """pointer of a packed weight (None for no key)"""
        return _p(self.w[key]) if key else None

    # ------------------------------------------------------------------ convolutions
    def splitk(self, rows, Cout, ksteps):
        """Split factor planned for a NOMINAL batch (not the actual one), so that the K summation order — and with it
        every output bit — is the same whether a panorama is processed inside a batch of 2 or of 64 (image-sharded
        multi-GPU runs reproduce single-GPU results bit for bit).  A lone panorama plans for SINGLE_BATCH instead:
        deeper splits on layer3/layer4/decoder, 1.28 -> 1.13 ms per forward, results equal to the batched ones to 2e-5 abs
        instead of bit for bit (`Engine.latency_plan = False` restores the one plan for all)."""
        S = int(self.lib.omni_conv2d_splitk_plan(rows // self.bs * self.plan_batch, Cout, ksteps))
        if S <= 1:
            return 1, None, 0
        return (S,) + self.e._workspace(S * rows * Cout * 4, self.device)

    def conv(self, x, key, M, H, Wd, C1, Cout, k, stride, pad, act, x2=None, C2=0, res=None, bias=True, out_f32=False, out=None, post=None):
        """One convolution (+ folded BN, bias, residual, activation).  In the f16x3 mode the activations x, x2, res and
        the result are split-half (SH) tensors (csrc/omni_sh.h) unless out_f32 asks for a plain fp32 NHWC result."""
        Ho = (H + 2 * pad - k) // stride + 1
        Wo = (Wd + 2 * pad - k) // stride + 1
        if out is None:
            out = self.new(M, Ho, Wo, Cout)
        S, ws, nb = self.splitk(M * Ho * Wo, Cout, k * k * (C1 + C2) // 32)
        late_post = None
        if post is not None and (S > 1 or not self.sh or out_f32):
            # the fused `+ post` epilogue exists for un-split SH launches only (omni_conv2d_sh_f16x3_post_ws rejects splitk > 1): a shape
            # whose plan splits K (few rows: small patches, nrows = 3, a lone panorama) adds it as a pass of its own instead
            late_post, post = post, None
        tensors = (_p(x), _p(x2), self.wp(key + (".w16" if self.sh else ".w")), self.wp(key + ".b") if bias else None, _p(res), _p(out))
        shape = (M, H, Wd, C1, C2, Cout, k, k, stride, pad, act, S, _p(ws), nb)
        fmt = (0 if out_f32 else 1) | self.x1
        if not self.sh:
            self.run("omni_conv2d_nhwc_f32_ws", "conv2d " + key, *tensors, *shape)
        elif post is not None:                                      # `+ post` after the activation, inside the epilogue (SH mode, never split)
            self.run("omni_conv2d_sh_f16x3_post_ws", "conv2d " + key, *tensors, fmt, *shape, _p(post), post.numel())
        else:
            self.run("omni_conv2d_sh_f16x3_ws", "conv2d " + key, *tensors, fmt | self.lat, *shape)
        if late_post is not None:                                   # (an fp32 NHWC output is never split-half)
            self.run("omni_add_period_f32" if (out_f32 or not self.sh) else "omni_add_period_sh", "add post " + key,
                     _p(out), _p(late_post), out.numel(), late_post.numel())
        return out

    def up_conv(self, x, key, M, H, Wd, C, Cout, act, out_f32=False, out=None):
        """conv3x3(upsample2x(x)) — `F.interpolate` + a decoder stage's first ConvBnReLU (:279-301), in the first form of four that serves the
        stage.  The two tap-product forms are chosen by the layer key, the arithmetic mode and the shape alone.  (de_conv0_0 and de_conv1_0 are
        never offered form 3: at patch size 128, the only one the network exists at, their 8 x 8 and 16 x 16 outputs are no shapes of the halo
        kernel, so outside `taps_first` they up-sample and convolve in two launches.)"""
        e, Ho, Wo = self.e, 2 * H, 2 * Wd
        result = lambda: self.new(M, Ho, Wo, Cout) if out is None else out        # made AFTER a form's intermediate tensor: a forward allocates in the order it always did
        taps = self.sh and e.terms == 3 and not out_f32
        if key in e.taps_first and taps and Cout % 32 == 0 and H * Wd <= 64:      # 1. tap products on the low-resolution map (a GEMM), then their sum
            y = self.conv(x, key + ".taps", M, H, Wd, C, 9 * Cout, 1, 1, 0, ACT_NONE, bias=False, out_f32=True)
            out = result()
            self.run("omni_up2_tapsum_sh", "tap sum " + key, _p(y), self.wp(key + ".b"), _p(out), M, H, Wd, Cout, act)
        elif key in e.taps_fused and taps and C == 64 and Cout == 64 and ((Wd == 32 and H % 8 == 0) or (H == 16 and Wd == 16)):     # 2. ... in one launch
            out = result()
            self.run("omni_conv3x3_up2_taps_sh_f16x3", "up+conv (tap products) " + key, _p(x), self.wp(key + ".tapsf.w16"), self.wp(key + ".b"), _p(out), 1,
                     M, H, Wd, C, Cout, act)
        elif self.sh and e.fuse_up and Wo % 32 == 0 and Ho % 4 == 0:      # 3. up-sampling inside the convolution's halo fill (same bits as 4.)
            out = result()
            self.run("omni_conv3x3_up2_sh_f16x3", "up+conv " + key, _p(x), self.wp(key + ".w16"), self.wp(key + ".b"), _p(out),
                     (0 if out_f32 else 1) | self.lat | self.x1, M, H, Wd, C, Cout, act)
        else:                                                       # 4. up-sample, then convolve
            y = self.new(M, Ho, Wo, C)
            self.run("omni_upsample_bilinear_sh" if self.sh else "omni_upsample_bilinear_f32", "upsample", _p(x), _p(y), M, H, Wd, C, Ho, Wo)
            out = self.conv(y, key, M, Ho, Wo, C, Cout, 3, 1, 1, act, out_f32=out_f32, out=out)
        return out

    # ------------------------------------------------------------------ transformer
    def transformer(self, d):
        """position embedding, six blocks, encoder_norm: fp32 [M, P/32, P/32, 32] -> fp32 [M, 512]"""
        tok = self.new(self.M, 512)
        self.run("omni_token_pack_f32", "token_pack", _p(d), self.wp("pos"), _p(tok), self.M, self.e.npatches, d.shape[1] * d.shape[2], 32)
        return self.blocks_sh(tok) if self.sh else self.blocks_f32(tok)

    def blocks_f32(self, tok):
        for i in range(6):
            t = f"t{i}."
            y = self.ln_f32(tok, t + "norm1.weight", t + "norm1.bias", 1e-5)
            q = self.gemm_f32(y, t + "attn.q.weight", None, 512, 512)
            kv = self.gemm_f32(y, t + "attn.kv.weight", None, 512, 1024)
            att = self.new(self.M, 512)
            self.run("omni_attention_f32", "attention", _p(q), _p(kv), _p(att), self.bs, self.e.npatches)
            tok = self.gemm_f32(att, t + "attn.proj.weight", t + "attn.proj.bias", 512, 512, res=tok)
            y = self.ln_f32(tok, t + "norm2.weight", t + "norm2.bias", 1e-5)
            h = self.gemm_f32(y, t + "mlp.fc1.weight", t + "mlp.fc1.bias", 512, 2048, act=ACT_GELU)
            tok = self.gemm_f32(h, t + "mlp.fc2.weight", t + "mlp.fc2.bias", 2048, 512, res=tok)
        return self.ln_f32(tok, "enc_norm.w", "enc_norm.b", 1e-6)

    def blocks_sh(self, tok):
        """LN / attention emit SH, the GEMMs run f16x3 from it"""
        state = _Tokens(tok)
        norms = [(f"t{i}.norm1.weight", f"t{i}.norm1.bias", 1e-5) for i in range(6)] + [("enc_norm.w", "enc_norm.b", 1e-6)]     # what consumes each block's result
        for i in range(6):
            t = f"t{i}."
            tok, qkv = self.next_norm(state, norms[i], t + "attn.qkv.w16")
            att = self.new(self.M, 512)
            self.run("omni_attention_qkv_sh", "attention", _p(qkv), _p(att), self.bs, self.e.npatches)
            tok = self.gemm_sh(att, t + "attn.proj.w16", t + "attn.proj.bias", 512, 512, res=tok)
            h = self.ln_gemm_sh(tok, t + "norm2.weight", t + "norm2.bias", 1e-5, t + "mlp.fc1.w16", t + "mlp.fc1.bias", 2048, act=ACT_GELU, out_sh=True)
            state = self.fc2(h, t + "mlp.fc2.w16", t + "mlp.fc2.bias", tok, norms[i + 1], out_sh=i < 5)
        return self.next_norm(state, norms[6])[1]

    def next_norm(self, state, ln, qkv=None):
        """The consumer of a token state: the LayerNorm `ln` = (weight key, bias key, eps) of the tokens and the `qkv` GEMM of the next block on
        it, or (qkv None) the final encoder_norm alone with an fp32 result — in the kernel that fits the state.  Returns (tokens, result)."""
        lnw, lnb, eps = ln
        if state.parts is not None:                                 # fc2's K slices: sum + bias + residual + LayerNorm (+ GEMM) in one kernel
            S = state.parts.shape[0]
            tok, out = self.new(self.M, 512), self.new(self.M, 1536 if qkv else 512)
            if qkv:
                self.run("omni_gemm_rows_ln_parts_sh_f16x3", "ln+gemm (slices) " + qkv, _p(state.parts), S, self.wp(state.bkey), _p(state.tok), _p(tok),
                         self.wp(lnw), self.wp(lnb), eps, _p(self.rows_weights(qkv, 1536, 512)), None, _p(out), 0, self.M, 1536, ACT_NONE)
            else:
                self.run("omni_splitk_reduce_ln512", "reduce+ln", _p(state.parts), S, self.wp(state.bkey), _p(state.tok), _p(tok),
                         self.wp(lnw), self.wp(lnb), eps, _p(out), 0, self.M)
            return tok, out
        if state.normed is not None:                                # fc2's second pass has made the LayerNorm already
            return state.tok, (self.gemm_sh(state.normed, qkv, None, 512, 1536) if qkv else state.normed)
        return state.tok, (self.ln_gemm_sh(state.tok, lnw, lnb, eps, qkv, None, 1536) if qkv else self.ln_f32(state.tok, lnw, lnb, eps))

    def gemm_f32(self, x, wkey, bkey, K, Nout, act=ACT_NONE, res=None):
        out = self.new(self.M, Nout)
        S, ws, nb = self.splitk(self.M, Nout, K // 32)
        self.run("omni_conv2d_nhwc_f32_ws", "gemm " + wkey, _p(x), None, self.wp(wkey), self.wp(bkey), _p(res), _p(out),
                 self.M, 1, 1, K, 0, Nout, 1, 1, 1, 0, act, S, _p(ws), nb)
        return out

    def rows_weights(self, w16key, Nout, K):
        """the transformer matrix `w16key` in the fragment order of omni_gemm_rows_sh_f16x3 (made on first use: only single-panorama
        forwards need the second copy, 75 MB for the six layers)"""
        key = w16key + ".rows"
        w = self.w.get(key)
        if w is None:
            src = self.w[w16key]
            w = torch.empty_like(src)
            self.run("omni_gemm_rows_pack", "gemm_rows_pack", _p(src), _p(w), Nout, K)
            if not torch.cuda.is_current_stream_capturing():     # engines on other streams share the dict: hand over a finished tensor
                torch.cuda.current_stream(src.device).synchronize()
            self.w[key] = w
        return w

    def gemm_sh(self, x, w16key, bkey, K, Nout, act=ACT_NONE, res=None, out_sh=False):
        """f16x3 GEMM on an SH activation matrix x [M, K]; res (fp32) and bias optional; result fp32 or SH"""
        out = self.new(self.M, Nout)
        if self.rows_form and K in (512, 2048):                     # a lone panorama: the register-streaming form
            self.run("omni_gemm_rows_sh_f16x3", "gemm " + w16key, _p(x), _p(self.rows_weights(w16key, Nout, K)), self.wp(bkey), _p(res), _p(out),
                     1 if out_sh else 0, self.M, K, Nout, act)
            return out
        S, ws, nb = (1, None, 0) if K <= 512 else self.splitk(self.M, Nout, K // 32)
        self.run("omni_conv2d_sh_f16x3_ws", "gemm " + w16key, _p(x), None, self.wp(w16key), self.wp(bkey), _p(res), _p(out),
                 (1 if out_sh else 0) | 2, self.M, 1, 1, K, 0, Nout, 1, 1, 1, 0, act, S, _p(ws), nb)
        return out

    def fc2(self, h, w16key, bkey, tok, nxt, out_sh):
        """tok + fc2(h) as a token state.  Batches: where fc2 runs split-K, the LayerNorm `nxt` = (weight key, bias key, eps) of the result, SH or fp32,
        in the same second pass (omni_gemm_sh_f16x3_ln512_ws).  A lone panorama: fc2 as K slices whose sum the NEXT kernel forms
        (omni_gemm_rows_slices_sh_f16x3)."""
        e, M = self.e, self.M
        if self.rows_form and e.fc2_slices > 1 and e.fuse_ln:
            parts = self.new(e.fc2_slices, M, 512)
            self.run("omni_gemm_rows_slices_sh_f16x3", "gemm slices " + w16key, _p(h), _p(self.rows_weights(w16key, 512, 2048)), _p(parts), M, 2048, 512, e.fc2_slices)
            return _Tokens(tok, parts=parts, bkey=bkey)
        S, ws, nb = (1, None, 0) if self.rows_form else self.splitk(M, 512, 2048 // 32)
        if S <= 1 or not e.fuse_fc2_ln:
            return _Tokens(self.gemm_sh(h, w16key, bkey, 2048, 512, res=tok))
        wk, bk, eps = nxt
        out, y = self.new(M, 512), self.new(M, 512)
        self.run("omni_gemm_sh_f16x3_ln512_ws", "gemm+ln " + w16key, _p(h), self.wp(w16key), self.wp(bkey), _p(tok), _p(out), self.wp(wk), self.wp(bk), eps,
                 _p(y), 1 if out_sh else 0, M, 2048, S, _p(ws), nb)
        return _Tokens(out, normed=y)

    def ln_gemm_sh(self, x, lnw, lnb, eps, w16key, bkey, Nout, act=ACT_NONE, out_sh=False):
        """LayerNorm(512) + GEMM (K = 512) on the fp32 token matrix x [M, 512]: one launch for a lone panorama, else the two kernels"""
        if self.rows_form and self.e.fuse_ln:
            out = self.new(self.M, Nout)
            self.run("omni_gemm_rows_ln_sh_f16x3", "ln+gemm " + w16key, _p(x), self.wp(lnw), self.wp(lnb), eps, _p(self.rows_weights(w16key, Nout, 512)),
                     self.wp(bkey), None, _p(out), 1 if out_sh else 0, self.M, Nout, act)
            return out
        y = torch.empty_like(x)
        self.run("omni_layernorm512_sh", "layernorm", _p(x), self.wp(lnw), self.wp(lnb), _p(y), self.M, eps)
        return self.gemm_sh(y, w16key, bkey, 512, Nout, act=act, out_sh=out_sh)

    def ln_f32(self, x, wk, bk, eps):
        y = torch.empty_like(x)
        self.run("omni_layernorm512_f32", "layernorm", _p(x), self.wp(wk), self.wp(bk), _p(y), self.M, eps)
        return y
