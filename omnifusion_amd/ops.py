"""Differentiable operators of libomnifusion_hip.so for torch models: the network's convolution and its batch normalisation, each with
its backward.

    y = conv2d(x, weight, bias=None, *, x2=None, res=None, stride=1, padding=0, act="none" | "relu", precision="f16x3" | "f16x1")
    layer = Conv2d(64, 64, 3, padding=1, act="relu")          # an nn.Conv2d whose forward is the call above (precision="f16x3")
    y = batch_norm(x, weight=None, bias=None, running_mean=None, running_var=None, *, res=None, training=True, momentum=0.1, eps=1e-5,
                   act="none" | "relu")
    layer = BatchNorm2d(64, act="relu")                       # an nn.BatchNorm2d whose forward(x, res=None) is the call above
    model, names = convert(model, precision=None)             # swaps the nn.Conv2d / nn.BatchNorm2d layers of a torch model in place

y = act(conv(cat(x, x2), weight) + bias + res) — the operator that is about 99 % of spherical_fusion's work (csrc/omni_conv.hip, f16x3
products on the matrix cores) — and its gradients w.r.t. x, x2, weight, bias and res (csrc/omni_conv_bwd.hip): the same
products, a fixed summation order, no atomics, no host synchronisation.  Only the gradients autograd asks for are computed.

Tensors: x [M,C1,H,W], x2 [M,C2,H,W], weight [Cout,C1+C2,k,k], res and y [M,Cout,Ho,Wo], float32 on an MI355X.  The storage of a
`torch.channels_last` tensor IS the library's NHWC (and that of a channels-last weight its [Cout][(ky,kx,c)]), so such tensors pass through
without a copy and y is channels-last; other formats are converted.  Limits: C1, C2, Cout multiples of 32 (the concat is never
materialised), k = 1 or 3, stride 1 or 2, no groups, no dilation; act "gelu" has no backward and is rejected (apply GELU outside).
No double backward.  There is no CPU path.

`precision` is the arithmetic of the convolution's products, forward and backward of one call alike.  "f16x3" (default):
every operand a pair of halfs, three matrix instructions per product block, fp32-class results.  "f16x1": the mixed precision of training
stacks — an operand is fp16(x) alone (0 below 2^-14), one matrix instruction per block, fp32 accumulation; about 2^-11 relative error per
operand, and an element of the output gradient below 2^-22 of its tensor's largest magnitude counts as 0 (the gradient is scaled into
[2^8, 2^9) on the device before it is rounded: a per-tensor dynamic loss scale).  Master weights, activations, saved tensors and every
gradient stay fp32 in both modes; parameters and state dicts do not change.  Anything else raises ValueError: training has no fp32
product path.  Conv2d, linear, Linear, TransformerBlock and TransformerCascade take the same keyword and expose `.precision`.

y = act(batch_norm(x) + res) (csrc/omni_batchnorm.hip) on x [M,C,H,W], C a multiple of 4: batch statistics over M.H.W with
`training=True` (the running buffers, when given, are updated in place, the variance unbiased), the running statistics with
`training=False` (the usual way to fine-tune).  Gradients w.r.t. x, weight, bias and res; the same rules: fixed summation order (in
double), no atomics, no host synchronisation, only what autograd asks for, channels-last tensors without a copy.  The per-channel
statistics of a BatchNorm3d over [B,C,P,P,N] are those of this operator over [M = B.N, C, P, P].  Not covered: momentum=None (the
cumulative average reads a counter on the host), fp16 storage, double backward.

Statistics across the ranks of a process group (csrc/omni_batchnorm.hip omni_syncbn_*) — data-parallel training, one
process per GPU:

    y = sync_batch_norm(x, weight=None, bias=None, running_mean=None, running_var=None, *, res=None, training=True, momentum=0.1,
                        eps=1e-5, act="none" | "relu", group=None)
    layer = SyncBatchNorm2d(64, act="relu", process_group=None)           # an ops.BatchNorm2d: same parameters, buffers, state dict
    model, names = convert_sync_batchnorm(model, process_group=None, skip=())   # swaps every ops.BatchNorm2d in place

batch_norm over the rows of ALL ranks: each rank sums its own rows in double, one dist.all_gather_records moves the records (2 C + 1
doubles per rank), every rank adds them in rank order — the same bits everywhere — and applies; the backward exchanges its two sums the
same way.  weight and bias receive THIS rank's gradient (dist.sync_gradients adds the ranks').  All ranks must call the operator in the
same order and ask for the same gradients.  Eval mode, world 1 or no process group: batch_norm itself.

The transformer between layer4 and the decoder (csrc/omni_transformer_bwd.hip), under the reference's state-dict names:

    y = layer_norm(x, weight=None, bias=None, eps=1e-5)       # over the last axis of x [..., C], C a multiple of 4, C <= 1024
    y = gelu(x)                                               # exact (erf); x.numel() a multiple of 4
    o = attention(q, kv, batch)                               # q [B.N, 512], kv [B.N, 1024] (k | v) -> [B.N, 512]; 4 heads of 128, N <= 64
    y = linear(x, weight, bias=None, res=None)                # x [rows, K] -> x W^T + bias + res through conv2d (K, out multiples of 32)
    LayerNorm, GELU, Linear                                   # the torch layers' parameters and state dicts
    TransformerBlock(512, 4), TransformerCascade(512, num_patch, depth=6, num_heads=4)

The same rules: fp32, fixed summation orders, no atomics, no host synchronisation, only the gradients autograd asks for.  No backward keeps
anything of its forward but the operator's inputs: layer_norm recomputes its statistics, attention its probabilities, gelu reads x.

The encoder's first operators and the decoder's up-sampling (csrc/omni_stem_conv.hip, omni_maxpool_bwd.hip, omni_upsample_bwd.hip,
DESIGN.md §22):

    y = stem_conv2d(x, weight, bias=None)                     # conv1: 7x7, stride 2, padding 3, x [M,3,H,W] (any H, W), weight [64,3,7,7]
    y = max_pool2d(x)                                         # 3x3, stride 2, padding 1; C a multiple of 4
    y = upsample_bilinear2x(x)                                # F.interpolate(size=(2H, 2W), bilinear, align_corners=False); C a multiple of 4
    StemConv2d(3, 64, 7, stride=2, padding=3, bias=False), MaxPool2d(3, 2, 1), UpsampleBilinear2x()
    model, names = convert(model, spatial=True)               # also swaps the stem and the nn.MaxPool2d(3, 2, 1) layers

stem_conv2d has no activation and no folded normalisation (batch_norm(..., act="relu") follows it) and is differentiable w.r.t. weight
and bias — fp32 FMAs, partial sums per chunk of output tiles, added in double in a fixed order; an x that requires a gradient is
rejected: the image gradient is not built.  max_pool2d and upsample_bilinear2x are differentiable w.r.t. x, both backwards as gathers:
the pool recomputes each window's winner from x (the first greatest element in scan order, torch's rule; no index map), the up-sampling
adds its at most 4 x 4 taps with constant weights.  The same rules: fp32, no atomics, no host synchronisation, only the gradients
autograd asks for, channels-last tensors without a copy (the stem's x is planar, its 37-KiB filter bank is transposed every step).

The two depth heads behind the decoder (csrc/omni_heads_bwd.hip):

    a, c = depth_heads(x, w_pred, b_pred, w_conf, b_conf, *, confidence=True)   # x [M,32,H,W]; w_* [1,32,3,3]; b_* [1]; a, c [M,1,H,W]
    DepthHeads()                                              # holds .pred and .weight_pred as nn.Conv2d(32, 1, 3, padding=1)

a = relu(pred(x)) . sigmoid(weight_pred(x)), c = sigmoid(weight_pred(x)); confidence=False returns (relu(pred(x)), None).  Any H, W; the
biases stay on the device (nothing is read back, the operator can be captured in a graph).  Differentiable w.r.t. x, both weights and
both biases: fp32 FMAs, the weight gradient as per-chunk partial sums added in double in a fixed order.  This backward DOES keep two
planes of its forward, the pre-activations (8 B per pixel): recomputing them would read the 128 B per pixel of x a second time.

The 1x1 convolutions of the point-feature MLPs (csrc/omni_point_conv.hip):

    y = point_conv(x, weight, *, scale=None)                  # weight [16,3,1,1] | [16,5,1,1] | [64,16,1,1], no bias; y [M,Cout,h,w]
    PointConv2d(3 | 5, 16, 1, bias=False), PointConv2d(16, 64, 1, bias=False)      # nn.Conv2d's parameter; forward(x, scale=None)

y = conv2d(x . scale, weight) in fp32 FMAs, three forms and no other: 3 -> 16 on a planar x [Mx,3,h,w] that is repeated M / Mx times
under an optional scale [M,1,h,w] (the unit rays times the re-projected depth of the iterative model: the product is never written),
5 -> 16 on a planar x, 16 -> 64 on a channels-last x.  Differentiable w.r.t. weight (per-chunk partial sums added in double in a fixed
order), scale (a gather per pixel) and, 16 -> 64 only, x; a planar x that requires a gradient raises NotImplementedError.  The same rules:
no atomics, no host synchronisation, only what autograd asks for, nothing kept but the inputs.
"""
import torch

from . import _lib
from ._lib import ptr as _p

ACTS = {"none": 0, "relu": 1}
PRECISIONS = ("f16x3", "f16x1")


def _check_precision(who, precision):
    """The product mode of a convolution, validated before anything is launched."""
    if isinstance(precision, str) and precision in PRECISIONS:
        return precision
    if precision == "fp32":
        raise ValueError(f"{who}: precision='fp32' is not available: training has no fp32 product path (use 'f16x3', fp32-class results)")
    raise ValueError(f"{who}: precision must be 'f16x3' or 'f16x1' (got {precision!r})")
_empty = torch.empty          # every buffer of this module is allocated through this name (tests fill them with NaN)


def _nhwc(t):
    """[M,C,H,W] of any memory format -> the contiguous [M,H,W,C] tensor (a view, without a copy, where t is channels-last)"""
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2)


def _new(shape, dev):
    return _empty(shape, dtype=torch.float32, device=dev)


def _workspace(query, who, *shape, dev):
    """-> (the workspace `query(*shape)` asks for, its bytes); `who` opens the rejection of a shape outside the library's plans"""
    nbytes = query(*shape)
    if nbytes == 0:
        raise ValueError(f"{who} outside the operator's scope")
    return _new((nbytes // 4,), dev), nbytes


def _check_f32_dev(named, optional=()):
    for name, t in named:
        if t is None and name in optional:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (got {t.dtype})")


def _check_args(x, weight, bias, x2, res, stride, padding, act):
    """Every rejection of conv2d, raised before anything is launched.  Returns (k, Ho, Wo)."""
    _check_f32_dev((("x", x), ("weight", weight), ("bias", bias), ("x2", x2), ("res", res)), optional=("bias", "x2", "res"))
    if act not in ACTS:
        if act == "gelu":
            raise ValueError("act='gelu' is not supported: the convolution's backward covers 'none' and 'relu' only (the forward does not "
                             "keep the pre-activation); apply GELU outside")
        raise ValueError(f"act must be 'none' or 'relu' (got {act!r})")
    if x.dim() != 4 or weight.dim() != 4 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [M,C1,H,W] tensor and weight [Cout,C1+C2,k,k] (got {tuple(x.shape)} and {tuple(weight.shape)})")
    M, C1, H, W = x.shape
    C2 = 0
    if x2 is not None:
        if x2.dim() != 4 or x2.shape[0] != M or tuple(x2.shape[2:]) != (H, W):
            raise ValueError(f"x2 must be [M,C2,H,W] with x's M, H, W (got {tuple(x2.shape)} for x {tuple(x.shape)})")
        C2 = x2.shape[1]
    Cout, Cw, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"kernel size must be 1x1 or 3x3 (got {k}x{k2})")
    if C1 % 32 or C2 % 32 or Cout % 32 or C1 == 0 or Cout == 0:
        raise ValueError(f"channel counts must be multiples of 32 (got C1 = {C1}, C2 = {C2}, Cout = {Cout})")
    if Cw != C1 + C2:
        raise ValueError(f"weight has {Cw} input channels, x and x2 have {C1} + {C2}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2 (got {stride!r})")
    if not isinstance(padding, int) or padding < 0 or H + 2 * padding < k or W + 2 * padding < k:
        raise ValueError(f"padding must be an int >= 0 that leaves room for the kernel (got {padding!r})")
    Ho, Wo = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise ValueError(f"bias must be [Cout] = [{Cout}] (got {tuple(bias.shape)})")
    if res is not None and tuple(res.shape) != (M, Cout, Ho, Wo):
        raise ValueError(f"res must have the result's shape {(M, Cout, Ho, Wo)} (got {tuple(res.shape)})")
    return k, Ho, Wo


def _forward_nhwc(x1, x2, w, bias, res, stride, pad, act, precision="f16x3"):
    """x1 [M,H,W,C1], x2 [M,H,W,C2] | None, w [Cout,k,k,C1+C2], res [M,Ho,Wo,Cout] | None, all contiguous -> y [M,Ho,Wo,Cout]"""
    lib = _lib.load()
    M, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    Cout, k = w.shape[0], w.shape[1]
    K = k * k * (C1 + C2)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x1_mode = precision == "f16x1"
    split, conv = ((lib.omni_conv2d_split_weights_f16x1, lib.omni_conv2d_nhwc_f16x1_ws) if x1_mode else
                   (lib.omni_conv2d_split_weights_f16x3, lib.omni_conv2d_nhwc_f16x3_ws))
    w16 = _empty(Cout * K * (1 if x1_mode else 2), dtype=torch.float16, device=x1.device)   # the weights change every step: split on the device
    y = _empty((M, Ho, Wo, Cout), dtype=torch.float32, device=x1.device)
    with torch.cuda.device(x1.device):
        st = _lib.stream_of(x1)
        _lib.check(split(_p(w), _p(w16), Cout, K, st), "conv2d_split_weights")
        _lib.check(conv(_p(x1), _p(x2), _p(w16), _p(bias), _p(res), _p(y), M, H, W, C1, C2, Cout, k, k, stride, pad, ACTS[act], 1, None, 0, st),
                   "conv2d")
    return y


def _backward_nhwc(g, y, x1, x2, w, stride, pad, act, need_x1, need_x2, need_w, precision="f16x3"):
    """The three calls of the backward on contiguous NHWC tensors.  Returns (dx1, dx2, dw, dbias, dz); dz is the residual's gradient."""
    lib = _lib.load()
    bwd_data, bwd_weight = ((lib.omni_conv2d_bwd_data_f16x1, lib.omni_conv2d_bwd_weight_f16x1) if precision == "f16x1" else
                            (lib.omni_conv2d_bwd_data_f16x3, lib.omni_conv2d_bwd_weight_f16x3))
    M, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    Cout, k = w.shape[0], w.shape[1]
    dev = x1.device
    shape = (M, H, W, C1, C2, Cout, k, k, stride, pad)
    ws, nbytes = _workspace(lib.omni_conv2d_bwd_workspace_bytes, f"conv2d backward: shape {shape} is", *shape, dev=dev)
    scale = _empty(2, dtype=torch.float32, device=dev)
    dbias = _empty(Cout, dtype=torch.float32, device=dev)
    relu = act == "relu"
    dz = _empty(tuple(g.shape), dtype=torch.float32, device=dev) if relu else None
    dx1 = dx2 = dw = None
    with torch.cuda.device(dev):
        st = _lib.stream_of(x1)
        _lib.check(lib.omni_conv2d_bwd_epilogue_f32(_p(g), _p(y) if relu else None, _p(dz), _p(dbias), _p(scale), g.numel() // Cout, Cout,
                                                    ACTS[act], _p(ws), nbytes, st), "conv2d_bwd_epilogue")
        if not relu:
            dz = g
        if need_x1 or need_x2:
            dx1 = _empty((M, H, W, C1), dtype=torch.float32, device=dev) if need_x1 else None
            dx2 = _empty((M, H, W, C2), dtype=torch.float32, device=dev) if need_x2 else None
            _lib.check(bwd_data(_p(dz), _p(w), _p(scale), _p(dx1), _p(dx2), *shape, _p(ws), nbytes, st), "conv2d_bwd_data")
        if need_w:
            dw = _empty(tuple(w.shape), dtype=torch.float32, device=dev)
            _lib.check(bwd_weight(_p(dz), _p(x1), _p(x2), _p(scale), _p(dw), *shape, _p(ws), nbytes, st), "conv2d_bwd_weight")
    return dx1, dx2, dw, dbias, dz


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, weight, bias, res, stride, padding, act, precision):
        x1n, x2n, wn, resn = _nhwc(x), _nhwc(x2), _nhwc(weight), _nhwc(res)
        b = bias.contiguous() if bias is not None else None
        y = _forward_nhwc(x1n, x2n, wn, b, resn, stride, padding, act, precision)
        ctx.conf = (stride, padding, act, precision)
        ctx.save_for_backward(x1n, x2n, wn, y if act == "relu" else None)
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x1n, x2n, wn, y = ctx.saved_tensors
        stride, padding, act, precision = ctx.conf
        need = ctx.needs_input_grad
        g = _nhwc(grad_out.to(torch.float32))
        dx1, dx2, dw, dbias, dz = _backward_nhwc(g, y, x1n, x2n, wn, stride, padding, act, need[0], x2n is not None and need[1], need[2],
                                                 precision)
        return (_nchw(dx1), _nchw(dx2), _nchw(dw), dbias if need[3] else None, _nchw(dz) if need[4] else None, None, None, None, None)


def conv2d(x, weight, bias=None, *, x2=None, res=None, stride=1, padding=0, act="none", precision="f16x3"):
    """act(conv(cat(x, x2), weight) + bias + res), differentiable w.r.t. x, x2, weight, bias and res; `precision` ("f16x3" | "f16x1") is
    the product mode of the forward and of the backward (module docstring)."""
    _check_precision("conv2d", precision)
    _check_args(x, weight, bias, x2, res, stride, padding, act)
    return _Conv2d.apply(x, x2, weight, bias, res, stride, padding, act, precision)


class Conv2d(torch.nn.Conv2d):
    """nn.Conv2d with the library's kernels under forward and backward, so that a torch model can swap its layers: the same parameters and
    state dict.  `act` ("none" | "relu") is fused; forward(x, x2=None, res=None) takes the optional second source and residual;
    `precision` ("f16x3" | "f16x1") is the product mode of its forward and backward."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, act="none", precision="f16x3", **kw):
        _check_precision("ops.Conv2d", precision)
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        if self.groups != 1 or tuple(self.dilation) != (1, 1) or self.padding_mode != "zeros" or isinstance(self.padding, str):
            raise ValueError("ops.Conv2d: no groups, no dilation, zero padding given as a number")
        if self.kernel_size[0] != self.kernel_size[1] or self.stride[0] != self.stride[1] or self.padding[0] != self.padding[1]:
            raise ValueError("ops.Conv2d: square kernels, one stride and one padding for both axes")
        if act not in ACTS:
            raise ValueError(f"ops.Conv2d: act must be 'none' or 'relu' (got {act!r}; GELU has no backward here)")
        self.act = act
        self.precision = precision

    def forward(self, x, x2=None, res=None):
        return conv2d(x, self.weight, self.bias, x2=x2, res=res, stride=self.stride[0], padding=self.padding[0], act=self.act,
                      precision=self.precision)

    def extra_repr(self):
        return f"{super().extra_repr()}, act={self.act}, precision={self.precision}"


# ------------------------------------------------------------------------------------------------ batch normalisation
def _check_bn_args(x, weight, bias, running_mean, running_var, res, training, momentum, eps, act, single_ok=False):
    """Every rejection of batch_norm, raised before anything is launched.  single_ok: one value per channel is legal in training mode
    (sync_batch_norm: the other ranks hold more)."""
    _check_f32_dev((("x", x), ("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var), ("res", res)),
                   optional=("weight", "bias", "running_mean", "running_var", "res"))
    if act not in ACTS:
        if act == "gelu":
            raise ValueError("act='gelu' is not supported: the batch normalisation's backward covers 'none' and 'relu' only (the forward "
                             "does not keep the pre-activation); apply GELU outside")
        raise ValueError(f"act must be 'none' or 'relu' (got {act!r})")
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [M,C,H,W] tensor (got {tuple(x.shape)})")
    M, C, H, W = x.shape
    if C % 4:
        raise ValueError(f"the channel count must be a multiple of 4 (got C = {C})")
    for t, name in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and tuple(t.shape) != (C,):
            raise ValueError(f"{name} must be [C] = [{C}] (got {tuple(t.shape)})")
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and t.requires_grad:
            raise ValueError(f"{name} is a buffer, updated in place: it cannot require a gradient")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var come together (got one of them)")
    if res is not None and tuple(res.shape) != tuple(x.shape):
        raise ValueError(f"res must have x's shape {tuple(x.shape)} (got {tuple(res.shape)})")
    if momentum is None:
        raise ValueError("momentum=None (the cumulative average) is not supported: it reads num_batches_tracked on the host")
    if not isinstance(momentum, (int, float)) or not 0.0 <= momentum <= 1.0:
        raise ValueError(f"momentum must be a number in [0, 1] (got {momentum!r})")
    if not isinstance(eps, (int, float)) or not 0.0 < eps < float("inf"):
        raise ValueError(f"eps must be a positive finite number (got {eps!r})")
    if training and M * H * W == 1 and not single_ok:
        raise ValueError(f"Expected more than 1 value per channel when training (got x of shape {tuple(x.shape)})")
    if not training and running_mean is None:
        raise ValueError("training=False needs running_mean and running_var")


def _bn_workspace(lib, rows, C, dev):
    return _workspace(lib.omni_batchnorm_workspace_bytes, f"batch_norm: {rows} rows of {C} channels are", rows, C, dev=dev)


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, training, momentum, eps, act):
        lib = _lib.load()
        xn, resn = _nhwc(x), _nhwc(res)
        w = weight.contiguous() if weight is not None else None
        b = bias.contiguous() if bias is not None else None
        M, H, W, C = xn.shape
        rows, dev = M * H * W, xn.device
        y = _empty((M, H, W, C), dtype=torch.float32, device=dev)
        saved = _empty((2, C), dtype=torch.float32, device=dev)
        ws, nbytes = _bn_workspace(lib, rows, C, dev) if training else (None, 0)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_batchnorm_fwd_f32(_p(xn), _p(resn), _p(w), _p(b), _p(running_mean), _p(running_var), _p(y), _p(saved), rows, C,
                                                  int(training), float(momentum), float(eps), ACTS[act], _p(ws), nbytes, _lib.stream_of(xn)),
                       "batch_norm")
        ctx.conf = (bool(training), act)
        ctx.save_for_backward(xn, w, saved, y if act == "relu" else None)
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        xn, w, saved, y = ctx.saved_tensors
        training, act = ctx.conf
        need_x, need_w, need_b, _, _, need_res = ctx.needs_input_grad[:6]
        relu = act == "relu"
        g = _nhwc(grad_out.to(torch.float32))
        M, H, W, C = xn.shape
        rows, dev = M * H * W, xn.device
        dx = _new((M, H, W, C), dev) if need_x else None
        dres = _new((M, H, W, C), dev) if need_res and relu else None
        dgamma, dbeta = _new((C,), dev) if need_w else None, _new((C,), dev) if need_b else None
        if dx is not None or dres is not None or dgamma is not None or dbeta is not None:
            reduce = need_w or need_b or (training and need_x)
            ws, nbytes = _bn_workspace(lib, rows, C, dev) if reduce else (None, 0)
            with torch.cuda.device(dev):
                _lib.check(lib.omni_batchnorm_bwd_f32(_p(g), _p(xn), _p(y), _p(w), _p(saved), _p(dx), _p(dres), _p(dgamma), _p(dbeta), rows, C,
                                                      int(training), ACTS[act], _p(ws), nbytes, _lib.stream_of(xn)),
                           "batch_norm_bwd" if reduce else "batch_norm_bwd_apply")
        if need_res and not relu:
            dres = g                                                           # the residual's gradient is grad_out itself: no copy
        return (_nchw(dx), dgamma, dbeta, None, None, _nchw(dres), None, None, None, None)


def batch_norm(x, weight=None, bias=None, running_mean=None, running_var=None, *, res=None, training=True, momentum=0.1, eps=1e-5, act="none"):
    """act(batch_norm(x) + res), differentiable w.r.t. x, weight, bias and res; running_mean / running_var are updated in place when
    `training` (module docstring)."""
    _check_bn_args(x, weight, bias, running_mean, running_var, res, training, momentum, eps, act)
    return _BatchNorm.apply(x, weight, bias, running_mean, running_var, res, bool(training), momentum, eps, act)


class BatchNorm2d(torch.nn.BatchNorm2d):
    """nn.BatchNorm2d with the library's kernels under forward and backward: the same parameters, buffers and state dict.  `act`
    ("none" | "relu") is fused; forward(x, res=None) takes the optional residual: y = act(bn(x) + res).  Batch statistics when
    self.training or not track_running_stats, else the running ones."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act="none", **kw):
        if momentum is None:
            raise ValueError("ops.BatchNorm2d: momentum=None (the cumulative average) is not supported: it reads num_batches_tracked on the host")
        if act not in ACTS:
            raise ValueError(f"ops.BatchNorm2d: act must be 'none' or 'relu' (got {act!r}; GELU has no backward here)")
        if num_features % 4:
            raise ValueError(f"ops.BatchNorm2d: the channel count must be a multiple of 4 (got {num_features})")
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats, **kw)
        self.act = act

    def forward(self, x, res=None):
        batch_stats = self.training or not self.track_running_stats
        if self.training and self.track_running_stats:
            self.num_batches_tracked.add_(1)                                   # on the device; nothing reads it here
        return batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, res=res, training=batch_stats,
                          momentum=self.momentum, eps=self.eps, act=self.act)


# ------------------------------------------------------------------------------------------------ statistics across ranks
SYNCBN_MAX_WORLD = 64


def _syncbn_world(group):
    """ranks that share the statistics: those of `group` (None: the default group), 1 without an initialised process group"""
    from . import dist as _dist
    return _dist._group_world(group)


def _check_syncbn_records(who, table, world, C, dev):
    if tuple(table.shape) != (world, 2 * C + 1) or table.dtype != torch.float64 or table.device != dev or not table.is_contiguous():
        raise ValueError(f"{who}: the gathered records must be a contiguous float64 [{world}, {2 * C + 1}] tensor on {dev} "
                         f"(got {table.dtype} {tuple(table.shape)} on {table.device})")


class _SyncBatchNorm(torch.autograd.Function):
    """Training mode, world > 1.  forward: stats -> gather -> apply; backward: reduce -> gather -> apply."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, momentum, eps, act, group, world):
        from . import dist as _dist
        lib = _lib.load()
        xn, resn = _nhwc(x), _nhwc(res)
        w = weight.contiguous() if weight is not None else None
        b = bias.contiguous() if bias is not None else None
        M, H, W, C = xn.shape
        rows, dev = M * H * W, xn.device
        y = _empty((M, H, W, C), dtype=torch.float32, device=dev)
        saved = _empty((2, C), dtype=torch.float32, device=dev)
        rec = _empty((2 * C + 1,), dtype=torch.float64, device=dev)
        ws, nbytes = _bn_workspace(lib, rows, C, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_syncbn_stats_f32(_p(xn), _p(rec), rows, C, _p(ws), nbytes, _lib.stream_of(xn)), "sync_batch_norm_stats")
            table = _dist.all_gather_records(rec, group)
            _check_syncbn_records("sync_batch_norm", table, world, C, dev)
            _lib.check(lib.omni_syncbn_fwd_apply_f32(_p(xn), _p(resn), _p(w), _p(b), _p(table), world, _p(running_mean), _p(running_var), _p(y),
                                                     _p(saved), rows, C, float(momentum), float(eps), ACTS[act], _lib.stream_of(xn)),
                       "sync_batch_norm_apply")
        ctx.conf = (act, group, world)
        ctx.save_for_backward(xn, w, saved, y if act == "relu" else None)
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from . import dist as _dist
        lib = _lib.load()
        xn, w, saved, y = ctx.saved_tensors
        act, group, world = ctx.conf
        need_x, need_w, need_b, _, _, need_res = ctx.needs_input_grad[:6]
        relu = act == "relu"
        g = _nhwc(grad_out.to(torch.float32))
        M, H, W, C = xn.shape
        rows, dev = M * H * W, xn.device
        dx = _new((M, H, W, C), dev) if need_x else None
        dres = _new((M, H, W, C), dev) if need_res and relu else None
        dgamma, dbeta = _new((C,), dev) if need_w else None, _new((C,), dev) if need_b else None
        with torch.cuda.device(dev):
            stream = _lib.stream_of(xn)
            dz_written = False
            table = None
            if need_x or need_w or need_b:
                rec = _empty((2 * C + 1,), dtype=torch.float64, device=dev)
                ws, nbytes = _bn_workspace(lib, rows, C, dev)
                dz_written = dres is not None                                  # the reduce pass writes dZ only where the residual wants it
                _lib.check(lib.omni_syncbn_bwd_reduce_f32(_p(g), _p(xn), _p(y), _p(saved), _p(dres), _p(rec), _p(dgamma), _p(dbeta), rows, C,
                                                          ACTS[act], _p(ws), nbytes, stream), "sync_batch_norm_bwd_reduce")
                if need_x:                                                     # the one collective of the backward: exactly when x needs a gradient
                    table = _dist.all_gather_records(rec, group)
                    _check_syncbn_records("sync_batch_norm (backward)", table, world, C, dev)
            if dx is not None or (dres is not None and not dz_written):
                _lib.check(lib.omni_syncbn_bwd_apply_f32(_p(dres if dz_written else g), _p(None if dz_written else y), _p(xn), _p(w), _p(saved),
                                                         _p(table), world, _p(dx), _p(None if dz_written else dres), rows, C, ACTS[act], stream),
                           "sync_batch_norm_bwd_apply")
        if need_res and not relu:
            dres = g                                                           # the residual's gradient is grad_out itself: no copy
        return (_nchw(dx), dgamma, dbeta, None, None, _nchw(dres), None, None, None, None, None)


def sync_batch_norm(x, weight=None, bias=None, running_mean=None, running_var=None, *, res=None, training=True, momentum=0.1, eps=1e-5,
                    act="none", group=None):
    """batch_norm whose training-mode statistics run over the rows of ALL ranks of `group` (None: the default process group): W ranks of b
    items compute what one device computes on W.b items (invstd = 1 / sqrt(var + eps)).  Forward: this rank's sums of x and
    x^2 in double -> one dist.all_gather_records -> every rank adds the records in rank order and applies; `saved` and the running
    buffers have the same bits on all ranks.  Backward: this rank's sums of dZ and dZ.xhat -> one gather -> dx.  The gradients of weight
    and bias are THIS rank's sums: like every other parameter's they are added by dist.sync_gradients.  The backward's collective runs
    exactly when x needs a gradient, so ALL ranks must ask for the same gradients (and call the operator in the same order), or the
    group hangs.  A rank may hold a single value per channel; the group's total must be more than one (not checked: the count stays on
    the device).  Eval mode, world 1 or no initialised process group: ops.batch_norm itself, the same bits, no collective."""
    world = _syncbn_world(group)
    if not training or world == 1:
        return batch_norm(x, weight, bias, running_mean, running_var, res=res, training=training, momentum=momentum, eps=eps, act=act)
    if world > SYNCBN_MAX_WORLD:
        raise ValueError(f"sync_batch_norm: at most {SYNCBN_MAX_WORLD} ranks share their statistics (the group has {world})")
    _check_bn_args(x, weight, bias, running_mean, running_var, res, True, momentum, eps, act, single_ok=True)
    return _SyncBatchNorm.apply(x, weight, bias, running_mean, running_var, res, momentum, eps, act, group, world)


class SyncBatchNorm2d(BatchNorm2d):
    """ops.BatchNorm2d with ops.sync_batch_norm under it: the same parameters, buffers, state dict, `act=` and forward(x, res=None).
    `process_group=None` is the default group.  In eval mode, at world 1 and without a process group it IS ops.BatchNorm2d."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act="none", process_group=None, **kw):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats, act=act, **kw)
        self.process_group = process_group

    def forward(self, x, res=None):
        batch_stats = self.training or not self.track_running_stats
        if self.training and self.track_running_stats:
            self.num_batches_tracked.add_(1)
        return sync_batch_norm(x, self.weight, self.bias, self.running_mean, self.running_var, res=res, training=batch_stats,
                               momentum=self.momentum, eps=self.eps, act=self.act, group=self.process_group)

    def extra_repr(self):
        return f"{super().extra_repr()}, process_group={self.process_group}"


# ------------------------------------------------------------------------------------------------ the transformer
LN_MAX_C = 1024                # one wave per row, four quads per lane
ATT_DIM, ATT_HEADS, ATT_MAX_N = 512, 4, 64


def _check_ln_width(who, C):
    if C % 4 or C < 4:
        raise ValueError(f"{who}: the normalised axis must be a positive multiple of 4 (got C = {C})")
    if C > LN_MAX_C:
        raise ValueError(f"{who}: at most {LN_MAX_C} values per row (got C = {C})")


def _check_ln_args(x, weight, bias, eps):
    _check_f32_dev((("x", x), ("weight", weight), ("bias", bias)), optional=("weight", "bias"))
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [..., C] tensor (got {tuple(x.shape)})")
    C = x.shape[-1]
    _check_ln_width("layer_norm", C)
    for t, name in ((weight, "weight"), (bias, "bias")):
        if t is not None and tuple(t.shape) != (C,):
            raise ValueError(f"{name} must be [C] = [{C}] (got {tuple(t.shape)})")
    if not isinstance(eps, (int, float)) or not 0.0 < eps < float("inf"):
        raise ValueError(f"eps must be a positive finite number (got {eps!r})")


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _lib.load()
        C = x.shape[-1]
        xc = x.contiguous().view(-1, C)
        w = weight.contiguous() if weight is not None else None
        b = bias.contiguous() if bias is not None else None
        rows, dev = xc.shape[0], xc.device
        y = _empty((rows, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_layernorm_fwd_f32(_p(xc), _p(w), _p(b), _p(y), rows, C, float(eps), _lib.stream_of(xc)), "layer_norm")
        ctx.eps = float(eps)
        ctx.save_for_backward(xc, w)
        return y.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        xc, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        rows, C = xc.shape
        dev = xc.device
        if not (need_x or need_w or need_b):
            return None, None, None, None
        g = grad_out.to(torch.float32).contiguous().view(rows, C)
        dx = _new((rows, C), dev) if need_x else None
        dgamma, dbeta = _new((C,), dev) if need_w else None, _new((C,), dev) if need_b else None
        ws, nbytes = None, 0
        if need_w or need_b:
            ws, nbytes = _workspace(lib.omni_layernorm_bwd_workspace_bytes, f"layer_norm: {rows} rows of {C} values are", rows, C, dev=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_layernorm_bwd_f32(_p(g), _p(xc), _p(w), _p(dx), _p(dgamma), _p(dbeta), rows, C, ctx.eps, _p(ws), nbytes,
                                                  _lib.stream_of(xc)), "layer_norm_bwd")
        return (dx.view(grad_out.shape) if dx is not None else None), dgamma, dbeta, None


def layer_norm(x, weight=None, bias=None, eps=1e-5):
    """Layer normalisation over the last axis of x [..., C] (biased variance, eps inside the root), differentiable w.r.t. x, weight and bias.
    At C = 512 the forward gives the bits of the engine's omni_layernorm512_f32."""
    _check_ln_args(x, weight, bias, eps)
    return _LayerNorm.apply(x, weight, bias, eps)


class LayerNorm(torch.nn.LayerNorm):
    """nn.LayerNorm over ONE axis with the library's kernels under forward and backward: the same parameters and state dict."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, bias=True, **kw):
        shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
        if len(shape) != 1:
            raise ValueError(f"ops.LayerNorm: one normalised axis (got normalized_shape = {shape})")
        _check_ln_width("ops.LayerNorm", shape[0])
        if not isinstance(eps, (int, float)) or not 0.0 < eps < float("inf"):
            raise ValueError(f"ops.LayerNorm: eps must be a positive finite number (got {eps!r})")
        super().__init__(shape, eps=eps, elementwise_affine=elementwise_affine, bias=bias, **kw)

    def forward(self, x):
        return layer_norm(x, self.weight, self.bias, self.eps)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        xc = x.contiguous()
        y = _empty(tuple(xc.shape), dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            _lib.check(lib.omni_gelu_fwd_f32(_p(xc), _p(y), xc.numel(), _lib.stream_of(xc)), "gelu")
        ctx.save_for_backward(xc)                                              # x, not y: the backward needs erf and exp of x
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        xc, = ctx.saved_tensors
        g = grad_out.to(torch.float32).contiguous()
        dx = _empty(tuple(xc.shape), dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            _lib.check(lib.omni_gelu_bwd_f32(_p(g), _p(xc), _p(dx), xc.numel(), _lib.stream_of(xc)), "gelu_bwd")
        return dx


def gelu(x):
    """0.5 x (1 + erf(x / sqrt 2)), the expression of the library's fused GELU epilogues, differentiable; x.numel() a multiple of 4."""
    _check_f32_dev((("x", x),))
    if x.numel() == 0 or x.numel() % 4:
        raise ValueError(f"gelu: the element count must be a positive multiple of 4 (got {x.numel()})")
    return _Gelu.apply(x)


class GELU(torch.nn.Module):
    def forward(self, x):
        return gelu(x)


def _check_attention_args(q, kv, batch):
    _check_f32_dev((("q", q), ("kv", kv)))
    if not isinstance(batch, int) or isinstance(batch, bool) or batch < 1:
        raise ValueError(f"batch must be a positive int (got {batch!r})")
    if q.dim() != 2 or kv.dim() != 2 or q.shape[0] == 0:
        raise ValueError(f"q must be a non-empty [B.N, 512] tensor and kv [B.N, 1024] (got {tuple(q.shape)} and {tuple(kv.shape)})")
    if q.shape[1] != ATT_DIM or kv.shape[1] != 2 * ATT_DIM:
        raise ValueError(f"attention: the model width is 512, four heads of 128: q [B.N, 512], kv [B.N, 1024] (got {tuple(q.shape)} and "
                         f"{tuple(kv.shape)})")
    rows = q.shape[0]
    if kv.shape[0] != rows or rows % batch:
        raise ValueError(f"attention: q and kv must have the same B.N rows, a multiple of batch = {batch} (got {rows} and {kv.shape[0]})")
    if rows // batch > ATT_MAX_N:
        raise ValueError(f"attention: at most {ATT_MAX_N} tokens per item (got N = {rows // batch})")
    return rows // batch


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, batch, N):
        lib = _lib.load()
        qc, kvc = q.contiguous(), kv.contiguous()
        out = _empty((batch * N, ATT_DIM), dtype=torch.float32, device=qc.device)
        with torch.cuda.device(qc.device):
            _lib.check(lib.omni_attention_f32(_p(qc), _p(kvc), _p(out), batch, N, _lib.stream_of(qc)), "attention")
        ctx.conf = (batch, N)
        ctx.save_for_backward(qc, kvc)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        qc, kvc = ctx.saved_tensors
        batch, N = ctx.conf
        need_q, need_kv = ctx.needs_input_grad[:2]
        if not (need_q or need_kv):
            return None, None, None, None
        dev = qc.device
        g = grad_out.to(torch.float32).contiguous()
        dq = _empty((batch * N, ATT_DIM), dtype=torch.float32, device=dev) if need_q else None
        dkv = _empty((batch * N, 2 * ATT_DIM), dtype=torch.float32, device=dev) if need_kv else None
        ws, nbytes = None, 0
        if need_kv:
            ws, nbytes = _workspace(lib.omni_attention_bwd_workspace_bytes, f"attention: {batch} items of {N} tokens are", batch, N, dev=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_attention_bwd_f32(_p(qc), _p(kvc), _p(g), _p(dq), _p(dkv), batch, N, _p(ws), nbytes, _lib.stream_of(qc)),
                       "attention_bwd")
        return dq, dkv, None, None


def attention(q, kv, batch):
    """softmax(q k^T / sqrt(128)) v per item and head: q [B.N, 512], kv [B.N, 1024] (k at column 0, v at column 512), B = batch ->
    [B.N, 512].  The forward is the engine's omni_attention_f32; differentiable w.r.t. q and kv."""
    N = _check_attention_args(q, kv, batch)
    return _Attention.apply(q, kv, batch, N)


def linear(x, weight, bias=None, res=None, precision="f16x3"):
    """x W^T + bias + res for x [rows, K], weight [out, K], res [rows, out]: conv2d on [rows, K, 1, 1] (its kernels, its backward, its
    checks: K and out multiples of 32; its `precision`)."""
    _check_precision("linear", precision)
    _check_f32_dev((("x", x), ("weight", weight), ("bias", bias), ("res", res)), optional=("bias", "res"))
    if x.dim() != 2 or weight.dim() != 2 or x.numel() == 0:
        raise ValueError(f"x must be a non-empty [rows, K] tensor and weight [out, K] (got {tuple(x.shape)} and {tuple(weight.shape)})")
    rows, out = x.shape[0], weight.shape[0]
    if res is not None and tuple(res.shape) != (rows, out):
        raise ValueError(f"res must have the result's shape {(rows, out)} (got {tuple(res.shape)})")
    y = conv2d(x[:, :, None, None], weight[:, :, None, None], bias, res=res[:, :, None, None] if res is not None else None,
               precision=precision)
    return y.reshape(rows, out)


class Linear(torch.nn.Linear):
    """nn.Linear with the convolution's kernels under forward and backward; forward(x [..., K], res=None) adds the residual in the kernel.
    `precision` ("f16x3" | "f16x1") is the convolution's product mode."""

    def __init__(self, in_features, out_features, bias=True, precision="f16x3", **kw):
        _check_precision("ops.Linear", precision)
        super().__init__(in_features, out_features, bias=bias, **kw)
        self.precision = precision

    def extra_repr(self):
        return f"{super().extra_repr()}, precision={self.precision}"

    def forward(self, x, res=None):
        if not isinstance(x, torch.Tensor) or x.dim() < 1:
            raise ValueError("x must be a tensor on an MI355X device; there is no CPU path")
        lead = x.shape[:-1]
        y = linear(x.reshape(-1, x.shape[-1]), self.weight, self.bias, res.reshape(-1, self.out_features) if res is not None else None,
                   precision=self.precision)
        return y.reshape(*lead, self.out_features)


def _check_transformer_conf(who, dim, num_heads):
    if dim != ATT_DIM or num_heads != ATT_HEADS:
        raise ValueError(f"{who}: the attention kernels cover width 512 with 4 heads of 128 (got dim = {dim}, num_heads = {num_heads})")


class _AttentionLayers(torch.nn.Module):
    def __init__(self, dim, precision="f16x3"):
        super().__init__()
        self.q, self.kv = Linear(dim, dim, bias=False, precision=precision), Linear(dim, 2 * dim, bias=False, precision=precision)
        self.proj = Linear(dim, dim, precision=precision)


class _MlpLayers(torch.nn.Module):
    def __init__(self, dim, precision="f16x3"):
        super().__init__()
        self.fc1, self.fc2 = Linear(dim, 4 * dim, precision=precision), Linear(4 * dim, dim, precision=precision)


class TransformerBlock(torch.nn.Module):
    """The reference's pre-LN block under its parameter names (norm1, attn.q, attn.kv, attn.proj, norm2, mlp.fc1, mlp.fc2):
    x + proj(attention(q(norm1 x), kv(norm1 x))), then x + fc2(gelu(fc1(norm2 x))); the two additions are the `res` of proj and fc2.
    forward(x [B.N, 512], batch = B).  Dropout and drop-path are identity in the reference's configuration and are not built.
    `precision` is the product mode of the five linear layers; layer norm, attention and GELU are fp32 in both modes."""

    def __init__(self, dim=ATT_DIM, num_heads=ATT_HEADS, precision="f16x3"):
        _check_transformer_conf("ops.TransformerBlock", dim, num_heads)
        _check_precision("ops.TransformerBlock", precision)
        super().__init__()
        self.precision = precision
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn = _AttentionLayers(dim, precision)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        self.mlp = _MlpLayers(dim, precision)

    def extra_repr(self):
        return f"precision={self.precision}"

    def forward(self, x, batch):
        y = self.norm1(x)
        a = attention(self.attn.q(y), self.attn.kv(y), batch)
        x = self.attn.proj(a, res=x)
        return self.mlp.fc2(gelu(self.mlp.fc1(self.norm2(x))), res=x)


class TransformerCascade(torch.nn.Module):
    """The reference's Transformer_cascade under its parameter names (pos_emb [1, num_patch, 512], layer.{i}, encoder_norm with eps 1e-6):
    forward(x [bs, num_patch, 512]) -> [bs, num_patch, 512].  The `transformer.*` entries of a spherical_fusion state dict load into it."""

    def __init__(self, emb_dims=ATT_DIM, num_patch=18, depth=6, num_heads=ATT_HEADS, precision="f16x3"):
        _check_transformer_conf("ops.TransformerCascade", emb_dims, num_heads)
        _check_precision("ops.TransformerCascade", precision)
        if not isinstance(num_patch, int) or not 1 <= num_patch <= ATT_MAX_N:
            raise ValueError(f"ops.TransformerCascade: 1 to {ATT_MAX_N} patches (got num_patch = {num_patch!r})")
        if not isinstance(depth, int) or depth < 1:
            raise ValueError(f"ops.TransformerCascade: depth >= 1 (got {depth!r})")
        super().__init__()
        self.precision = precision
        self.layer = torch.nn.ModuleList([TransformerBlock(emb_dims, num_heads, precision) for _ in range(depth)])
        self.encoder_norm = LayerNorm(emb_dims, eps=1e-6)
        self.pos_emb = torch.nn.Parameter(torch.zeros(1, num_patch, emb_dims))
        torch.nn.init.normal_(self.pos_emb, std=0.02)

    def extra_repr(self):
        return f"precision={self.precision}"

    def forward(self, x):
        _check_f32_dev((("x", x),))
        if x.dim() != 3 or tuple(x.shape[1:]) != tuple(self.pos_emb.shape[1:]) or x.shape[0] == 0:
            raise ValueError(f"x must be [bs, {self.pos_emb.shape[1]}, {self.pos_emb.shape[2]}] (got {tuple(x.shape)})")
        bs, N, C = x.shape
        h = (x + self.pos_emb).reshape(bs * N, C)
        for blk in self.layer:
            h = blk(h, bs)
        return self.encoder_norm(h).reshape(bs, N, C)


# ------------------------------------------------------------------------------------------------ stem, max-pool, up-sampling
STEM_GEOMETRY = "a 7x7 convolution at stride 2 with padding 3 from 3 to 64 channels"
POOL_GEOMETRY = "a 3x3 max-pool at stride 2 with padding 1"


def _check_stem_args(x, weight, bias):
    """Every rejection of stem_conv2d, raised before anything is launched."""
    _check_f32_dev((("x", x), ("weight", weight), ("bias", bias)), optional=("bias",))
    if weight.dim() != 4 or tuple(weight.shape) != (64, 3, 7, 7):
        raise ValueError(f"stem_conv2d: weight must be [64,3,7,7]: {STEM_GEOMETRY} is the only geometry built (got {tuple(weight.shape)})")
    if x.dim() != 4 or x.numel() == 0 or x.shape[1] != 3:
        raise ValueError(f"stem_conv2d: x must be a non-empty [M,3,H,W] tensor (got {tuple(x.shape)})")
    if bias is not None and tuple(bias.shape) != (64,):
        raise ValueError(f"stem_conv2d: bias must be [64] (got {tuple(bias.shape)})")
    if x.requires_grad:
        raise ValueError("stem_conv2d: x requires a gradient, but the image gradient of the stem is not built (no training script asks "
                         "for it); pass x.detach()")


class _StemConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        xc = x.contiguous()                                                    # planar [M,3,H,W]
        wk = weight.permute(2, 3, 1, 0).contiguous()                           # [7,7,3,64] = the library's [147][64]; 37 KiB, every step
        b = bias.contiguous() if bias is not None else None
        M, _, H, W = xc.shape
        y = _empty((M, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            _lib.check(lib.omni_stem_conv_fwd_f32(_p(xc), _p(wk), _p(b), _p(y), M, H, W, _lib.stream_of(xc)), "stem_conv2d")
        ctx.has_bias = bias is not None
        ctx.save_for_backward(xc)
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        xc, = ctx.saved_tensors
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_w or need_b):
            return None, None, None
        M, _, H, W = xc.shape
        dev = xc.device
        g = _nhwc(grad_out.to(torch.float32))
        ws, nbytes = _workspace(lib.omni_stem_conv_bwd_workspace_bytes, f"stem_conv2d backward: x of shape {tuple(xc.shape)} is", M, H, W,
                                dev=dev)
        dw = _empty((7, 7, 3, 64), dtype=torch.float32, device=dev) if need_w else None
        db = _empty(64, dtype=torch.float32, device=dev) if need_b else None
        with torch.cuda.device(dev):
            _lib.check(lib.omni_stem_conv_bwd_weight_f32(_p(g), _p(xc), _p(dw), _p(db), M, H, W, _p(ws), nbytes, _lib.stream_of(xc)),
                       "stem_conv2d_bwd_weight")
        return None, (dw.permute(3, 2, 0, 1) if need_w else None), db            # a view of [147][64]: no copy


def stem_conv2d(x, weight, bias=None):
    """conv(x, weight) + bias for the encoder's conv1 alone — 7x7, stride 2, padding 3, x [M,3,H,W] (any H, W), weight [64,3,7,7] ->
    channels-last [M,64,Ho,Wo]; no activation, no folded normalisation.  Differentiable w.r.t. weight and bias, not w.r.t. x."""
    _check_stem_args(x, weight, bias)
    return _StemConv2d.apply(x, weight, bias)


def _stem_in_scope(m):
    return (m.in_channels == 3 and m.out_channels == 64 and tuple(m.kernel_size) == (7, 7) and tuple(m.stride) == (2, 2)
            and not isinstance(m.padding, str) and tuple(m.padding) == (3, 3) and m.groups == 1 and tuple(m.dilation) == (1, 1)
            and m.padding_mode == "zeros")


class StemConv2d(torch.nn.Conv2d):
    """nn.Conv2d(3, 64, 7, stride=2, padding=3) with the library's kernels under forward and backward: the same parameters and state dict.
    Any other geometry is rejected."""

    def __init__(self, in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False, **kw):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias, **kw)
        if not _stem_in_scope(self):
            raise ValueError(f"ops.StemConv2d: {STEM_GEOMETRY}, no groups, no dilation, zero padding, is the only geometry built (got {self})")

    def forward(self, x):
        return stem_conv2d(x, self.weight, self.bias)


def _check_spatial_x(who, x):
    _check_f32_dev((("x", x),))
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"{who}: x must be a non-empty [M,C,H,W] tensor (got {tuple(x.shape)})")
    if x.shape[1] % 4:
        raise ValueError(f"{who}: the channel count must be a multiple of 4 (got C = {x.shape[1]})")


class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        xn = _nhwc(x)
        M, H, W, C = xn.shape
        y = _empty((M, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32, device=xn.device)
        with torch.cuda.device(xn.device):
            _lib.check(lib.omni_maxpool3x3s2_f32(_p(xn), _p(y), M, H, W, C, _lib.stream_of(xn)), "max_pool2d")
        ctx.save_for_backward(xn)                                              # the winners are recomputed from x: no index map
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None
        lib = _lib.load()
        xn, = ctx.saved_tensors
        M, H, W, C = xn.shape
        g = _nhwc(grad_out.to(torch.float32))
        dx = _empty((M, H, W, C), dtype=torch.float32, device=xn.device)
        with torch.cuda.device(xn.device):
            _lib.check(lib.omni_maxpool3x3s2_bwd_f32(_p(g), _p(xn), _p(dx), M, H, W, C, _lib.stream_of(xn)), "max_pool2d_bwd")
        return _nchw(dx)


def max_pool2d(x):
    """F.max_pool2d(x, 3, 2, 1) on x [M,C,H,W], C a multiple of 4, differentiable w.r.t. x: the gradient of a window goes to its first
    greatest element in scan order, as in torch.  (A NaN is dropped, not propagated: DESIGN.md §7.)"""
    _check_spatial_x("max_pool2d", x)
    return _MaxPool2d.apply(x)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _pool_in_scope(m):
    return (_pair(m.kernel_size) == (3, 3) and _pair(m.stride) == (2, 2) and _pair(m.padding) == (1, 1) and _pair(m.dilation) == (1, 1)
            and not m.ceil_mode and not m.return_indices)


class MaxPool2d(torch.nn.MaxPool2d):
    """nn.MaxPool2d(3, 2, 1) with the library's kernels under forward and backward.  Any other geometry is rejected."""

    def __init__(self, kernel_size=3, stride=2, padding=1, **kw):
        super().__init__(kernel_size, stride=stride, padding=padding, **kw)
        if not _pool_in_scope(self):
            raise ValueError(f"ops.MaxPool2d: {POOL_GEOMETRY}, dilation 1, ceil_mode=False, return_indices=False, is the only geometry "
                             f"built (got {self})")

    def forward(self, x):
        return max_pool2d(x)


class _UpsampleBilinear2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        xn = _nhwc(x)
        M, H, W, C = xn.shape
        y = _empty((M, 2 * H, 2 * W, C), dtype=torch.float32, device=xn.device)
        with torch.cuda.device(xn.device):
            _lib.check(lib.omni_upsample_bilinear_f32(_p(xn), _p(y), M, H, W, C, 2 * H, 2 * W, _lib.stream_of(xn)), "upsample_bilinear2x")
        ctx.shape = (M, H, W, C)                                               # the operator is linear: its backward reads grad_out alone
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None
        lib = _lib.load()
        M, H, W, C = ctx.shape
        g = _nhwc(grad_out.to(torch.float32))
        dx = _empty((M, H, W, C), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(lib.omni_upsample_bilinear2x_bwd_f32(_p(g), _p(dx), M, H, W, C, _lib.stream_of(g)), "upsample_bilinear2x_bwd")
        return _nchw(dx)


def upsample_bilinear2x(x):
    """F.interpolate(x, size=(2H, 2W), mode="bilinear", align_corners=False) on x [M,C,H,W], C a multiple of 4, differentiable w.r.t. x."""
    _check_spatial_x("upsample_bilinear2x", x)
    return _UpsampleBilinear2x.apply(x)


class UpsampleBilinear2x(torch.nn.Module):
    def forward(self, x):
        return upsample_bilinear2x(x)


# ------------------------------------------------------------------------------------------------ the depth heads
HEADS_C = 32


def _check_heads_args(x, w_pred, b_pred, w_conf, b_conf):
    """Every rejection of depth_heads, raised before anything is launched."""
    _check_f32_dev((("x", x), ("w_pred", w_pred), ("b_pred", b_pred), ("w_conf", w_conf), ("b_conf", b_conf)))
    if len({t.device for t in (x, w_pred, b_pred, w_conf, b_conf)}) != 1:
        raise ValueError("depth_heads: x, the weights and the biases must be on one device")
    if x.dim() != 4 or x.numel() == 0 or x.shape[1] != HEADS_C:
        raise ValueError(f"depth_heads: x must be a non-empty [M,{HEADS_C},H,W] tensor (got {tuple(x.shape)})")
    for t, name in ((w_pred, "w_pred"), (w_conf, "w_conf")):
        if tuple(t.shape) != (1, HEADS_C, 3, 3):
            raise ValueError(f"depth_heads: {name} must be [1,{HEADS_C},3,3]: a 3x3 convolution from {HEADS_C} channels to 1 with padding 1 "
                             f"is the only geometry built (got {tuple(t.shape)})")
    for t, name in ((b_pred, "b_pred"), (b_conf, "b_conf")):
        if tuple(t.shape) != (1,):
            raise ValueError(f"depth_heads: {name} must be [1] (got {tuple(t.shape)})")
    if x.shape[0] * x.shape[2] * x.shape[3] >= 1 << 31:
        raise ValueError(f"depth_heads: x of shape {tuple(x.shape)} has 2^31 pixels or more")


class _DepthHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_pred, b_pred, w_conf, b_conf, confidence):
        lib = _lib.load()
        xn = _nhwc(x)
        M, H, W, _ = xn.shape
        dev = xn.device
        w, bias = _new((2, 3, 3, HEADS_C), dev), _new((2,), dev)              # [2][9][32] and the two biases, packed on the device (2.3 KB)
        w[0:1].copy_(w_pred.detach().permute(0, 2, 3, 1)); w[1:2].copy_(w_conf.detach().permute(0, 2, 3, 1))
        bias[0:1].copy_(b_pred.detach()); bias[1:2].copy_(b_conf.detach())
        pending = any(ctx.needs_input_grad[:5])
        a, c = _new((M, 1, H, W), dev), _new((M, 1, H, W), dev) if confidence else None
        p, q = (_new((M, H, W), dev), _new((M, H, W), dev)) if pending else (None, None)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_depth_heads_fwd_f32(_p(xn), _p(w), _p(bias), _p(a), _p(c), _p(p), _p(q), M, H, W, int(confidence),
                                                    _lib.stream_of(xn)), "depth_heads")
        ctx.confidence = confidence
        ctx.set_materialize_grads(False)
        if pending:
            ctx.save_for_backward(xn, w, p, q)                                 # p and q are kept: 8 B per pixel against 128 B of x
        return (a, c) if confidence else a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_a, grad_c=None):
        need = ctx.needs_input_grad
        conf = ctx.confidence
        need_x, need_w, need_b = need[0], need[1] or (conf and need[3]), need[2] or (conf and need[4])
        if (grad_a is None and grad_c is None) or not (need_x or need_w or need_b):
            return (None,) * 6
        lib = _lib.load()
        xn, w, p, q = ctx.saved_tensors
        M, H, W, _ = xn.shape
        dev = xn.device
        ga = grad_a.to(torch.float32).contiguous() if grad_a is not None else None
        gc = grad_c.to(torch.float32).contiguous() if grad_c is not None else None
        ws, nbytes = _workspace(lib.omni_depth_heads_bwd_workspace_bytes, f"depth_heads backward: x of shape {(M, HEADS_C, H, W)} is", M, H, W,
                                dev=dev)
        dx = _new((M, H, W, HEADS_C), dev) if need_x else None
        dw = _new((2, 3, 3, HEADS_C), dev) if need_w else None
        db = _new((2,), dev) if need_b else None
        with torch.cuda.device(dev):
            _lib.check(lib.omni_depth_heads_bwd_f32(_p(ga), _p(gc), _p(p), _p(q), _p(xn), _p(w), _p(dx), _p(dw), _p(db), M, H, W, int(conf),
                                                    _p(ws), nbytes, _lib.stream_of(xn)), "depth_heads_bwd")
        live = conf or gc is not None                                          # without the product and without grad_c nothing reaches weight_pred
        return (_nchw(dx), dw[0:1].permute(0, 3, 1, 2) if need[1] else None, db[0:1] if need[2] else None,
                dw[1:2].permute(0, 3, 1, 2) if need[3] and live else None, db[1:2] if need[4] and live else None, None)


def depth_heads(x, w_pred, b_pred, w_conf, b_conf, *, confidence=True):
    """The two heads of spherical_fusion: p = conv3x3(x, w_pred) + b_pred, q = conv3x3(x, w_conf) + b_conf (padding 1) on x [M,32,H,W], any
    H, W; returns (a, c) [M,1,H,W] with a = relu(p) . sigmoid(q), c = sigmoid(q), or (relu(p), None) with confidence=False.
    Differentiable w.r.t. x, both weights [1,32,3,3] and both biases [1], which stay on the device."""
    _check_heads_args(x, w_pred, b_pred, w_conf, b_conf)
    if confidence:
        return _DepthHeads.apply(x, w_pred, b_pred, w_conf, b_conf, True)
    return _DepthHeads.apply(x, w_pred, b_pred, w_conf, b_conf, False), None


class DepthHeads(torch.nn.Module):
    """The heads under the reference's parameter names: .pred and .weight_pred, each an nn.Conv2d(32, 1, 3, padding=1) that holds the
    parameters; forward(x, confidence=True) is depth_heads."""

    def __init__(self):
        super().__init__()
        self.pred = torch.nn.Conv2d(HEADS_C, 1, 3, padding=1)
        self.weight_pred = torch.nn.Conv2d(HEADS_C, 1, 3, padding=1)

    def forward(self, x, confidence=True):
        return depth_heads(x, self.pred.weight, self.pred.bias, self.weight_pred.weight, self.weight_pred.bias, confidence=confidence)


# ------------------------------------------------------------------------------------------------ the point-feature MLPs
POINT_FORMS = {(3, 16): "planar", (5, 16): "planar", (16, 64): "channels_last"}      # (Cin, Cout) -> the layout of x the kernel reads


def _check_point_args(x, weight, scale):
    """Every rejection of point_conv, raised before anything is launched: shapes first, then gradients, dtypes and devices.  Returns
    (Mx, M, h, w, Cin, Cout)."""
    for name, t in (("x", x), ("weight", weight)) + ((("scale", scale),) if scale is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"point_conv: {name} must be a tensor")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or tuple(weight.shape[1::-1]) not in POINT_FORMS:
        raise ValueError(f"point_conv: weight must be [16,3,1,1], [16,5,1,1] or [64,16,1,1]: 1x1 convolutions from 3 or 5 to 16 and from 16 to 64 "
                         f"channels are the only ones built (got {tuple(weight.shape)})")
    Cout, Cin = weight.shape[:2]
    if x.dim() != 4 or x.numel() == 0 or x.shape[1] != Cin:
        raise ValueError(f"point_conv: x must be a non-empty [Mx,{Cin},h,w] tensor for a weight {tuple(weight.shape)} (got {tuple(x.shape)})")
    Mx, _, h, w = x.shape
    M = Mx
    if scale is not None:
        if Cin != 3:
            raise ValueError(f"point_conv: only the 3 -> 16 form takes a scale (weight {tuple(weight.shape)})")
        if scale.dim() != 4 or scale.shape[1] != 1 or tuple(scale.shape[2:]) != (h, w) or scale.shape[0] == 0 or scale.shape[0] % Mx:
            raise ValueError(f"point_conv: scale must be [M,1,{h},{w}] with M a multiple of x's {Mx} items (got {tuple(scale.shape)})")
        M = scale.shape[0]
    if M * h * w >= 1 << 31:
        raise ValueError(f"point_conv: {M} maps of {h} x {w} have 2^31 pixels or more")
    if x.requires_grad and torch.is_grad_enabled() and POINT_FORMS[(Cin, Cout)] == "planar":
        raise NotImplementedError(f"point_conv: x requires a gradient, but the planar (broadcast) {Cin} -> {Cout} form has none w.r.t. x — the "
                                  f"rays and the patch centres are constants; pass x.detach()")
    for name, t in (("x", x), ("weight", weight), ("scale", scale)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"point_conv: {name} must be float32 (got {t.dtype})")
    _check_f32_dev((("x", x), ("weight", weight), ("scale", scale)), optional=("scale",))
    if len({t.device for t in (x, weight, scale) if t is not None}) != 1:
        raise ValueError("point_conv: x, weight and scale must be on one device")
    return Mx, M, h, w, Cin, Cout


class _PointConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, scale):
        lib = _lib.load()
        Cout, Cin = weight.shape[:2]
        xs = _nhwc(x) if POINT_FORMS[(Cin, Cout)] == "channels_last" else x.contiguous()      # the storage the form reads: no copy where x has it
        wc = weight.detach().contiguous()                                      # [Cout,Cin,1,1]: the library's [Cout][Cin]
        sc = scale.contiguous() if scale is not None else None
        Mx, h, w = x.shape[0], x.shape[2], x.shape[3]
        M = sc.shape[0] if sc is not None else Mx
        dev = x.device
        y = _new((M, h, w, Cout), dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_point_conv_fwd_f32(_p(xs), _p(wc), _p(sc), _p(y), Mx, M, h * w, Cin, Cout, _lib.stream_of(y)), "point_conv")
        ctx.dims = (Mx, M, h, w, Cin, Cout)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xs, wc, sc)                                  # the inputs, nothing of the forward
        return _nchw(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        need_x, need_w, need_s = ctx.needs_input_grad
        if not (need_x or need_w or need_s):
            return None, None, None
        lib = _lib.load()
        xs, wc, sc = ctx.saved_tensors
        Mx, M, h, w, Cin, Cout = ctx.dims
        dev = xs.device
        g = _nhwc(grad_out.to(torch.float32))
        dx = _new((M, h, w, Cin), dev) if need_x else None
        dw = _new((Cout, Cin, 1, 1), dev) if need_w else None
        ds = _new((M, 1, h, w), dev) if need_s else None
        ws, nbytes = (None, 0)
        if need_w:
            ws, nbytes = _workspace(lib.omni_point_conv_bwd_workspace_bytes, f"point_conv backward: {M} maps of {h} x {w} are", M, h * w, Cin, Cout,
                                    dev=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.omni_point_conv_bwd_f32(_p(g), _p(xs), _p(wc), _p(sc), _p(dx), _p(dw), _p(ds), Mx, M, h * w, Cin, Cout, _p(ws), nbytes,
                                                   _lib.stream_of(g)), "point_conv_bwd")
        return _nchw(dx), dw, ds


def point_conv(x, weight, *, scale=None):
    """A 1x1 convolution of the point-feature MLPs without bias: y = conv2d(x . scale, weight), in three forms and no other.
    weight [16,3,1,1]: x [Mx,3,h,w] planar, repeated M / Mx times under an optional scale [M,1,h,w] (the unit rays times the depth of
    model/spherical_model_iterative.py:387-393); weight [16,5,1,1]: x [M,5,h,w] planar; weight [64,16,1,1]: x [M,16,h,w] channels-last.
    y [M,Cout,h,w] is channels-last, the layout batch_norm takes without a copy.  Differentiable w.r.t. weight, scale and — the 16 -> 64
    form only — x; a planar x that requires a gradient raises NotImplementedError."""
    _check_point_args(x, weight, scale)
    return _PointConv.apply(x, weight, scale)


class PointConv2d(torch.nn.Conv2d):
    """nn.Conv2d(3 | 5, 16, 1, bias=False) or nn.Conv2d(16, 64, 1, bias=False) — the same Parameter [Cout,Cin,1,1] under the same name —
    whose forward(x, scale=None) is point_conv."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=False, **kw):
        if (in_channels, out_channels) not in POINT_FORMS or bias or tuple(_pair(kernel_size)) != (1, 1) \
                or tuple(_pair(stride)) != (1, 1) or tuple(_pair(padding)) != (0, 0):
            raise ValueError("ops.PointConv2d: 1x1 convolutions from 3 or 5 to 16 and from 16 to 64 channels, stride 1, no padding, no bias, are "
                             "the only ones built")
        super().__init__(in_channels, out_channels, 1, bias=False, **kw)

    def forward(self, x, scale=None):
        return point_conv(x, self.weight, scale=scale)


def _conv_in_scope(m):
    return (m.groups == 1 and tuple(m.dilation) == (1, 1) and m.padding_mode == "zeros" and not isinstance(m.padding, str)
            and m.kernel_size[0] == m.kernel_size[1] and m.kernel_size[0] in (1, 3) and m.stride[0] == m.stride[1] and m.stride[0] in (1, 2)
            and m.padding[0] == m.padding[1] and m.in_channels % 32 == 0 and m.out_channels % 32 == 0)


def _swap_class(old, cls):
    """A `cls` layer that holds old's own Parameter and buffer objects (and hooks, mode, dtype): no tensor is copied or re-created."""
    new = cls.__new__(cls)
    new.__dict__.update(old.__dict__)
    for reg in ("_parameters", "_buffers", "_modules"):
        new.__dict__[reg] = dict(old.__dict__[reg])
    if cls in (Conv2d, BatchNorm2d):
        new.act = "none"
    return new


def convert(module, spatial=False, precision=None):
    """Replaces, in place, every nn.Conv2d inside Conv2d's scope (module docstring) and every nn.BatchNorm2d (channels a multiple of 4, a
    numeric momentum) by the class of this module, act="none".  The new layers hold the SAME Parameter and buffer objects, so an optimiser
    built before or after sees the same tensors and the state dict keeps its keys.  Everything else — a 3-channel stem, grouped or dilated
    convolutions, momentum=None layers, subclasses — is left alone.  With `spatial=True` the stem, nn.Conv2d(3, 64, 7, stride=2,
    padding=3) (no groups, no dilation, zero padding; a bias is allowed), becomes a StemConv2d and nn.MaxPool2d(3, 2, 1) (dilation 1,
    ceil_mode=False, return_indices=False) a MaxPool2d as well.  `precision` ("f16x3" | "f16x1"; None = the default, "f16x3") is the
    product mode of every Conv2d created.  Returns (module, [the names replaced])."""
    precision = _check_precision("convert", "f16x3" if precision is None else precision)

    def swapped(m):
        if type(m) is torch.nn.Conv2d and _conv_in_scope(m):
            new = _swap_class(m, Conv2d)
            new.precision = precision
            return new
        if type(m) is torch.nn.BatchNorm2d and m.momentum is not None and m.num_features % 4 == 0:
            return _swap_class(m, BatchNorm2d)
        if spatial and type(m) is torch.nn.Conv2d and _stem_in_scope(m):
            return _swap_class(m, StemConv2d)
        if spatial and type(m) is torch.nn.MaxPool2d and _pool_in_scope(m):
            return _swap_class(m, MaxPool2d)
        return None

    root = swapped(module)
    if root is not None:
        return root, [""]
    names = []
    for pname, parent in list(module.named_modules()):
        for cname, child in list(parent.named_children()):
            new = swapped(child)
            if new is not None:
                setattr(parent, cname, new)
                names.append(f"{pname}.{cname}" if pname else cname)
    return module, names


def convert_sync_batchnorm(module, process_group=None, skip=()):
    """Replaces, in place, every ops.BatchNorm2d by an ops.SyncBatchNorm2d of `process_group` (None: the default group); an
    nn.BatchNorm2d in convert's scope goes through convert first (the module's convolutions are NOT touched here).  The new layer holds the
    SAME Parameter and buffer objects, hooks, mode and `act`: the state dict keeps its keys, order and tensors.  `skip`: name prefixes
    ("mlp_points" covers "mlp_points" and "mlp_points.1", not "mlp_points1") whose layers stay unsynchronised — those whose input is
    identical on every rank.  Layers that are SyncBatchNorm2d already are left alone: a second call replaces nothing.  Returns
    (module, [the names replaced])."""
    if isinstance(skip, str):
        raise ValueError(f"convert_sync_batchnorm: skip is a sequence of name prefixes, not a string (got {skip!r})")
    skip = tuple(skip)
    if not all(isinstance(s, str) and s for s in skip):
        raise ValueError(f"convert_sync_batchnorm: skip holds non-empty name prefixes (got {skip!r})")
    if not isinstance(module, torch.nn.Module):
        raise ValueError(f"convert_sync_batchnorm: an nn.Module is expected (got {type(module).__name__})")

    def skipped(name):
        return any(name == s or name.startswith(s + ".") for s in skip)

    def swapped(m):
        if type(m) is torch.nn.BatchNorm2d and m.momentum is not None and m.num_features % 4 == 0:
            m = _swap_class(m, BatchNorm2d)
        if type(m) is BatchNorm2d:
            new = _swap_class(m, SyncBatchNorm2d)
            new.process_group = process_group
            return new
        return None

    root = None if skipped("") else swapped(module)
    if root is not None:
        return root, [""]
    names = []
    for pname, parent in list(module.named_modules()):
        for cname, child in list(parent.named_children()):
            name = f"{pname}.{cname}" if pname else cname
            new = None if skipped(name) else swapped(child)
            if new is not None:
                setattr(parent, cname, new)
                names.append(name)
    return module, names
