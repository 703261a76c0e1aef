"""The guided (edge-aware) smoothness term of the self-supervised objective — mirror of the reference's supervision/smoothness.py:3-8.

    loss = guided_smoothness_loss(input_duv, guide_duv, mask, weights)          # the reference's name and signature, over precomputed maps
         = sum(where(mask, input_duv * exp(-guide_duv) * weights, 0)) / sum(mask)

    loss = depth_smoothness(depth, image, mask, weights=None, sgrid=None)       # the fused form: a 0-d float32 tensor on the device
         = guided_smoothness_loss(dV_dxyz(coords_3d(sgrid, depth)), dI_duv(image), mask, weights)

depth, mask and weights are [B,1,H,W], image is [B,C,H,W], sgrid is any [1,2,H,W] grid (None: spherical.grid.default_sgrid(H, W), which is
create_spherical_grid(W) when H == W // 2).  weights may also be [1,1,H,W] (spherical_confidence(sgrid)); None means 1.  Everything numeric
runs in libomnifusion_hip.so (csrc/omni_smoothness.hip): depth_smoothness is ONE tiled pass over depth, image, mask and weights
(no vertex, difference or magnitude map is written) and ONE gather kernel for d loss / d depth; nothing is copied to the host.  The sums are
taken in a fixed order without atomics: two runs give the same bits.  depth_smoothness is differentiable w.r.t. depth only,
guided_smoothness_loss w.r.t. input_duv only; any other argument requiring grad raises.

Masks may be bool, uint8 or float; an element is valid where it is non-zero.  The mask SELECTS: nothing at a masked pixel — a NaN depth, an
infinite weight — reaches the sum through that pixel's own term (the reference multiplies the zeroed term by the weight, so its 0 * inf is
NaN).  A masked pixel's depth still enters the differences of its left and upper neighbours, as in the reference.
sum(mask) == 0 gives the reference's 0 / 0 = NaN (and NaN gradients); it is not special-cased.
Kinks, as torch autograd: d|x|/dx = 0 at 0 (every last-column du and last-row dv, by replicate padding), and the gradient of the 2-norm is
0 where the norm is 0 (the bottom-right pixel).
"""
import torch

from .. import _lib
from .._lib import ptr as _p
from ..spherical.grid import default_sgrid, direction_factors


def _f32(t):
    return t.contiguous().to(torch.float32)


def _mask32(mask):
    return mask.contiguous() if mask.dtype == torch.float32 else (mask != 0).to(torch.float32).contiguous()


def _workspace(nbytes, device):
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)


class _DepthSmoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, image, mask, weights, fac):
        lib = _lib.load()
        B, C, H, W = image.shape
        ws = _workspace(lib.omni_depth_smoothness_workspace_bytes(B, H, W), depth.device)
        loss = torch.empty(1, dtype=torch.float32, device=depth.device)
        with torch.cuda.device(depth.device):
            _lib.check(lib.omni_depth_smoothness_f32(_p(depth), _p(image), _p(mask), _p(weights), _p(fac), B, C, H, W, _p(ws), _p(loss),
                                                     _lib.stream_of(depth)), "depth_smoothness")
        ctx.save_for_backward(depth, image, mask, weights, fac, ws)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        depth, image, mask, weights, fac, ws = ctx.saved_tensors
        lib = _lib.load()
        B, C, H, W = image.shape
        g = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(depth)
        with torch.cuda.device(depth.device):
            _lib.check(lib.omni_depth_smoothness_grad_f32(_p(depth), _p(image), _p(mask), _p(weights), _p(fac), B, C, H, W, _p(ws), _p(g), _p(grad),
                                                          _lib.stream_of(depth)), "depth_smoothness backward")
        return grad, None, None, None, None


class _GuidedSmoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_duv, guide_duv, mask, weights):
        lib = _lib.load()
        n = input_duv.numel()
        ws = _workspace(lib.omni_guided_smoothness_workspace_bytes(n), input_duv.device)
        loss = torch.empty(1, dtype=torch.float32, device=input_duv.device)
        with torch.cuda.device(input_duv.device):
            _lib.check(lib.omni_guided_smoothness_f32(_p(input_duv), _p(guide_duv), _p(mask), _p(weights), n, _p(ws), _p(loss),
                                                      _lib.stream_of(input_duv)), "guided_smoothness_loss")
        ctx.save_for_backward(guide_duv, mask, weights, ws)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        guide_duv, mask, weights, ws = ctx.saved_tensors
        g = grad_out.contiguous().to(torch.float32)
        grad = torch.empty_like(guide_duv)
        with torch.cuda.device(guide_duv.device):
            _lib.check(_lib.load().omni_guided_smoothness_grad_f32(_p(guide_duv), _p(mask), _p(weights), guide_duv.numel(), _p(ws), _p(g), _p(grad),
                                                                   _lib.stream_of(guide_duv)), "guided_smoothness_loss backward")
        return grad, None, None, None


def _check_common(named, first):
    """named: ((tensor, name), ...), the differentiable one first."""
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    frozen = [name for t, name in named[1:] if t.requires_grad]
    if frozen:
        raise ValueError(f"the smoothness term is differentiable w.r.t. {first} only: {', '.join(frozen)} must not require grad")
    for t, name in named:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    dev = named[0][0].device
    if any(t.device != dev for t, _ in named):
        raise ValueError(", ".join(name for _, name in named) + " must live on the same device")


def guided_smoothness_loss(input_duv, guide_duv, mask, weights):
    """-> 0-d float32 tensor on the device; differentiable w.r.t. input_duv.  guide_duv, mask and weights broadcast to input_duv's shape."""
    _check_common(((input_duv, "input_duv"), (guide_duv, "guide_duv"), (mask, "mask"), (weights, "weights")), "input_duv")
    if input_duv.numel() == 0 or not input_duv.is_floating_point() or not guide_duv.is_floating_point() or not weights.is_floating_point():
        raise ValueError(f"input_duv, guide_duv and weights must be non-empty floating-point tensors (got input_duv of shape {tuple(input_duv.shape)})")
    try:
        guide_duv, mask, weights = (t.expand(input_duv.shape) for t in (guide_duv, mask, weights))
    except RuntimeError:
        raise ValueError(f"guide_duv, mask and weights must have (or broadcast to) the shape of input_duv {tuple(input_duv.shape)} "
                         f"(got {tuple(guide_duv.shape)}, {tuple(mask.shape)}, {tuple(weights.shape)})") from None
    return _GuidedSmoothness.apply(_f32(input_duv), _f32(guide_duv), _mask32(mask), _f32(weights))


def depth_smoothness(depth, image, mask, weights=None, sgrid=None):
    """-> 0-d float32 tensor on the device; one forward launch pair, one backward launch; differentiable w.r.t. depth."""
    named = [(depth, "depth"), (image, "image"), (mask, "mask")] + ([(weights, "weights")] if weights is not None else [])
    _check_common(tuple(named), "depth")
    if depth.dim() != 4 or depth.shape[1] != 1 or depth.numel() == 0:
        raise ValueError(f"depth must be a non-empty [B,1,H,W] tensor (got shape {tuple(depth.shape)})")
    B, _, H, W = depth.shape
    if image.dim() != 4 or image.shape[1] < 1 or (image.shape[0], image.shape[2], image.shape[3]) != (B, H, W):
        raise ValueError(f"image must be [B,C,H,W] with the B, H, W of depth {tuple(depth.shape)} (got shape {tuple(image.shape)})")
    if mask.shape != depth.shape:
        raise ValueError(f"depth and mask must have the same shape [B,1,H,W] (got {tuple(depth.shape)}, {tuple(mask.shape)})")
    if weights is not None and tuple(weights.shape) not in ((B, 1, H, W), (1, 1, H, W)):
        raise ValueError(f"weights must be [B,1,H,W] or [1,1,H,W] for depth {tuple(depth.shape)} (got shape {tuple(weights.shape)})")
    if not depth.is_floating_point() or not image.is_floating_point() or (weights is not None and not weights.is_floating_point()):
        raise ValueError("depth, image and weights must be floating-point tensors")
    if sgrid is None:
        sgrid = default_sgrid(H, W, depth.device)
    else:
        if not isinstance(sgrid, torch.Tensor) or tuple(sgrid.shape) != (1, 2, H, W):
            raise ValueError(f"sgrid must be a [1,2,H,W] tensor for depth {tuple(depth.shape)} (got {tuple(sgrid.shape) if isinstance(sgrid, torch.Tensor) else type(sgrid).__name__})")
        if sgrid.requires_grad:
            raise ValueError("the smoothness term is differentiable w.r.t. depth only: sgrid must not require grad")
    fac = direction_factors(sgrid, depth.device)
    w = None if weights is None else _f32(weights.expand(depth.shape))
    return _DepthSmoothness.apply(_f32(depth), _f32(image), _mask32(mask), w, fac)
