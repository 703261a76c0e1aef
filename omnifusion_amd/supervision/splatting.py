"""render — host-side mirror of /root/reference/supervision/splatting.py:73-80 (forward bilinear splatting), on the device.

    recon, mask = render(img, depth, coords, max_depth=20.0)     # img [B,C,H,W], depth [B,1,H,W], coords [B,2,H,W] (u = column, v = row)

Same name, arguments and values as the reference: each source pixel splats img * w and w (w = 1 / exp(2 depth / max_depth)) onto
the four pixels around (u, v) with bilinear weights (corners off the image, and corner weights below 1e-3, are dropped); then
recon = sum(img * w) / sum(w) and mask = sum(w) > 1e-3 (a bool tensor [B,1,H,W]).  Everything runs in libomnifusion_hip.so
(csrc/omni_dibr.hip): one pre-pass, one splat kernel with 64-bit fixed-point integer atomics, one normalise kernel.  Unlike the
reference's fp32 scatter_add the sums do not depend on the order of arrival: the result is the same bits on every run.

Differentiable like the reference's: if img, depth or coords requires grad, recon carries a hand-written backward (a gather kernel,
no atomics: every source pixel re-derives its corners and reads its targets) that produces only the gradients asked
for; mask is not differentiable.  Without a grad-requiring input the forward path is the inference one, launch for launch.
`render_to` (:83-88) is not provided.  Divergences: DESIGN.md §7 (d5, NaN poisoning; d6, depth-0 gradients).
"""
import torch

from .. import _lib
from .._lib import ptr as _p


def _check(name, t, ndim=4):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.requires_grad and not t.is_cuda:
        raise ValueError(f"{name} requires grad but is not on an MI355X device: the backward, like the forward, has no CPU path")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions [B,.,H,W] (got shape {tuple(t.shape)})")


def grad_needs_device(**tensors):
    """A CPU tensor that requires grad is refused first and by that name: there is no CPU path, forward or backward."""
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad and not t.is_cuda:
            raise ValueError(f"{name} requires grad but is not on an MI355X device: the backward, like the forward, has no CPU path")


def check_image_depth(img, depth):
    """Validate img [B,C,H,W] and depth [B,1,H,W] (GPU float32); returns B, C, H, W."""
    _check("img", img)
    _check("depth", depth)
    B, C, H, W = img.shape
    if depth.shape != (B, 1, H, W):
        raise ValueError(f"depth must be [B,1,H,W] = {(B, 1, H, W)} (got {tuple(depth.shape)})")
    if depth.device != img.device:
        raise ValueError("img and depth must live on the same device")
    if B < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError("empty tensor")
    return B, C, H, W


def run(img, depth, want_mask, launch, want_wt=False):
    """Allocate recon / mask / workspace (and the weight sum, for a backward) on img's device and call
    `launch(lib, recon, mask, wt, workspace, stream)`."""
    lib = _lib.load()
    B, C, H, W = img.shape
    recon = torch.empty((B, C, H, W), dtype=torch.float32, device=img.device)
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=img.device) if want_mask else None
    wt = torch.empty((B, 1, H, W), dtype=torch.float32, device=img.device) if want_wt else None
    ws = torch.empty(lib.omni_dibr_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=img.device)
    with torch.cuda.device(img.device):
        launch(lib, recon, mask, wt, ws, _lib.stream_of(img))
    mask = mask.view(torch.bool) if want_mask else None
    return (recon, mask, wt) if want_wt else (recon, mask)


def run_backward(img, grad_recon, needs, launch):
    """Allocate the requested gradients (needs: name -> shape or None) and the record workspace; call
    `launch(lib, grad_recon, grads, workspace, stream)`; returns the dict of gradients (None where not requested)."""
    lib = _lib.load()
    B, C, H, W = img.shape
    grads = {k: (torch.empty(shape, dtype=torch.float32, device=img.device) if shape is not None else None) for k, shape in needs.items()}
    ws = torch.empty(lib.omni_dibr_bwd_workspace_bytes(B, C, H, W), dtype=torch.uint8, device=img.device)
    g = grad_recon.contiguous().to(torch.float32)
    with torch.cuda.device(img.device):
        launch(lib, g, grads, ws, _lib.stream_of(img))
    return grads


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, depth, coords, max_depth):
        B, C, H, W = img.shape

        def launch(lib, recon, mask, wt, ws, stream):
            _lib.check(lib.omni_splat_render_wt_f32(_p(img), _p(depth), _p(coords), float(max_depth), _p(recon), _p(mask), _p(wt),
                                                    B, C, H, W, _p(ws), stream), "splatting.render")
        recon, mask, wt = run(img, depth, True, launch, want_wt=True)
        ctx.save_for_backward(img, depth, coords, recon, wt)
        ctx.max_depth = float(max_depth)
        ctx.mark_non_differentiable(mask)
        return recon, mask

    @staticmethod
    def backward(ctx, grad_recon, _grad_mask):
        img, depth, coords, recon, wt = ctx.saved_tensors
        B, C, H, W = img.shape
        needs = dict(img=img.shape if ctx.needs_input_grad[0] else None, depth=depth.shape if ctx.needs_input_grad[1] else None,
                     coords=coords.shape if ctx.needs_input_grad[2] else None)

        def launch(lib, g, grads, ws, stream):
            _lib.check(lib.omni_splat_render_bwd_f32(_p(g), _p(recon), _p(wt), _p(img), _p(depth), _p(coords), ctx.max_depth,
                                                     _p(grads["img"]), _p(grads["depth"]), _p(grads["coords"]), B, C, H, W, _p(ws), stream),
                       "splatting.render backward")
        grads = run_backward(img, grad_recon, needs, launch)
        return grads["img"], grads["depth"], grads["coords"], None


def render(img, depth, coords, max_depth=20.0):
    grad_needs_device(img=img, depth=depth, coords=coords)
    B, C, H, W = check_image_depth(img, depth)
    _check("coords", coords)
    if coords.shape != (B, 2, H, W):
        raise ValueError(f"coords must be [B,2,H,W] = {(B, 2, H, W)} (got {tuple(coords.shape)})")
    if coords.device != img.device:
        raise ValueError("coords must live on img's device")
    img, depth, coords = img.contiguous(), depth.contiguous(), coords.contiguous()

    if torch.is_grad_enabled() and (img.requires_grad or depth.requires_grad or coords.requires_grad):
        return _Render.apply(img, depth, coords, max_depth)

    def launch(lib, recon, mask, wt, ws, stream):
        _lib.check(lib.omni_splat_render_f32(_p(img), _p(depth), _p(coords), float(max_depth), _p(recon), _p(mask),
                                             B, C, H, W, _p(ws), stream), "splatting.render")
    return run(img, depth, True, launch)
