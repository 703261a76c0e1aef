"""Shared plumbing of the free-view samplers (equi2pers_torch.py, pers2equi_torch.py, views_to_erp): argument checks, the per-view
rotation tables and the launches of csrc/omni_freeview.hip and csrc/omni_freeview_bwd.hip.  Nothing here computes a sample: there is
no CPU / PyTorch path.  The plain mirrors refuse an input that requires grad; equi_pers/differentiable.py holds the autograd functions
(same launches, allow_grad=True, and the launch_*_bwd functions below).

The two rotation tables of a set of angles (forward R2.R1, inverse R2^-1 | R1^-1; omni_freeview_rotations, float64 rounded once) are
built on the host and copied to the device the first time a (theta, phi, device) is seen, then kept (the last 64 sets).  A later call
with the same angles launches its kernel and nothing else, so it can be captured into a graph on one stream after one warm-up call.
Angles given as a device tensor are read back on every call (one synchronisation): pass them on the host where that matters.
"""
import collections

import torch

from .. import _lib
from .._lib import ptr as _p

_TABLES = collections.OrderedDict()          # (theta bytes, phi bytes, device) -> (rot_fwd [N,9], rot_inv [N,18]) on the device
_TABLES_MAX = 64


NO_BACKWARD = "the plain free-view mirrors have no backward; the differentiable operators are omnifusion_amd.equi_pers.differentiable"


def check_image(name, t, ndim=4, allow_grad=False):
    """A float32 tensor on the GPU; unless allow_grad, one that does not require grad (the plain mirrors have no backward)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype}); float16 storage is not implemented for free-view sampling")
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dimensions (got shape {tuple(t.shape)})")
    if not allow_grad and t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} requires grad: {NO_BACKWARD}")
    if t.numel() == 0:
        raise ValueError(f"{name} is empty")


def check_view(hFOV, wFOV, h, w):
    hFOV, wFOV, h, w = float(hFOV), float(wFOV), int(h), int(w)
    if not (0.0 < hFOV < 180.0 and 0.0 < wFOV < 180.0):
        raise ValueError(f"hFOV and wFOV must lie in (0, 180) degrees (got {hFOV}, {wFOV})")
    if h < 2 or w < 2:
        raise ValueError(f"an image needs at least 2 x 2 pixels (got {h} x {w})")
    return hFOV, wFOV, h, w


def angles(theta, phi):
    """theta, phi (sequences or tensors of degrees, one per view) -> two float32 CPU tensors of equal length N >= 1."""
    out = []
    for name, a in (("theta", theta), ("phi", phi)):
        if isinstance(a, torch.Tensor) and a.requires_grad:
            raise NotImplementedError(f"{name} requires grad: free-view sampling has no gradient with respect to the angles")
        a = torch.as_tensor(a).detach().to("cpu", torch.float32).reshape(-1).contiguous()
        if not bool(torch.isfinite(a).all()):
            raise ValueError(f"{name} must be finite")
        out.append(a)
    if out[0].numel() != out[1].numel():
        raise ValueError(f"theta and phi must have one entry per view each (got {out[0].numel()} and {out[1].numel()})")
    if out[0].numel() < 1:
        raise ValueError("at least one view is needed")
    return out


def rotations(theta, phi):
    """-> (rot_fwd [N,3,3], rot_inv [N,2,3,3]) float32 CPU tensors: R2.R1, and (R2^-1, R1^-1), of the reference's `rotation_matrix`."""
    theta, phi = angles(theta, phi)
    n = theta.numel()
    fwd = torch.empty(n, 3, 3, dtype=torch.float32)
    inv = torch.empty(n, 2, 3, 3, dtype=torch.float32)
    _lib.check(_lib.load().omni_freeview_rotations(_p(theta), _p(phi), n, _p(fwd), _p(inv)), "freeview rotations")
    return fwd, inv


def tables(theta, phi, device):
    theta, phi = angles(theta, phi)
    key = (theta.numpy().tobytes(), phi.numpy().tobytes(), str(device))
    hit = _TABLES.get(key)
    if hit is not None:
        _TABLES.move_to_end(key)
        return hit
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("free-view sampling: these angles are new to this device and their rotation table cannot be uploaded while "
                           "a graph is being captured; run the call once before capturing")
    fwd, inv = rotations(theta, phi)
    hit = (fwd.reshape(-1, 9).to(device), inv.reshape(-1, 18).to(device))
    _TABLES[key] = hit
    while len(_TABLES) > _TABLES_MAX:
        _TABLES.popitem(last=False)
    return hit


def launch_equi2pers(equi_img, hFOV, wFOV, theta, phi, h, w, layout, allow_grad=False):
    check_image("equi_img", equi_img, allow_grad=allow_grad)
    hFOV, wFOV, h, w = check_view(hFOV, wFOV, h, w)
    B, C, H, W = equi_img.shape
    check_view(hFOV, wFOV, H, W)
    fwd, _ = tables(theta, phi, equi_img.device)
    N = fwd.shape[0]
    equi_img = equi_img.detach().contiguous()
    shape = (B, N, C, h, w) if layout == _lib.LAYOUT_BNCHW else (B, C, h, N * w)
    pers = torch.empty(shape, dtype=torch.float32, device=equi_img.device)
    with torch.cuda.device(equi_img.device):
        _lib.check(_lib.load().omni_freeview_equi2pers_f32(_p(equi_img), _p(pers), _p(fwd), B, C, H, W, N, h, w, hFOV, wFOV, layout,
                                                           _lib.stream_of(equi_img)), "freeview equi2pers")
    return pers


def launch_pers2equi(pers_img, hFOV, wFOV, theta, phi, H, W, allow_grad=False):
    """-> (erp [N,C,H,W] float32, mask [N,1,H,W] uint8)"""
    check_image("pers_img", pers_img, allow_grad=allow_grad)
    hFOV, wFOV, H, W = check_view(hFOV, wFOV, H, W)
    N, C, h, w = pers_img.shape
    check_view(hFOV, wFOV, h, w)
    _, inv = tables(theta, phi, pers_img.device)
    if inv.shape[0] != N:
        raise ValueError(f"pers_img holds {N} views but theta / phi name {inv.shape[0]}")
    pers_img = pers_img.detach().contiguous()
    erp = torch.empty((N, C, H, W), dtype=torch.float32, device=pers_img.device)
    mask = torch.empty((N, 1, H, W), dtype=torch.uint8, device=pers_img.device)
    with torch.cuda.device(pers_img.device):
        _lib.check(_lib.load().omni_freeview_pers2equi_f32(_p(pers_img), _p(erp), _p(mask), _p(inv), N, C, h, w, H, W, hFOV, wFOV,
                                                           _lib.stream_of(pers_img)), "freeview pers2equi")
    return erp, mask


def views_to_erp(pers, hFOV, wFOV, theta, phi, H, W, allow_grad=False):
    """N views merged onto one panorama per batch item (no reference counterpart).

        erp, count = views_to_erp(pers, hFOV, wFOV, theta, phi, H, W)      # pers [B,N,C,h,w] -> erp [B,C,H,W], count [1,1,H,W] uint8

    erp = sum_v sample_v mask_v / max(sum_v mask_v, 1) with the per-view samples and masks of pers2equi_torch.pers2equi, views summed in
    index order; count = sum_v mask_v, the number of views that cover a pixel (the same for every batch item).  One kernel; the N
    per-view panoramas are never written."""
    check_image("pers", pers, ndim=5, allow_grad=allow_grad)
    hFOV, wFOV, H, W = check_view(hFOV, wFOV, H, W)
    B, N, C, h, w = pers.shape
    check_view(hFOV, wFOV, h, w)
    _, inv = tables(theta, phi, pers.device)
    if inv.shape[0] != N:
        raise ValueError(f"pers holds {N} views but theta / phi name {inv.shape[0]}")
    if N > 255:
        raise ValueError("views_to_erp merges at most 255 views")
    pers = pers.detach().contiguous()
    erp = torch.empty((B, C, H, W), dtype=torch.float32, device=pers.device)
    count = torch.empty((1, 1, H, W), dtype=torch.uint8, device=pers.device)
    with torch.cuda.device(pers.device):
        _lib.check(_lib.load().omni_freeview_merge_f32(_p(pers), _p(erp), _p(count), _p(inv), B, N, C, h, w, H, W, hFOV, wFOV,
                                                       _lib.stream_of(pers)), "freeview views_to_erp")
    return erp, count


# ---------------------------------------------------------------------------------------------------------------- backward launches
# Each takes the upstream gradient of the forward's output (float32, contiguous, on the device), allocates the gradient and the workspace
# as torch tensors and launches on the current stream; the rotation tables are the forward's (cached: nothing is uploaded).
def _bwd(op, grad_out, shape, images, call):
    lib = _lib.load()
    grad_in = torch.empty(shape, dtype=torch.float32, device=grad_out.device)
    nbytes = lib.omni_freeview_bwd_workspace_bytes(op, images, shape[-3], shape[-2], shape[-1])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=grad_out.device)
    with torch.cuda.device(grad_out.device):
        call(lib, grad_in, ws, _lib.stream_of(grad_out))
    return grad_in


def launch_equi2pers_bwd(grad_pers, erp_shape, hFOV, wFOV, theta, phi, h, w, layout):
    """grad_pers ([B,N,C,h,w] or [B,C,h,N*w], as `layout`) -> grad_equi_img [B,C,H,W]"""
    B, C, H, W = erp_shape
    fwd, _ = tables(theta, phi, grad_pers.device)
    N = fwd.shape[0]

    def call(lib, grad_erp, ws, stream):
        _lib.check(lib.omni_freeview_equi2pers_bwd_f32(_p(grad_pers), _p(grad_erp), _p(fwd), B, C, H, W, N, h, w, hFOV, wFOV, layout, _p(ws), stream),
                   "freeview equi2pers backward")
    return _bwd(0, grad_pers, (B, C, H, W), B, call)


def launch_pers2equi_bwd(grad_erp, pers_shape, hFOV, wFOV, theta, phi, H, W):
    """grad_erp [N,C,H,W] -> grad_pers_img [N,C,h,w]"""
    N, C, h, w = pers_shape
    _, inv = tables(theta, phi, grad_erp.device)

    def call(lib, grad_pers, ws, stream):
        _lib.check(lib.omni_freeview_pers2equi_bwd_f32(_p(grad_erp), _p(grad_pers), _p(inv), N, C, h, w, H, W, hFOV, wFOV, _p(ws), stream),
                   "freeview pers2equi backward")
    return _bwd(1, grad_erp, (N, C, h, w), N, call)


def launch_views_to_erp_bwd(grad_erp, pers_shape, hFOV, wFOV, theta, phi, H, W):
    """grad_erp [B,C,H,W] -> grad_pers [B,N,C,h,w]"""
    B, N, C, h, w = pers_shape
    _, inv = tables(theta, phi, grad_erp.device)

    def call(lib, grad_pers, ws, stream):
        _lib.check(lib.omni_freeview_merge_bwd_f32(_p(grad_erp), _p(grad_pers), _p(inv), B, N, C, h, w, H, W, hFOV, wFOV, _p(ws), stream),
                   "freeview views_to_erp backward")
    return _bwd(2, grad_erp, (B, N, C, h, w), B * N, call)


def cubemap_views():
    """-> (theta, phi): the six cube faces (front, right, back, left, up, down) as view angles in degrees; use hFOV = wFOV = 90."""
    return (torch.tensor([0.0, 90.0, 180.0, -90.0, 0.0, 0.0], dtype=torch.float32),
            torch.tensor([0.0, 0.0, 0.0, 0.0, 90.0, -90.0], dtype=torch.float32))
