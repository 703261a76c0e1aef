"""ssim_loss — host-side mirror of the reference's supervision/ssim.py:86-90, on the device.

    ssim = ssim_loss(prediction, groundtruth, kernel_size=5, std=1.5, mode='gaussian')      # the SSIM map, [B,C,H,W]

Same name, arguments and values as the reference: 'gaussian' is the zero-padded depthwise Gaussian window (:23-63), 'box' the valid
average (AvgPool2d, stride 1) with the map zero-padded back to [H,W] (:65-84).  One kernel of libomnifusion_hip.so
(csrc/omni_photometric.hip): a tile of both images with its halo is staged in LDS once and the window runs separably over the five
moments; the sums are fp64.  Odd windows 3 .. 11.  Forward only: the differentiable entry is photometric.calculate_loss.
"""
import ctypes
import math

import torch

from .. import _lib
from .._lib import ptr as _p

MODES = {"gaussian": 0, "box": 1}


def window_weights(kernel_size, std, mode):
    """The 1-D window as (ctypes float array, mode code).  Gaussian: exp(-(x - k//2)^2 / (2 std^2)) normalised in float64, stored as
    float32 (ssim.py:9-12); box: 1/k.  Raises ValueError for an even or out-of-range window or an unknown mode."""
    if mode not in MODES:
        raise ValueError(f"unknown SSIM mode {mode!r}: 'gaussian' or 'box'")
    k = int(kernel_size)
    if k != kernel_size or k < 3 or k > 11 or k % 2 == 0:
        raise ValueError(f"the SSIM window must be odd and within 3 .. 11 (got {kernel_size})")
    if mode == "gaussian":
        if not (std > 0.0 and math.isfinite(std)):
            raise ValueError("std must be finite and > 0")
        g = [math.exp(-(x - k // 2) ** 2 / float(2 * std ** 2)) for x in range(k)]
        total = sum(g)
        g = [v / total for v in g]
    else:
        g = [1.0 / k] * k
    return (ctypes.c_float * k)(*g), MODES[mode]


def check_pair(prediction, groundtruth, names=("prediction", "groundtruth")):
    for name, t in zip(names, (prediction, groundtruth)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must be a tensor on an MI355X device; there is no CPU path")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (got {t.dtype})")
        if t.dim() != 4 or t.numel() == 0:
            raise ValueError(f"{name} must be a non-empty [B,C,H,W] tensor (got shape {tuple(t.shape)})")
    if prediction.shape != groundtruth.shape:
        raise ValueError(f"{names[0]} and {names[1]} must have the same shape (got {tuple(prediction.shape)} and {tuple(groundtruth.shape)})")
    if prediction.device != groundtruth.device:
        raise ValueError(f"{names[0]} and {names[1]} must live on the same device")
    return prediction.shape


def ssim_loss(prediction, groundtruth, kernel_size=5, std=1.5, mode='gaussian'):
    win, code = window_weights(kernel_size, std, mode)
    B, C, H, W = check_pair(prediction, groundtruth)
    if prediction.requires_grad or groundtruth.requires_grad:
        raise ValueError("ssim_loss is forward only; the differentiable entry is supervision.photometric.calculate_loss")
    if code == 1 and (H < kernel_size or W < kernel_size):
        raise ValueError("the box window does not fit the image")
    x, y = prediction.contiguous(), groundtruth.contiguous()
    out = torch.empty_like(x)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.omni_ssim_f32(_p(x), _p(y), B, C, H, W, int(kernel_size), win, code, _p(out), _lib.stream_of(x)), "ssim_loss")
    return out
