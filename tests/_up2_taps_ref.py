"""float64 restatement of `conv3x3(upsample2x(x))` as tap products on the low-resolution map (tests/test_up2_taps_*.py):
tap-major repack, nine 1x1 products, up-sampling of each product, shifted sum with zero outside the up-sampled map."""
import torch
import torch.nn.functional as F


def taps_repack(w):
    """[Cout, Cin, 3, 3] -> [9*Cout, Cin], row t*Cout + co = w[co, :, ky, kx] with t = ky*3 + kx (the layout of `<name>.taps.w16`)"""
    return w.permute(2, 3, 0, 1).reshape(9 * w.shape[0], w.shape[1])


def tap_products(x, w):
    """x [M, Hl, Wl, Cin], w [Cout, Cin, 3, 3] -> Y [M, Hl, Wl, 9, Cout] in float64"""
    y = x.double() @ taps_repack(w.double()).t()
    return y.reshape(*x.shape[:3], 9, w.shape[0])


def tap_sum(y, bias=None, relu=False):
    """Y [M, Hl, Wl, 9, Cout] -> bias + sum_t [q + t - 1 inside] up2(Y_t)[q + t - 1], [M, 2Hl, 2Wl, Cout] in float64"""
    M, Hl, Wl, _, Co = y.shape
    planes = y.double().permute(0, 3, 4, 1, 2).reshape(M, 9 * Co, Hl, Wl)
    up = F.interpolate(planes, scale_factor=2, mode="bilinear", align_corners=False).reshape(M, 9, Co, 2 * Hl, 2 * Wl)
    up = F.pad(up, (1, 1, 1, 1))                                  # taps outside the up-sampled map contribute nothing
    out = torch.zeros((M, Co, 2 * Hl, 2 * Wl), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += up[:, ky * 3 + kx, :, ky:ky + 2 * Hl, kx:kx + 2 * Wl]
    if bias is not None:
        out += bias.double()[None, :, None, None]
    if relu:
        out = F.relu(out)
    return out.permute(0, 2, 3, 1).contiguous()


def direct(x, w, bias=None, relu=False):
    """the operator itself: F.conv2d(F.interpolate(x, 2x, bilinear, align_corners=False), w, padding=1), NHWC in and out, float64"""
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    out = F.conv2d(up, w.double(), None if bias is None else bias.double(), padding=1)
    return (F.relu(out) if relu else out).permute(0, 2, 3, 1).contiguous()
