"""The separable tap sum of csrc/omni_up2_tapsum.h — the one text that up2_taps_fused_kernel (csrc/omni_conv_up2_taps.hip) and up2_heads_taps_kernel
(csrc/omni_conv_up2_heads_taps.hip) both run — restated in float64 with the header's own weight tables, clamps and tap order, against the operator
`conv2d(interpolate(x, 2, bilinear), w, pad 1)`.  This is the specification the header is read against:

  vertical stage, per tap (ky, kx), on the thread's own column:
      S_kx[i][ay][j] (+)= hy[ay + ky] * Y[clamp(i - 1 + r)][j] + ly[ay + ky] * Y[clamp(i + r)][j],            r = (ay + ky) >> 1
  horizontal stage, once per kx after its three ky taps:
      out[2i + ay][2j + bx] += hx[bx + kx] * S_kx[i][ay][clamp(j - 1 + c)] + lx[bx + kx] * S_kx[i][ay][clamp(j + c)],   c = (bx + kx) >> 1
  taps kx-major: 0, 3, 6, 1, 4, 7, 2, 5, 8.

15 multiply-adds per output element and channel (9 vertical, 6 horizontal) instead of the 36 of the tap-by-tap bilinear sum."""
import numpy as np
import pytest
import torch

from _up2_taps_ref import direct, tap_products

TAP_ORDER = (0, 3, 6, 1, 4, 7, 2, 5, 8)


def tables(k, n):
    """(h[0..3], l[0..3]) of low-resolution index k in a map of n: weights of up-sampled index 2k + u - 1 on the pair (clamp(k - 1 + (u >> 1)), clamp(k + (u >> 1))):
    0.75 / 0.25, zero where 2k + u - 1 is outside the up-sampled map, 1.0 / 0.0 where the pair is clamped at the low edge."""
    lo, hi = k == 0, k == n - 1
    h = [0.0 if lo else 0.75, 1.0 if lo else 0.25, 0.75, 0.0 if hi else 0.25]
    l = [0.0 if lo else 0.25, 0.0 if lo else 0.75, 0.25, 0.0 if hi else 0.75]
    return h, l


def sep_tap_sum(y):
    """Y [Hl, Wl, 9, C] float64 -> [2Hl, 2Wl, C]: the two-stage sum, in the kernel's order of operations"""
    Hl, Wl, _, C = y.shape
    out = np.zeros((2 * Hl, 2 * Wl, C))
    cl = lambda v, n: min(max(v, 0), n - 1)
    for g in range(3):                                             # one kx group: taps TAP_ORDER[3g .. 3g + 2]
        S = np.zeros((Hl, 2, Wl, C))
        for tp in TAP_ORDER[3 * g:3 * g + 3]:
            ky, kx = divmod(tp, 3)
            assert kx == g
            for i in range(Hl):
                hy, ly = tables(i, Hl)
                for ay in range(2):
                    uy = ay + ky
                    r = uy >> 1
                    S[i, ay] += hy[uy] * y[cl(i - 1 + r, Hl), :, tp] + ly[uy] * y[cl(i + r, Hl), :, tp]
        for j in range(Wl):
            hx, lx = tables(j, Wl)
            for bx in range(2):
                ux = bx + g
                c = ux >> 1
                out[0::2, 2 * j + bx] += hx[ux] * S[:, 0, cl(j - 1 + c, Wl)] + lx[ux] * S[:, 0, cl(j + c, Wl)]
                out[1::2, 2 * j + bx] += hx[ux] * S[:, 1, cl(j - 1 + c, Wl)] + lx[ux] * S[:, 1, cl(j + c, Wl)]
    return out


@pytest.mark.parametrize("hw", [(8, 32), (16, 16), (3, 5)], ids=["band_8x32", "image_16x16", "odd_3x5"])
def test_two_stage_sum_is_the_operator(hw):
    """the kernel's two forms (one band that holds both edges, a whole image) and a map off every tile size, edges included: 1e-12 of float64"""
    Hl, Wl = hw
    C, Co = 5, 4
    g = torch.Generator().manual_seed(27)
    x = torch.randn(1, Hl, Wl, C, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64)
    ref = direct(x, w)[0].numpy()
    got = sep_tap_sum(tap_products(x, w)[0].numpy())
    d = np.abs(got - ref).max()
    print(f"{hw}: max |two-stage - conv2d(interpolate)| = {d:.3g}, ref max {np.abs(ref).max():.3g}")
    assert d < 1e-12


def test_tables_are_the_bilinear_weights():
    """the tables against the index arithmetic of align_corners=False up-sampling: src = max(0.5 (p + 0.5) - 0.5, 0), l = frac(src)"""
    for n in (3, 8, 16):
        for k in range(n):
            h, l = tables(k, n)
            for u in range(4):
                p = 2 * k + u - 1
                if p < 0 or p >= 2 * n:
                    assert h[u] == 0.0 and l[u] == 0.0
                    continue
                src = max(0.5 * (p + 0.5) - 0.5, 0.0)
                i0 = int(np.floor(src)); frac = src - i0
                i1 = min(i0 + 1, n - 1)
                pair = (min(max(k - 1 + (u >> 1), 0), n - 1), min(max(k + (u >> 1), 0), n - 1))
                want = np.zeros(n); want[i0] += 1.0 - frac; want[i1] += frac
                have = np.zeros(n); have[pair[0]] += h[u]; have[pair[1]] += l[u]
                assert np.array_equal(want, have), (n, k, u)
