// omni_heads_hr.h — the first half of the fused heads and its record `hr`, shared by its two writers, conv3x3_up2_g1_kernel<HEADS> (omni_conv_up2.hip) and
// up2_heads_taps_kernel (omni_conv_up2_heads_taps.hip), and by its reader, heads_finish_kernel (omni_conv_up2.hip).  Device side: a constant, a forceinline helper and a macro.
//
// The `pred` / `weight_pred` heads (3x3, 32 -> 1 each) of de_conv4_0's output x, out[q] = sum_{dy,dx} w[dy][dx] . x[q + (dy,dx)], turned around: pixel p
// contributes w[dy][dx] . x[p] to q = p - (dy,dx) — eighteen 32-channel dot products per pixel (9 taps x 2 heads), which are ONE matrix product per 32-pixel
// row segment: rows = (dy, head, dx) in the order of omni_heads_pack_f16x3, k = the 32 channels in the order a lane's accumulator quads hold them, three f16x3
// terms = 6 matrix instructions (heads_product).  The three dx terms of a row are summed across neighbouring lanes in the fixed order dx = -1, 0, +1, which
// leaves per tile row and (dy, head) 34 partial sums — pixels -1 .. 32: the two outer ones belong to the neighbouring tiles' pixels (OMNI_HEADS_HR_WRITE).
// The record (tile = 4 output rows x 32 pixels, tiles in image order [m][tile row][tile column]):
//   hr [tile][row 4][(dy, head) 6][HR_PITCH floats: 32 sums | pixel -1 | pixel 32 | 2 pad]
// 3.4 KB per tile.  heads_finish_kernel adds the three rows (dy) and the neighbour tiles' outer sums in a fixed order.
#pragma once
#include "omni_conv_sh_common.h"

namespace {

constexpr int HR_PITCH = 36;                                 // floats per (tile row, (dy, head)) record of `hr`: 32 sums, pixel -1, pixel 32, 2 of padding (16-byte rows)

// hwf: the lane's fragments of heads.w16f [hi kc0, hi kc1, lo kc0, lo kc1]; ph / pl: hi and lo of the lane's pixel, k chunks 0 and 1 -> d0 = hi . hi,
// d1 = lo . hi + hi . lo (the value is d0 + 2^-11 d1)
__device__ __forceinline__ void heads_product(const h8v (&hwf)[4], const h8v (&ph)[2], const h8v (&pl)[2], f16v& d0, f16v& d1)
{
    d0 = (f16v)(0.0f); d1 = (f16v)(0.0f);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
        d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[kc], ph[kc], d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[2 + kc], ph[kc], d1, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[kc], pl[kc], d1, 0, 0, 0);
    }
}

}  // namespace

// d0, d1 (heads_product) of one 32-pixel row segment -> its row group HP = hr + (tile * 4 + row) * (6 * HR_PITCH); PX = lane & 31, H = lane >> 5.
// Matrix rows (reg & 3) + 8 (reg >> 2) + 4 h: register group g = 0..2 is (dy, head) pair g + 3h, its registers 0..2 are dx = -1, 0, +1.
// A macro, not a function: as a function (by value or by reference, with the address formed inside or outside) hipcc compiles conv3x3_up2_g1_kernel<HEADS>
// to 2 instructions more than in place — tests/test_precision_f16x1.py pins that kernel's instruction count — and up2_heads_taps_kernel to 30 more.
#define OMNI_HEADS_HR_WRITE(D0, D1, HP, PX, H) \
    _Pragma("unroll") \
    for (int g_ = 0; g_ < 3; ++g_) { \
        const float tl_ = fmaf((D1)[4 * g_], 4.8828125e-4f, (D0)[4 * g_]), tc_ = fmaf((D1)[4 * g_ + 1], 4.8828125e-4f, (D0)[4 * g_ + 1]), \
                    tr_ = fmaf((D1)[4 * g_ + 2], 4.8828125e-4f, (D0)[4 * g_ + 2]); \
        /* out[q] takes w[dx] . x[q + dx]: its dx = -1 term comes from pixel q - 1, its dx = +1 term from pixel q + 1 */ \
        const float fl_ = __shfl_up(tl_, 1, 32), fr_ = __shfl_down(tr_, 1, 32); \
        const float sum_ = (((PX) > 0 ? fl_ : 0.0f) + tc_) + ((PX) < 31 ? fr_ : 0.0f); \
        float* rowp_ = (HP) + (g_ + 3 * (H)) * HR_PITCH; \
        rowp_[PX] = sum_; \
        if ((PX) == 0) rowp_[32] = tr_;                      /* pixel -1 of this row (the left neighbour tile's column 31) takes my dx = +1 term */ \
        if ((PX) == 31) rowp_[33] = tl_;                     /* pixel 32 takes my dx = -1 term */ \
    }
