// omni_area.h — cv2.INTER_AREA sampling shared by the input kernels (omni_io.hip: plain preprocess; omni_augment.hip: the same arithmetic
// behind the augmentation's column map).  One definition, so that both units round to the same bits.  gfx950 only.
#pragma once
#include "omni_internal.h"

// ------------------------------------------------------------------ cv2.INTER_AREA
// OpenCV's area resampling of a down-scale by (sx, sy) = (src / dst): output pixel d covers the source interval
// [d*s, (d+1)*s); every source pixel contributes with the length of its overlap, normalised by min(s, src - d*s)
// (resize.cpp `computeResizeAreaTab`).  For an integer scale this is the plain box average.  uint8 images are averaged in float and
// rounded to nearest-even back to uint8 (saturate_cast<uchar>(float) = cvRound), BEFORE the loader's /255.
// The oracle (oracle/io_ref.py) restates the same published algorithm; cv2 itself is not installed here: parity unpinned.
struct AreaSpan { int i0, i1; float w0, w1, inv; };   // full cells [i0, i1) weight 1, partial cells i0-1 (w0) and i1 (w1), 1/cell width

__device__ __forceinline__ AreaSpan area_span(int d, float scale, int ssize)
{
    const float fs1 = (float)d * scale, fs2 = fminf(fs1 + scale, (float)ssize);
    const float cell = fminf(scale, (float)ssize - fs1);
    AreaSpan s;
    s.i0 = (int)ceilf(fs1); s.i1 = (int)floorf(fs2);
    if (s.i1 > ssize) s.i1 = ssize;
    if (s.i0 > s.i1) s.i0 = s.i1;
    s.w0 = (float)s.i0 - fs1;                          // overlap with cell i0-1 (0 when aligned)
    s.w1 = fs2 - (float)s.i1;                          // overlap with cell i1
    if (s.w0 < 1e-3f) s.w0 = 0.0f;                     // OpenCV drops overlaps <= 1e-3
    if (s.w1 < 1e-3f) s.w1 = 0.0f;
    s.inv = 1.0f / cell;
    return s;
}

// area average of channel c at destination pixel (y, x); src interleaved [Hs][Ws][C] of SrcT
template <typename SrcT>
__device__ __forceinline__ float area_sample(const SrcT* __restrict__ src, int Hs, int Ws, int C, int c, const AreaSpan& sy, const AreaSpan& sx)
{
    float acc = 0.0f;
    auto row = [&](int yy, float wy) {
        const SrcT* r = src + (size_t)yy * Ws * C + c;
        float a = 0.0f;
        if (sx.w0 > 0.0f) a += (float)r[(size_t)(sx.i0 - 1) * C] * sx.w0;
        for (int xx = sx.i0; xx < sx.i1; ++xx) a += (float)r[(size_t)xx * C];
        if (sx.w1 > 0.0f) a += (float)r[(size_t)sx.i1 * C] * sx.w1;
        acc += a * wy;
    };
    if (sy.w0 > 0.0f) row(sy.i0 - 1, sy.w0);
    for (int yy = sy.i0; yy < sy.i1; ++yy) row(yy, 1.0f);
    if (sy.w1 > 0.0f) row(sy.i1, sy.w1);
    return acc * (sx.inv * sy.inv);
}

// back to uint8 as OpenCV does it: saturate_cast (nearest-even); its 2x2 fast path computes (a + b + c + d + 2) >> 2 (half up)
__device__ __forceinline__ float area_round_u8(float avg, bool half_up)
{
    return fminf(255.0f, fmaxf(0.0f, half_up ? floorf(avg + 0.5f) : rintf(avg)));
}
