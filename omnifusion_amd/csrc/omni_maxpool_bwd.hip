// omni_maxpool_bwd.hip — the backward of the encoder's 3x3, stride-2, padding-1 max-pool (omni_maxpool3x3s2_f32) as a GATHER
// (DESIGN.md §22).  fp32 NHWC, C a multiple of 4.
//
// One thread handles four channels of a 2 x 2 block of INPUT pixels, rows 2a, 2a+1 and columns 2b, 2b+1.  The windows that contain them
// are oy in {a, a+1} x ox in {b, b+1} (those past the last window dropped); together they cover the 5 x 5 input pixels from (2a-1, 2b-1),
// which the thread reads once — 6.25 reads per pixel where a thread per pixel makes 20.  For each window, in (oy, ox) order, it recomputes
// the winner from x and adds the window's g to the pixel of the block that is the winner, if one is: a pixel of an even row or column
// lies in one window along that axis, of an odd one in two, so every pixel adds its at most 2 x 2 windows in (oy, ox) order.  The winner
// is the FIRST greatest element in (ky, kx) scan order over the taps inside the map — torch's rule, `val > maxval` — which decides where
// the gradient of a window of equal values goes: the pool's input is a ReLU output and whole windows of exact zeros are common.  A NaN
// never compares greater, so it wins only as the first tap of a window with nothing greater than -inf behind it (the forward's fmaxf
// drops it the same way).  No index map is stored, no atomics: every dx element is written once, from sums in a fixed order.
#include <cmath>

#include "omni_internal.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void pool3x3s2_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ dx,
                                                            size_t total, int H, int W, int C, int Ho, int Wo, int A, int B)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = C / 4;
    const int c = (int)(i % c4) * 4;
    size_t r = i / c4;
    const int b = (int)(r % B); r /= B;
    const int a = (int)(r % A);
    const size_t m = r / A;
    const int y0 = 2 * a - 1, x0 = 2 * b - 1;
    f4v v[5][5];
    bool in[5][5];
#pragma unroll
    for (int p = 0; p < 5; ++p)
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int yy = y0 + p, xx = x0 + q;
            in[p][q] = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            v[p][q] = f4v{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (in[p][q]) v[p][q] = *reinterpret_cast<const f4v*>(x + ((m * H + yy) * (size_t)W + xx) * C + c);
        }
    f4v acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int wy = 0; wy < 2; ++wy)
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
            const int oy = a + wy, ox = b + wx;
            if (oy >= Ho || ox >= Wo) continue;
            f4v best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int win[4] = {-1, -1, -1, -1};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if (in[2 * wy + ky][2 * wx + kx]) {
                        const f4v t = v[2 * wy + ky][2 * wx + kx];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool gt = t[e] > best[e];
                            if (gt || win[e] < 0) win[e] = ky * 3 + kx;          // (win < 0: the first tap inside the map)
                            if (gt) best[e] = t[e];
                        }
                    }
                }
            const f4v gv = *reinterpret_cast<const f4v*>(g + ((m * Ho + oy) * (size_t)Wo + ox) * C + c);
            // the block's pixel (dy, dx) is tap (dy + 1 - 2 wy, dx + 1 - 2 wx) of this window where that lies in 0 .. 2
#pragma unroll
            for (int dy = wy; dy < 2; ++dy)
#pragma unroll
                for (int dxx = wx; dxx < 2; ++dxx) {
                    const int mine = (dy + 1 - 2 * wy) * 3 + (dxx + 1 - 2 * wx);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[dy][dxx][e] += win[e] == mine ? gv[e] : 0.0f;
                }
        }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dxx = 0; dxx < 2; ++dxx) {
            const int iy = 2 * a + dy, ix = 2 * b + dxx;
            if (iy < H && ix < W) *reinterpret_cast<f4v*>(dx + ((m * H + iy) * (size_t)W + ix) * C + c) = acc[dy][dxx];
        }
}

}  // namespace

extern "C" int omni_maxpool3x3s2_bwd_f32(const float* g, const float* x, float* dx, int M, int H, int W, int C, omni_stream_t stream)
{
    if (!g || !x || !dx) OMNI_FAIL(OMNI_ERR_INVALID, "omni_maxpool3x3s2_bwd: null pointer");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_maxpool3x3s2_bwd: M, H, W >= 1");
    if (C <= 0 || C % 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_maxpool3x3s2_bwd: channels must be a positive multiple of 4");
    const int A = H / 2 + H % 2, B = W / 2 + W % 2;                        // 2 x 2 pixel blocks per axis
    const size_t total = (size_t)M * A * B * (C / 4), blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_maxpool3x3s2_bwd: too many elements for one launch");
    hipLaunchKernelGGL(pool3x3s2_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, x, dx, total, H, W, C, (H - 1) / 2 + 1,
                       (W - 1) / 2 + 1, A, B);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
