// omni_upsample_bwd.hip — the backward of the decoder's exact 2x bilinear up-sampling (omni_upsample_bilinear_f32 with Ho = 2H, Wo = 2W,
// align_corners=False) as a GATHER.  fp32 NHWC, C a multiple of 4.
//
// Per axis, output o reads source coordinate max(0, (o + 0.5) / 2 - 0.5): the weights are the constants 0.25 and 0.75, and 1 where the
// coordinate is clamped (o = 0) or the second tap falls on the first (o = 2H - 1).  Turned round, input i receives
//     0.25 g[2i-1] (i >= 1),   0.75 g[2i] (1 . g[0] at i = 0),   0.75 g[2i+1] (1 . g[2H-1] at i = H-1),   0.25 g[2i+2] (i <= H-2);
// at H = 1 both outputs carry weight 1.  The 2-D weight is the product of the two axes' (exact in fp32: multiples of 1/16).  One thread
// handles four channels of one input pixel and adds its at most 4 x 4 taps in (row, column) order: no atomics, the same bits on every run.
#include "omni_internal.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// the taps of input i on an axis of n inputs: output indices o0 .. o0 + cnt - 1, weights w[0 .. cnt)
__device__ __forceinline__ void up2_taps(int i, int n, int& o0, int& cnt, float (&w)[4])
{
    const bool lo = i >= 1, hi = i <= n - 2;
    o0 = lo ? 2 * i - 1 : 0;
    const float near = hi ? 0.75f : 1.0f, far = hi ? 0.25f : 0.0f;     // the taps 2i+1 and 2i+2
    w[0] = lo ? 0.25f : 1.0f;                                          // (selects, no indexed writes: the arrays stay in registers)
    w[1] = lo ? 0.75f : near;
    w[2] = lo ? near : far;
    w[3] = lo ? far : 0.0f;
    cnt = 2 + (lo ? 1 : 0) + (hi ? 1 : 0);
}

__global__ __launch_bounds__(256) void up2_bilinear_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, size_t total, int H, int W,
                                                               int C)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = C / 4;
    const int c = (int)(i % c4) * 4;
    size_t r = i / c4;
    const int ix = (int)(r % W); r /= W;
    const int iy = (int)(r % H);
    const size_t m = r / H;
    int oy0, ny, ox0, nx;
    float wy[4], wx[4];
    up2_taps(iy, H, oy0, ny, wy);
    up2_taps(ix, W, ox0, nx, wx);
    const size_t Ho = (size_t)2 * H, Wo = (size_t)2 * W;
    f4v acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a < ny) {
            const float* row = g + ((m * Ho + oy0 + a) * Wo + ox0) * C + c;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b < nx) {
                    const f4v v = *reinterpret_cast<const f4v*>(row + (size_t)b * C);
                    const float w = wy[a] * wx[b];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += w * v[e];
                }
            }
        }
    }
    *reinterpret_cast<f4v*>(dx + ((m * H + iy) * (size_t)W + ix) * C + c) = acc;
}

}  // namespace

extern "C" int omni_upsample_bilinear2x_bwd_f32(const float* g, float* dx, int M, int H, int W, int C, omni_stream_t stream)
{
    if (!g || !dx) OMNI_FAIL(OMNI_ERR_INVALID, "omni_upsample_bilinear2x_bwd: null pointer");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_upsample_bilinear2x_bwd: M, H, W >= 1");
    if (C <= 0 || C % 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_upsample_bilinear2x_bwd: channels must be a positive multiple of 4");
    if (H > 0x3fffffff || W > 0x3fffffff) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_upsample_bilinear2x_bwd: 2H and 2W must fit an int");
    const size_t total = (size_t)M * H * W * (C / 4), blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_upsample_bilinear2x_bwd: too many elements for one launch");
    hipLaunchKernelGGL(up2_bilinear_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, dx, total, H, W, C);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
